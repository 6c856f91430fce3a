"""Spiral arms (S), the radial laws `Moffat` and `Ferrer` (R) and everything in one model (X: a boxy Ferrer with a
spiral and modes, a pixel-integrated Sersic, a Moffat, a tilted sky) on the fields of
tests/test_gpu_extra_image_fields.py, which their own test files never use: several PSFs with a free index, a mask,
NaN `sci` and bad `ivm` pixels on both sides of the Ferrer's cut-off, rectangular shapes both ways, hipFFT's
rectangular shapes, passes of two (the spiral block at aux_base + 12 n_sersic and the radial block at aux_base +
18 n_sersic behind a pass offset), `linear_accumulation` 1, a field set with a plain, a modes-only, a spiral and a law
field in four registration orders with row-based calls through every view, a joint fit, and the samplers with a free
index.  Everything is held to tests/extra_contract.py, which tests/test_extra_image_contract.py pins on the CPU.

Structure, helpers and bounds are those of tests/test_gpu_extra_image_fields.py: the raw model per pixel to
`RAW_BOUND` (1e-11; 1e-10 where a pixel-integrated component is in the model) -- by `law_error` where the model has a
Ferrer, whose pixels next to the cut-off are judged relative to Sigma_0 --, the five images to
`test_gpu_random.image_tol`, log-likelihoods and log-posteriors to 1e-9 |ll|."""
import numpy as np
import pytest

import extra_contract as xc
import test_gpu_random as tgr
from test_gpu_extra_image_fields import FIXED_MODES, check_ll
from test_gpu_general_components import RAW_BOUND

pytestmark = pytest.mark.gpu


def raw_bound(kind):
    return 1e-10 if kind == 'X' else RAW_BOUND


def check_raw(model, got, want, bound, tag):
    """want: `contract_with_state`'s tuple of the walker.  The condition on the inputs first (no compared pixel of a
    Ferrer within EDGE_MARGIN of its cut-off), then the error as the model is judged."""
    assert want[3] >= xc.EDGE_MARGIN, (tag, want[3])
    err = xc.judge_raw(model, got, want[1]['raw_model'], want[2], tag)
    assert err <= bound, (tag, err)
    return err


def slot_of(kind, law):
    return [s.get('law') for s in xc.KINDS[kind]['sersics']].index(law)


# -- (a) several PSFs with a free index, on masked fields with bad pixels ---------------------------------------------
@pytest.mark.parametrize('backend,kind,shape', xc.LAW_CASES, ids=xc.case_id)
def test_several_psfs_with_a_free_index(backend, kind, shape):
    """tests/test_gpu_extra_image_fields.py's test of this name, step for step, for S, R and X: six distinct walkers
    in passes of two whose PSF_Index values cover every PSF, 0.4 and 1.5 and an index outside the support, on a field
    with a mask, NaN `sci` and bad `ivm` pixels (R, X: inside and outside the Ferrer's support; X: one in the
    integrated box).  log_posterior_batch against contract + log_priors_batch; an index outside the support is -inf
    and leaves the others' bits unchanged; sample_images of one walker per PSF from ONE call: the raw model finite at
    every pixel, the bad ones included, and the five images; log_likelihood_batch through the host's rows."""
    case, field = xc.law_case(kind, shape)
    xc.field_features(case, field, xc.integrated_centre(kind, shape))
    n_psf = xc.N_PSF[shape]
    model = xc.make_model(case, backend=backend, max_walkers=8, **xc.KINDS[kind])
    assert model._backend == backend and model.param_names[-1] == 'PSF_Index'
    thetas = xc.several_psf_thetas(model, shape)
    index = np.array(xc.psf_indices(n_psf))
    inside = (np.rint(index) >= 0) & (np.rint(index) < n_psf)
    want = [xc.contract_with_state(model, field, t) for t in thetas]
    tag = '%s %s %dx%d' % ((backend, kind) + shape)
    assert tgr.several_passes(model, len(thetas)) == 2
    lp = model.log_posterior_batch(thetas)
    prior = model.log_priors_batch(thetas)
    worst_ll = 0.0
    for w in range(len(thetas)):
        if not inside[w]:
            assert want[w][0] == -np.inf and prior[w] == -np.inf and lp[w] == -np.inf, (tag, w, lp[w])
        else:
            worst_ll = max(worst_ll, check_ll(lp[w], want[w][0] + prior[w], want[w][0], (tag, w)))
    assert len(np.unique(lp[inside])) == inside.sum()
    # the same batch with the outside walkers moved onto PSF 0: the others' bits do not change
    moved = thetas.copy()
    moved[~inside, -1] = 0.0
    again = model.log_posterior_batch(moved)
    assert np.all(np.isfinite(again)) and np.array_equal(again[inside], lp[inside]), tag
    # one walker per PSF in one call: index 0.4 -> PSF 0, 1.0 -> PSF 1, 1.5 -> PSF 2 where there are three
    pick = [2, 1] + ([3] if n_psf == 3 else [])
    assert [int(np.rint(index[w])) for w in pick] == list(range(n_psf))
    dev = model.sample_images(thetas[pick])
    worst_raw = max(check_raw(model, dev['raw_model'][j], want[w], raw_bound(kind), (tag, w)) for j, w in enumerate(pick))
    tgr.check_images(dev, [want[w][1] for w in pick], tag)
    ll_rows = model.log_likelihood_batch(thetas)
    for w in np.flatnonzero(inside):
        worst_ll = max(worst_ll, check_ll(ll_rows[w], want[w][0], want[w][0], (tag, 'rows', w)))
    print('%s: worst raw-model error %.2e, worst log-likelihood relative error %.2e' % (tag, worst_raw, worst_ll))
    model.close()


# -- (b) a field set of every keyword kind ----------------------------------------------------------------------------
FIXED_ARMS = dict(r_in=2.0, r_out=9.0, winding=150.0, inclination=35.0, sky_angle=20.0)
SET_FIELDS = {'P': ((96, 70), dict(sersics=[{}, {}])),
              'F': ((64, 64), dict(sersics=[dict(fourier=FIXED_MODES), {}])),
              'S': ((70, 96), dict(sersics=[dict(boxiness=0.6, spiral=FIXED_ARMS), {}])),
              'R': ((64, 128), dict(sersics=[dict(law='moffat'), dict(law=('ferrer', dict(beta=0.5)), boxiness=0.6)]))}


@pytest.mark.parametrize('order', ['PFSR', 'RSFP', 'SPRF', 'FRPS'])
def test_field_set_of_every_keyword_kind(order):
    """A plain 96x70 field, a modes-only 64x64 field, a boxy spiral 70x96 field and a 64x128 field with a Moffat and a
    boxy Ferrer (the keywords' values fixed: 19 free parameters each), two PSFs each, in four registration orders:
    the context's auxiliary width grows in up to three steps, every keyword-bearing kind registers first once and
    last once, and the plain field sits at each end and in the middle.  The shared context (96 x 128) is taller and
    wider than at least two fields.  As test_field_set_with_two_psfs_per_field: against each field's contract (1e-9);
    against its own context within 1e-12 of the largest value, bit-identical where the transform shapes agree; a field
    alone in the call bitwise equal to the same field in the full call; and for EVERY field the row-based calls
    through its view -- `sample_images` (the raw model per pixel, the five images) and `log_likelihood_batch` --
    against the contract: the views of the fields whose own auxiliary rows are shorter than the context's."""
    from psfmc_amd.models import FieldSet
    specs = [(k,) + SET_FIELDS[k] for k in order]
    ferrer_at = lambda kind, shape: xc.scene(shape)[2][1]['xy'] if kind == 'R' else None
    cases = [xc.field_case(shape, 800 + shape[1] + 3 * shape[0], 2, box_at=ferrer_at(kind, shape)) for kind, shape, _ in specs]
    fields = [xc.oracle_field(c) for c in cases]
    for c, f, (kind, shape, _) in zip(cases, fields, specs):
        xc.field_features(c, f, ferrer_at(kind, shape))
    fs = FieldSet([xc.make_model(c, max_walkers=1, **kw) for c, (_, _, kw) in zip(cases, specs)], max_walkers=32)
    own = [xc.make_model(c, max_walkers=16, **kw) for c, (_, _, kw) in zip(cases, specs)]
    thetas = [np.array([xc.theta_of(m, *xc.scene(shape, i)[:2], xc.scene(shape, i)[2][:2], psf=float(p))
                        for i, p in enumerate((0, 1, 1, 0))]) for m, (_, shape, _) in zip(own, specs)]
    assert fs.num_params == 19 and all(t.shape == (4, 19) for t in thetas)
    ny, nx = int(fs.context.get_option('transform_ny')), int(fs.context.get_option('transform_nx'))
    assert sum(s[0] < ny for _, s, _ in specs) >= 2 and sum(s[1] < nx for _, s, _ in specs) >= 2
    got = fs.log_posterior_batch(thetas)
    transform = fs.context.get_option('transform_ny'), fs.context.get_option('transform_nx')
    for f, (kind, shape, _) in enumerate(specs):
        tag = '%s field %d (%s %dx%d)' % ((order, f, kind) + shape)
        alone = [None] * 4
        alone[f] = thetas[f]
        assert np.array_equal(fs.log_posterior_batch(alone)[f], got[f]), tag
        prior = fs.models[f].log_priors_batch(thetas[f])
        want = [xc.contract_with_state(own[f], fields[f], t) for t in thetas[f]]
        worst_ll = max(check_ll(got[f][i], want[i][0] + prior[i], want[i][0], (tag, i)) for i in range(4))
        mine = own[f].log_posterior_batch(thetas[f])
        assert np.abs(got[f] - mine).max() <= 1e-12 * np.abs(mine).max(), tag
        imgs = fs.models[f].sample_images(thetas[f][:2])
        a = imgs['raw_model']
        b = own[f].sample_images(thetas[f][:2], ('raw_model',))['raw_model']
        assert a.shape == (2,) + shape and np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), tag
        if (own[f].engine.get_option('transform_ny'), own[f].engine.get_option('transform_nx')) == transform:
            assert np.array_equal(got[f], mine) and np.array_equal(a, b), tag
        worst_raw = max(check_raw(own[f], a[i], want[i], RAW_BOUND, (tag, i)) for i in range(2))
        tgr.check_images(imgs, [w[1] for w in want[:2]], tag)
        ll_rows = fs.models[f].log_likelihood_batch(thetas[f])
        worst_ll = max([worst_ll] + [check_ll(ll_rows[i], want[i][0], want[i][0], (tag, 'rows', i)) for i in range(4)])
        print('%s: worst raw-model error %.2e, worst log-likelihood relative error %.2e' % (tag, worst_raw, worst_ll))
    fs.close()
    for m in own:
        m.close()


# -- (c) a joint fit ----------------------------------------------------------------------------------------------------
def check_field_sums(model, thetas, imgs, tag):
    """A field's posterior sums of these walkers against the contract's means, on the contract's finite pixels, at the
    bound of test_joint_fit_with_two_psfs_per_exposure (1e-11 of the largest value, the weight map as a variance)."""
    model.reset_images()
    model.accumulate_samples(thetas)
    post = model.collect_posterior_images()
    with np.errstate(all='ignore'):
        for kind in ('raw_model', 'convolved_model', 'residual', 'point_source_subtracted'):
            mean = np.mean([w[kind] for w in imgs], axis=0)
            fin = np.isfinite(mean)
            assert np.array_equal(np.isfinite(post[kind]), fin), (tag, kind)
            assert np.max(np.abs(post[kind][fin] - mean[fin])) <= 1e-11 * np.max(np.abs(mean[fin])), (tag, kind)
        var = np.mean([1 / w['composite_ivm'] for w in imgs], axis=0)
        fin = np.isfinite(var)
        assert np.array_equal(np.isfinite(1 / post['composite_ivm']), fin), tag
        assert np.max(np.abs(1 / post['composite_ivm'][fin] - var[fin])) <= 1e-11 * np.max(np.abs(var[fin])), tag


def test_joint_fit_of_spiral_and_law_exposures():
    """Two exposures, 64x64 and 70x96, two PSFs each: a boxy Moffat with a spiral, a boxy Ferrer and a tilted sky; the
    positions, the Ferrer's r_out and the PSF index per field, everything else -- the spiral's and the laws' own
    parameters among them -- shared.  The four walkers take the four combinations of the two exposures' PSFs.  The
    joint log-posterior is the sum of the contract log-likelihoods + log_priors_batch (1e-9); one walker alone equals
    itself in the batch bit for bit; each field's posterior sums against the contract's means on its finite
    pixels."""
    from psfmc_amd import JointModel
    shapes = [(64, 64), (70, 96)]
    kw = dict(sersics=[dict(law='moffat', boxiness=xc.FREE, spiral=xc.ARMS), dict(law='ferrer', boxiness=xc.FREE)],
              slope=xc.FREE, extent=96)
    cases = [xc.field_case(s, 900 + s[1], 2, box_at=xc.scene(s)[2][1]['xy']) for s in shapes]
    fields = [xc.oracle_field(c) for c in cases]
    for c, f, s in zip(cases, fields, shapes):
        xc.field_features(c, f, xc.scene(s)[2][1]['xy'])
    joint = JointModel([xc.make_model(c, max_walkers=1, **kw) for c in cases],
                       per_field=['1_PointSource_xy', '2_Moffat_xy', '3_Ferrer_xy', '3_Ferrer_r_out'], max_walkers=16)
    own = [xc.make_model(c, max_walkers=1, **kw) for c in cases]
    names = joint.param_names
    assert names[-2:] == ['PSF_Index_f0', 'PSF_Index_f1'] and '3_Ferrer_r_out_f1' in names
    for shared in ('2_Moffat_beta', '3_Ferrer_beta', '3_Ferrer_alpha', '2_Moffat_spiral_wind', '2_Moffat_spiral_r_out'):
        assert names.count(shared) == 1, shared
    own_names = sum(([n] * w for n, w in zip(own[1].param_names, own[1].param_lens)), [])
    thetas = np.zeros((4, joint.num_params))
    for f in (1, 0):
        th = np.array([xc.theta_of(own[f], *xc.scene(shapes[f], i)[:2], xc.scene(shapes[f], i)[2][:2],
                                   psf=float((i // 2, i % 2)[f])) for i in range(4)])
        if f == 1:
            th[:, own_names.index('3_Ferrer_r_out')] += 1.5                 # the exposures' own r_out differ
        thetas[:, joint.field_columns(f)] = th
    got = joint.log_posterior_batch(thetas)
    prior = joint.log_priors_batch(thetas)
    want = [[xc.contract_with_state(own[f], fields[f], joint.field_theta(t, f)[0]) for t in thetas] for f in range(2)]
    r_out = [joint.field_theta(thetas, f)[:, own_names.index('3_Ferrer_r_out')] for f in range(2)]
    assert np.allclose(r_out[1] - r_out[0], 1.5)
    worst = 0.0
    for i in range(4):
        assert min(want[0][i][3], want[1][i][3]) >= xc.EDGE_MARGIN
        total = (want[0][i][0] + want[1][i][0]) + prior[i]
        worst = max(worst, check_ll(got[i], total, total, i))
    assert len(np.unique(got)) == 4
    assert joint.log_posterior_batch(thetas[2:3])[0] == got[2]
    print('joint fit: worst log-posterior relative error %.2e' % worst)
    for f, m in enumerate(joint.field_models):
        check_field_sums(m, joint.field_theta(thetas, f), [w[1] for w in want[f]], f)
    joint.close()


# -- (d) row-based calls in several passes -------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', xc.LAW_KINDS)
def test_row_based_calls_in_several_passes(kind):
    """Five walkers on the two PSFs of a 70x96 field -- the last one's Moffat (R, X) centred off the image:
    log_likelihood_batch and sample_images in passes of two (chunk_walkers 2: the pass offsets of the auxiliary
    rows, whose spiral and radial blocks lie behind the Fourier block) are bit-identical to the same calls with the
    library's own pass size and within bounds of the contract; accumulate_samples under linear_accumulation 1 (the
    route through k_raster_sums_extra) and 0 against the contract's means (`check_posterior_sums`)."""
    shape = (70, 96)
    case, field = xc.law_case(kind, shape)
    model = xc.make_model(case, max_walkers=8, **xc.KINDS[kind])
    n_s = len(xc.KINDS[kind]['sersics'])
    scenes = [xc.scene(shape, i) for i in range(5)]
    if kind != 'S':
        scenes[4][2][slot_of(kind, 'moffat')]['xy'] = (-3.6, shape[0] // 2 + 0.4)
    thetas = np.array([xc.theta_of(model, sky, ps, sersics[:n_s], psf=float(p))
                       for (sky, ps, sersics), p in zip(scenes, (0, 1, 1, 0, 1))])
    assert np.all(np.isfinite(model.log_priors_batch(thetas)))
    eng = model.engine
    assert eng.pass_size(5) > 2
    ll_one = model.log_likelihood_batch(thetas)
    img_one = model.sample_images(thetas)
    eng.set_option('chunk_walkers', 2)
    assert eng.pass_size(5) <= 2
    ll = model.log_likelihood_batch(thetas)
    img = model.sample_images(thetas)
    assert np.array_equal(ll, ll_one), kind
    for k in img:
        assert np.array_equal(img[k], img_one[k], equal_nan=True), (kind, k)
    want = [xc.contract_with_state(model, field, t) for t in thetas]
    worst_ll = max(check_ll(ll[i], want[i][0], want[i][0], (kind, i)) for i in range(5))
    worst_raw = max(check_raw(model, img['raw_model'][i], want[i], raw_bound(kind), (kind, i)) for i in range(5))
    refs = [w[1] for w in want]
    tgr.check_images(img, refs, kind)
    for linear in (1, 0):
        eng.set_option('linear_accumulation', linear)
        assert eng.get_option('linear_accumulation') == linear
        tgr.check_posterior_sums(model, thetas, refs, (kind, 'linear_accumulation', linear))
    print('rows %s 70x96: worst raw-model error %.2e, worst log-likelihood relative error %.2e' % (kind, worst_raw, worst_ll))
    model.close()


# -- (e) the samplers ------------------------------------------------------------------------------------------------------
def lean_model(n_max):
    """Sky + PointSource (a fixed position) + a boxy Ferrer with a spiral (its winding free; beta and r_out_b constants)
    + a Moffat (a fixed position and fwhm_b) on a 64x64 field with two PSFs and a free PSF_Index: 12 free parameters
    (24 walkers are an ensemble).  Returns (model, start [n_max, 12]: a ball about the scene, the index alternating)."""
    shape = (64, 64)
    case = xc.field_case(shape, 78, 2)
    arms = dict(r_in=2.0, r_out=9.0, winding=xc.FREE, inclination=35.0, sky_angle=20.0)
    model = xc.make_model(case, [dict(law=('ferrer', dict(beta=0.5, r_out_b=6.0)), boxiness=xc.FREE, spiral=arms),
                                 dict(law=('moffat', dict(xy=(33.6, 31.2), fwhm_b=2.5)))], max_walkers=n_max, lean=True)
    assert model.num_params == 12 and model.param_names[-1] == 'PSF_Index'
    assert model.sersic_radial_kinds == [2, 1] and model.sersic_spiral_flags == [True, False]
    sky, ps, sersics = xc.scene(shape)
    base = xc.theta_of(model, sky, ps, sersics[:2], psf=0.0)
    p0 = base + np.random.RandomState(2).normal(size=(n_max, len(base))) * 1e-2
    p0[:, -1] = np.arange(n_max) % 2
    assert np.all(np.isfinite(model.log_priors_batch(p0)))
    return model, p0


def test_device_sampler_with_a_free_psf_index():
    """24 walkers, 20 iterations: the device-resident chain equals the host loop's fed the device's own
    log-posteriors, bit for bit; some steps are accepted; every log-posterior the host loop saw is finite, or -inf
    exactly where a prior is -inf -- among them proposals whose index left the support."""
    from psfmc_amd.sampler import EnsembleSampler, DeviceEnsembleSampler
    n_w = 24
    model, p0 = lean_model(n_w)
    seen = []

    def lnpost(theta):
        out = model.log_posterior_batch(theta)
        seen.append((np.array(theta), out.copy()))
        return out
    host = EnsembleSampler(n_w, model.num_params, batch_lnpostfn=lnpost)
    dev = DeviceEnsembleSampler(n_w, model, block=7)
    for s in (host, dev):
        s.random_state = np.random.RandomState(8).get_state()
    list(host.sample(p0, iterations=20))
    list(dev.sample(p0, iterations=20))
    assert np.array_equal(dev.chain, host.chain) and np.array_equal(dev.naccepted, host.naccepted)
    assert np.array_equal(dev.lnprobability, host.lnprobability)
    assert dev.naccepted.sum() > 0 and np.all(np.isfinite(dev.lnprobability))
    theta = np.concatenate([t for t, _ in seen])
    lp = np.concatenate([v for _, v in seen])
    prior = model.log_priors_batch(theta)
    assert np.array_equal(np.isfinite(lp), np.isfinite(prior)) and np.all(lp[~np.isfinite(lp)] == -np.inf)
    left = ~((np.rint(theta[:, -1]) >= 0) & (np.rint(theta[:, -1]) <= 1))
    print('sampler: %d evaluations, %d with the index outside the support, %d accepted steps'
          % (len(lp), left.sum(), dev.naccepted.sum()))
    assert left.sum() > 0 and np.all(lp[left] == -np.inf)
    model.close()


def test_tempered_sampler_with_a_free_psf_index():
    """Four rungs of 24 walkers, ten iterations: chain, log-probabilities, log-likelihoods, acceptances and swaps equal
    the host contract's (tests/test_gpu_radial_laws.py compares them so)."""
    from psfmc_amd.sampler import TemperedEnsembleSampler, DeviceTemperedSampler, default_betas
    model, p0 = lean_model(4 * 24)
    betas = default_betas(4, 50.0)
    p0 = p0.reshape(4, 24, -1)
    host = TemperedEnsembleSampler(24, model.num_params, betas, model.log_likelihood_and_prior_batch)
    dev = DeviceTemperedSampler(24, model, betas=betas, block=4)
    for s in (host, dev):
        s.random_state = np.random.RandomState(11).get_state()
    list(host.sample(p0, iterations=10))
    list(dev.sample(p0, iterations=10))
    assert np.array_equal(dev.chain, host.chain)
    assert np.array_equal(dev.lnprobability, host.lnprobability)
    assert np.array_equal(dev.lnlikelihood, host.lnlikelihood)
    assert np.array_equal(dev.naccepted_t, host.naccepted_t) and np.array_equal(dev.nswap, host.nswap)
    assert np.all(np.isfinite(dev.lnlikelihood)) and dev.naccepted_t.sum() > 0
    assert len({0.0, 1.0} & set(np.rint(dev.chain[..., -1]).ravel())) == 2          # both PSFs stay in the chain
    model.close()
