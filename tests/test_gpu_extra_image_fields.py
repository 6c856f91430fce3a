"""The extra-image models -- pixel-integrated Sersic (I), boxiness + tilted sky (G), boxiness + Fourier modes (F) and a
mixed model (M) -- on the fields their own test files never use: several PSFs with a free index (so that a walker's PSF
index is NOT its field), a mask, NaN `sci` and bad `ivm` pixels, rectangular shapes both ways with the integrated
box clipped at every edge, field sets and joint fits with two PSFs per field and fields narrower AND shorter than
the shared context, row-based calls in several passes, and the sampler with a free index.  Everything is held to
tests/extra_contract.py, which tests/test_extra_image_contract.py pins to the oracle on the CPU.

Bounds are the project's own: the raw model per pixel to `RAW_BOUND` (1e-11; 1e-10 where a pixel-integrated component
is in the model), the five images to `test_gpu_random.image_tol`, log-likelihoods and log-posteriors to 1e-9 |ll|."""
import numpy as np
import pytest

import extra_contract as xc
import test_gpu_random as tgr
from test_gpu_general_components import RAW_BOUND

pytestmark = pytest.mark.gpu

LL_BOUND = 1e-9


def raw_bound(kind):
    """The default rasteriser's bound; the pixel-integrated profile's own where the model has one
    (tests/test_gpu_sersic_integrated.py assert_raw_matches)."""
    return 1e-10 if kind in ('I', 'M') else RAW_BOUND


def check_raw(got, want, bound, tag):
    err = xc.raw_error(got, want, tag)
    assert err <= bound, (tag, err)
    return err


def check_ll(got, want, scale, tag):
    assert np.isfinite(want) and np.isfinite(got), (tag, got, want)
    err = abs(got - want) / abs(scale)
    assert err <= LL_BOUND, (tag, got, want)
    return err


# -- (a) several PSFs with a free index, (b) on masked fields with bad pixels --------------------------------------
@pytest.mark.parametrize('backend,kind,shape', xc.CASES, ids=xc.case_id)
def test_several_psfs_with_a_free_index(backend, kind, shape):
    """Six distinct walkers in passes of two whose PSF_Index values cover every PSF, 0.4 and 1.5 (rounding, round
    half even) and an index outside the support.  The field has a mask, NaN `sci` and bad `ivm` pixels, one of them in
    the integrated component's 7x7 box (asserted).  64x128 / 128x64: unguarded power-of-two rows; 70x96 / 96x70:
    embedded (WRAP), rectangular both ways; 96x150: a built general side; 64x320: power tables; 64x1152:
    k_rows3_fwd; hipfft: k_raster.

    log_posterior_batch against contract + log_priors_batch; an index outside the support is -inf and leaves the
    others' bits unchanged; sample_images of one walker per PSF from ONE call: the raw model per pixel -- finite at
    every pixel, the bad ones included -- and the five images (finite masks equal the contract's, then
    `image_tol`); log_likelihood_batch through the host's rows."""
    case, field = xc.several_psf_case(kind, shape)
    xc.field_features(case, field, xc.integrated_centre(kind, shape))
    n_psf = xc.N_PSF[shape]
    model = xc.make_model(case, backend=backend, max_walkers=8, **xc.KINDS[kind])
    assert model._backend == backend and model.param_names[-1] == 'PSF_Index'
    thetas = xc.several_psf_thetas(model, shape)
    index = np.array(xc.psf_indices(n_psf))
    inside = (np.rint(index) >= 0) & (np.rint(index) < n_psf)
    want = [xc.contract_evaluate(model, field, t) for t in thetas]
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
    worst_raw = max(check_raw(dev['raw_model'][j], want[w][1]['raw_model'], raw_bound(kind), (tag, w))
                    for j, w in enumerate(pick))
    tgr.check_images(dev, [want[w][1] for w in pick], tag)
    ll_rows = model.log_likelihood_batch(thetas)
    for w in np.flatnonzero(inside):
        worst_ll = max(worst_ll, check_ll(ll_rows[w], want[w][0], want[w][0], (tag, 'rows', w)))
    print('%s: worst raw-model relative error %.2e, worst log-likelihood relative error %.2e' % (tag, worst_raw, worst_ll))
    model.close()


# -- (c) rectangular integrated boxes -------------------------------------------------------------------------------
def clipped_centres(shape):
    """Centres whose 7x7 box and refinement pixels are clipped in every way on a (ny, nx) image."""
    ny, nx = shape
    lo, hi = min(shape), max(shape)
    far = 0.5 * (lo + hi) + 0.3                 # on the long axis beyond the short one's length: lo + 3 < far < hi - 3
    assert lo + 3 < far < hi - 3
    along = (far, lo / 2 + 0.2) if nx > ny else (lo / 2 + 0.2, far)
    return [(1.3, ny / 2 + 0.2), (nx - 1.6, ny / 2 - 0.3),                              # clipped on x only
            (nx / 2 + 0.4, 0.8), (nx / 2 - 0.3, ny - 2.2),                              # on y only
            (0.7, 1.2), (nx - 1.4, 0.6), (1.1, ny - 1.3), (nx - 1.2, ny - 0.9),         # on both: the four corners
            (nx - 0.5, ny / 2 + 0.2), (nx / 2 + 0.4, ny - 0.5),                         # x + 1/2, y + 1/2 on the outer edge
            (nx - 1.5, ny - 1.5),                                                       # a pixel corner one pixel inside
            along, along[::-1]]                                                        # ... and transposed: off the image


BOX_CASES = [('fused', 'I', shape) for shape, _ in xc.FUSED_SHAPES] + [('fused', 'M', (70, 96)), ('hipfft', 'I', (64, 128))]


@pytest.mark.parametrize('backend,kind,shape', BOX_CASES, ids=xc.case_id)
def test_rectangular_integrated_boxes(backend, kind, shape):
    """The integrated component's centre at thirteen places of a rectangular field (two calls of at most 7 walkers,
    PSF 0 and PSF 1 alternating): clipped on x only, on y only, at the four corners, with x + 1/2 (y + 1/2) exactly
    on the last column's (row's) outer edge, on a pixel corner one pixel inside the far corner, on the long axis
    beyond the short axis' length (a swapped lx / ly clip drops or writes pixels there) and that point transposed.
    Raw model per pixel 1e-10, log-likelihood through the raw vectors and through the rows 1e-9."""
    case, field = xc.several_psf_case(kind, shape)
    model = xc.make_model(case, backend=backend, max_walkers=8, **xc.KINDS[kind])
    which = model.sersic_integrate.index(True)
    n_s = len(model.sersic_integrate)
    thetas = []
    for i, xy in enumerate(clipped_centres(shape)):
        sky, ps, sersics = xc.scene(shape)
        sersics = [dict(s) for s in sersics[:n_s]]
        sersics[which]['xy'] = xy
        thetas.append(xc.theta_of(model, sky, ps, sersics, psf=float(i % 2)))
    thetas = np.array(thetas)
    tag = '%s %s %dx%d' % ((backend, kind) + shape)
    worst_raw = worst_ll = 0.0
    for part in (slice(0, 7), slice(7, None)):
        th = thetas[part]
        raw = model.sample_images(th, ('raw_model',))['raw_model']
        lp = model.log_posterior_batch(th)
        prior = model.log_priors_batch(th)
        ll_rows = model.log_likelihood_batch(th)
        for j, t in enumerate(th):
            want_ll, want = xc.contract_evaluate(model, field, t)
            worst_raw = max(worst_raw, check_raw(raw[j], want['raw_model'], 1e-10, (tag, part.start + j)))
            worst_ll = max(worst_ll, check_ll(lp[j], want_ll + prior[j], want_ll, (tag, part.start + j)),
                           check_ll(ll_rows[j], want_ll, want_ll, (tag, 'rows', part.start + j)))
    print('%s: worst raw-model relative error %.2e, worst log-likelihood relative error %.2e' % (tag, worst_raw, worst_ll))
    model.close()


# -- (d) a field set: two PSFs per field, different shapes, different keywords ----------------------------------------
FIXED_MODES = {1: (0.2, 30.0), 3: (-0.15, 25.0), 4: (0.1, -100.0)}
SET_FIELDS = [((64, 64), 'F', dict(sersics=[dict(boxiness=0.6, fourier=FIXED_MODES), {}])),
              ((70, 96), 'I', dict(sersics=[{}, dict(integrate=True)], slope=(3e-4, -2e-4))),
              ((96, 70), 'P', dict(sersics=[{}, {}]))]


@pytest.mark.parametrize('order', [(0, 1, 2), (2, 1, 0)], ids=['modes-first', 'plain-first'])
def test_field_set_with_two_psfs_per_field(order):
    """A 64x64 field with boxiness and modes, a 70x96 field with a pixel-integrated SECOND Sersic and a tilted sky, and
    a plain 96x70 field (the keywords' values fixed: the same free parameters), each with two PSFs, in either
    registration order.  The shared context is taller than the 64x64 and the 70x96 field need and wider than the 64x64
    and the 96x70 one (lx < nx and ly < ny both occur), and a walker's PSF index is 2 field + PSF: not its field.  Each field's
    batch has walkers on PSF 0 and on PSF 1.  Against the field's own contract (1e-9); against its own context within
    1e-12 of the largest value, bit-identical where the transform shapes agree; a field alone in the call bitwise
    equal to the same field in the full call; the field's raw images through its view against the contract."""
    from psfmc_amd.models import FieldSet
    specs = [SET_FIELDS[i] for i in order]
    cases = [xc.field_case(shape, 800 + shape[1] + 3 * shape[0], 2,
                           box_at=xc.scene(shape)[2][1]['xy'] if kind == 'I' else None) for shape, kind, _ in specs]
    fields = [xc.oracle_field(c) for c in cases]
    for c, f, (shape, kind, _) in zip(cases, fields, specs):
        xc.field_features(c, f, xc.scene(shape)[2][1]['xy'] if kind == 'I' else None)
    fs = FieldSet([xc.make_model(c, max_walkers=1, **kw) for c, (_, _, kw) in zip(cases, specs)], max_walkers=32)
    own = [xc.make_model(c, max_walkers=16, **kw) for c, (_, _, kw) in zip(cases, specs)]
    thetas = [np.array([xc.theta_of(m, *xc.scene(shape, i)[:2], xc.scene(shape, i)[2][:2], psf=float(p))
                        for i, p in enumerate((0, 1, 1, 0))]) for m, (shape, _, _) in zip(own, specs)]
    assert fs.num_params == 19 and all(t.shape == (4, 19) for t in thetas)
    ny, nx = int(fs.context.get_option('transform_ny')), int(fs.context.get_option('transform_nx'))
    assert sum(s[0] < ny for s, _, _ in specs) >= 2 and sum(s[1] < nx for s, _, _ in specs) >= 2
    got = fs.log_posterior_batch(thetas)
    transform = fs.context.get_option('transform_ny'), fs.context.get_option('transform_nx')
    for f, (shape, kind, _) in enumerate(specs):
        tag = 'field %d (%s %dx%d)' % ((f, kind) + shape)
        alone = [None] * 3
        alone[f] = thetas[f]
        assert np.array_equal(fs.log_posterior_batch(alone)[f], got[f]), tag
        prior = fs.models[f].log_priors_batch(thetas[f])
        want = [xc.contract_evaluate(own[f], fields[f], t) for t in thetas[f]]
        worst_ll = max(check_ll(got[f][i], want[i][0] + prior[i], want[i][0], (tag, i)) for i in range(4))
        mine = own[f].log_posterior_batch(thetas[f])
        assert np.abs(got[f] - mine).max() <= 1e-12 * np.abs(mine).max(), tag
        a = fs.models[f].sample_images(thetas[f][:2], ('raw_model',))['raw_model']
        b = own[f].sample_images(thetas[f][:2], ('raw_model',))['raw_model']
        assert a.shape == (2,) + shape and np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), tag
        if (own[f].engine.get_option('transform_ny'), own[f].engine.get_option('transform_nx')) == transform:
            assert np.array_equal(got[f], mine) and np.array_equal(a, b), tag
        worst_raw = max(check_raw(a[i], want[i][1]['raw_model'], 1e-10 if kind == 'I' else RAW_BOUND, (tag, i))
                        for i in range(2))
        print('%s: worst raw-model relative error %.2e, worst log-likelihood relative error %.2e' % (tag, worst_raw, worst_ll))
    fs.close()
    for m in own:
        m.close()


# -- (e) a joint fit --------------------------------------------------------------------------------------------------
def test_joint_fit_with_two_psfs_per_exposure():
    """Two exposures, 64x64 and 70x96, two PSFs each, boxiness and modes {1, 3, 4} free on both; the positions and
    (as `JointModel` always has it, tests/test_joint_link.py) the PSF index per field: the four walkers take the four
    combinations of the two exposures' PSFs.  The joint log-posterior is the sum of the contract log-likelihoods +
    log_priors_batch (1e-9); one walker alone equals itself in the batch bit for bit; each field's posterior sums of
    the walkers against the contract's means at the bound of test_accumulated_images_against_the_contract (1e-11 of
    the largest value, the weight map as a variance), on the contract's finite pixels."""
    from psfmc_amd import JointModel
    shapes = [(64, 64), (70, 96)]
    cases = [xc.field_case(s, 900 + s[1], 2) for s in shapes]
    fields = [xc.oracle_field(c) for c in cases]
    for c, f in zip(cases, fields):
        xc.field_features(c, f)
    kw = xc.KINDS['F']
    joint = JointModel([xc.make_model(c, max_walkers=1, **kw) for c in cases],
                       per_field=['1_PointSource_xy', '2_Sersic_xy', '3_Sersic_xy'], max_walkers=16)
    own = [xc.make_model(c, max_walkers=1, **kw) for c in cases]
    names = joint.param_names
    assert names[-2:] == ['PSF_Index_f0', 'PSF_Index_f1'] and names.count('2_Sersic_f1_amp') == 1
    thetas = np.zeros((4, joint.num_params))
    for f in (1, 0):
        thetas[:, joint.field_columns(f)] = [xc.theta_of(own[f], *xc.scene(shapes[f], i)[:2], xc.scene(shapes[f], i)[2][:2],
                                                         psf=float((i // 2, i % 2)[f])) for i in range(4)]
    got = joint.log_posterior_batch(thetas)
    prior = joint.log_priors_batch(thetas)
    want = [[xc.contract_evaluate(own[f], fields[f], joint.field_theta(t, f)[0]) for t in thetas] for f in range(2)]
    worst = 0.0
    for i in range(4):
        total = (want[0][i][0] + want[1][i][0]) + prior[i]
        worst = max(worst, check_ll(got[i], total, total, i))
    assert len(np.unique(got)) == 4
    assert joint.log_posterior_batch(thetas[2:3])[0] == got[2]
    print('joint fit: worst log-posterior relative error %.2e' % worst)
    for f, m in enumerate(joint.field_models):
        m.reset_images()
        m.accumulate_samples(joint.field_theta(thetas, f))
        post = m.collect_posterior_images()
        imgs = [w[1] for w in want[f]]
        with np.errstate(all='ignore'):
            for kind in ('raw_model', 'convolved_model', 'residual', 'point_source_subtracted'):
                mean = np.mean([w[kind] for w in imgs], axis=0)
                fin = np.isfinite(mean)
                assert np.array_equal(np.isfinite(post[kind]), fin), (f, kind)
                assert np.max(np.abs(post[kind][fin] - mean[fin])) <= 1e-11 * np.max(np.abs(mean[fin])), (f, kind)
            var = np.mean([1 / w['composite_ivm'] for w in imgs], axis=0)
            fin = np.isfinite(var)
            assert np.array_equal(np.isfinite(1 / post['composite_ivm']), fin), f
            assert np.max(np.abs(1 / post['composite_ivm'][fin] - var[fin])) <= 1e-11 * np.max(np.abs(var[fin])), f
    joint.close()


# -- (f) row-based calls in several passes -----------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['G', 'F', 'M'])
def test_row_based_calls_in_several_passes(kind):
    """Five walkers on the two PSFs of a 70x96 field: log_likelihood_batch and sample_images in passes of two
    (chunk_walkers 2: the pass offsets of the auxiliary rows, the general and the Fourier parameters) are bit-identical
    to the same calls with the library's own pass size and within bounds of the contract; accumulate_samples under
    linear_accumulation 1 (the route through k_raster_sums_extra) and 0 against the contract's means
    (`check_posterior_sums`)."""
    shape = (70, 96)
    case, field = xc.several_psf_case(kind, shape)
    model = xc.make_model(case, max_walkers=8, **xc.KINDS[kind])
    n_s = len(xc.KINDS[kind]['sersics'])
    thetas = np.array([xc.theta_of(model, *xc.scene(shape, i)[:2], xc.scene(shape, i)[2][:n_s], psf=float(p))
                       for i, p in enumerate((0, 1, 1, 0, 1))])
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
    want = [xc.contract_evaluate(model, field, t) for t in thetas]
    worst_ll = max(check_ll(ll[i], want[i][0], want[i][0], (kind, i)) for i in range(5))
    worst_raw = max(check_raw(img['raw_model'][i], want[i][1]['raw_model'], raw_bound(kind), (kind, i)) for i in range(5))
    refs = [w[1] for w in want]
    tgr.check_images(img, refs, kind)
    for linear in (1, 0):
        eng.set_option('linear_accumulation', linear)
        assert eng.get_option('linear_accumulation') == linear
        tgr.check_posterior_sums(model, thetas, refs, (kind, 'linear_accumulation', linear))
    print('rows %s 70x96: worst raw-model relative error %.2e, worst log-likelihood relative error %.2e'
          % (kind, worst_raw, worst_ll))
    model.close()


# -- (g) the sampler ----------------------------------------------------------------------------------------------------
def test_device_sampler_with_a_free_psf_index():
    """A lean boxiness + modes model (12 free parameters) with two PSFs and a free PSF_Index, 24 walkers, 20
    iterations: the device-resident chain equals the host loop's fed the device's own log-posteriors, bit for bit; some
    steps are accepted; every log-posterior the host loop saw is finite, or -inf exactly where a prior is -inf --
    among them proposals whose index left the support."""
    from psfmc_amd.sampler import EnsembleSampler, DeviceEnsembleSampler
    shape, n_w = (64, 64), 24
    case = xc.field_case(shape, 77, 2)
    model = xc.make_model(case, [dict(boxiness=xc.FREE, fourier={1: (xc.FREE, xc.FREE), 3: (xc.FREE, 25.0)})],
                          max_walkers=n_w, lean=True)
    assert model.num_params == 12 and model.param_names[-1] == 'PSF_Index'
    sky, ps, sersics = xc.scene(shape)
    base = xc.theta_of(model, sky, ps, sersics[:1], psf=0.0)
    rng = np.random.RandomState(2)
    p0 = base + rng.normal(size=(n_w, len(base))) * 1e-2
    names = sum(([n] * w for n, w in zip(model.param_names, model.param_lens)), [])
    re, rb = names.index('2_Sersic_reff'), names.index('2_Sersic_reff_b')
    p0[:, rb] = np.minimum(p0[:, rb], p0[:, re] - 1e-3)
    p0[:, -1] = np.arange(n_w) % 2
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
    assert np.all(lp[left] == -np.inf)
    model.close()
