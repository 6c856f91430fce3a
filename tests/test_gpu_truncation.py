"""Inner and outer truncation of general components on the device, held to the numpy definition
(`Sersic.truncated_image`, `Sersic.general_mean_image(..., truncation)`) composed with the oracle's point source,
convolution and likelihood: raw images per pixel on both back ends, from raw vectors and from rows with auxiliary rows;
neutrality towards contexts and models without the keyword, removal, batch independence and the support, the pixel mean,
the samplers, sharded half-steps, posterior sums, field sets, joint fits, f32 storage, the library's refusals and a planted ring.  Field,
model and contract helpers are those of tests/test_gpu_radial_laws.py and tests/test_gpu_general_components.py."""
import numpy as np
import pytest

import test_gpu_fourier_modes as tgf
import test_gpu_general_components as tgg
import test_gpu_general_mean as tgm
import test_gpu_radial_laws as tgr
import test_gpu_spiral_arms as tgs
from extra_contract import EDGE_MARGIN, ferrer_state, law_error
from test_gpu_general_components import RAW_BOUND, contract_evaluate, make_field, oracle_field
from test_gpu_radial_laws import U, build, column, named, vector
from psfmc_amd.ModelComponents import Ferrer, Moffat, Sersic

pytestmark = pytest.mark.gpu

TR = lambda: U(-5.0, 90.0)               # a truncation radius: wider than the support
TWO = {2: ('free', 'free'), 3: ('free', 25.0)}
ARMS = dict(r_in='free', r_out='free', winding='free', inclination=35.0, sky_angle=20.0)
# how a component is dressed: bare, boxiness + modes, boxiness + spiral, everything
DRESS = [dict(), dict(boxiness='free', fourier=TWO), dict(boxiness='free', spiral=ARMS),
         dict(boxiness='free', fourier=TWO, spiral=ARMS)]
DRESS_VALUES = [dict(), dict(boxiness=0.7, f2_amp=0.2, f2_phase=30.0, f3_amp=-0.15),
                dict(boxiness=-0.4, spiral_r_in=2.0, spiral_r_out=10.0, spiral_wind=150.0),
                dict(boxiness=0.5, f2_amp=-0.2, f2_phase=100.0, f3_amp=0.1, spiral_r_in=0.0, spiral_r_out=7.0,
                     spiral_wind=-120.0)]


def cut(sides):
    return {k: (TR(), TR()) for k in sides}


def radii(sides, inner, outer):
    out = {}
    if 'inner' in sides:
        out.update(trunc_in_lo=inner[0], trunc_in_hi=inner[1])
    if 'outer' in sides:
        out.update(trunc_out_lo=outer[0], trunc_out_hi=outer[1])
    return out


IN, OUT, BOTH = ('inner',), ('outer',), ('inner', 'outer')
# (sides, dress) of the Sersic, the Moffat and the Ferrer of each model: every law with every choice of sides and with
# every dress, in four models
PLAN = [((IN, 0), (OUT, 1), (BOTH, 2)), ((OUT, 1), (BOTH, 2), (IN, 3)), ((BOTH, 2), (IN, 3), (OUT, 0)),
        ((BOTH, 3), (BOTH, 0), (BOTH, 1))]


def contract_sets(fld):
    """[(components, [{name: value}])]: four models of a Sersic, a Moffat and a Ferrer (`PLAN`), two walkers each.
    Walker 0: ramps a few pixels wide inside the components; the Sersic's and the Moffat's inner ramp (0.5, 3) and
    outer ramp (0.5, 4) have their steep part on the component's brightest pixels.  Walker 1: overlapping sides
    (in_hi = 12 > out_lo = 6), a lo of exactly 0, a centre on a pixel centre (Moffat) and one outside the image
    (Sersic), a ramp half a pixel wide (Ferrer)."""
    ny, nx = fld['shape']
    cx, cy = nx // 2, ny // 2
    small = 0.31 * min(ny, nx)
    sets = []
    for plan in PLAN:
        (s_sides, s_d), (m_sides, m_d), (f_sides, f_d) = plan
        comps = [(Sersic, dict(angle='free', truncation=cut(s_sides), **DRESS[s_d])),
                 (Moffat, dict(angle='free', truncation=cut(m_sides), **DRESS[m_d])),
                 (Ferrer, dict(angle='free', truncation=cut(f_sides), **DRESS[f_d]))]
        cases = []
        for i in range(2):
            ser = dict(angle=-20.0 + 50 * i, index=(1.0, 2.5)[i], mag=18.5, reff=(8.0, 14.0)[i], reff_b=(3.0, 9.0)[i],
                       xy=((cx + 3.2, cy - 1.1), (-3.6, cy + 0.4))[i], **DRESS_VALUES[s_d])
            ser.update(radii(s_sides, ((0.5, 3.0), (0.0, 12.0))[i], ((0.5, 4.0), (6.0, 40.0))[i]))
            mof = dict(angle=110.0 - 30 * i, beta=(2.5, 1.2)[i], fwhm=(6.0, 9.0)[i], fwhm_b=(4.0, 3.0)[i], mag=18.8,
                       xy=((cx + 0.25, cy + 0.4), (float(cx - 3), float(cy + 2)))[i], **DRESS_VALUES[m_d])
            mof.update(radii(m_sides, ((0.5, 3.0), (4.0, 12.0))[i], ((0.5, 4.0), (6.0, 16.0))[i]))
            fer = dict(alpha=(2.0, 0.5)[i], angle=30.0 + 40 * i, beta=(0.0, 1.5)[i], mag=18.0, r_out=(small, 1.3 * small)[i],
                       r_out_b=(0.45 * small, 0.9 * small)[i], xy=((cx - 1.4, cy + 0.7), (cx + 0.37, cy - 0.21))[i],
                       **DRESS_VALUES[f_d])
            fer.update(radii(f_sides, ((3.0, 7.0), (5.0, 5.5))[i], ((9.0, 15.0), (11.0, 11.5))[i]))
            cases.append(dict(named(2, 'Sersic', **ser), **dict(named(3, 'Moffat', **mof), **named(4, 'Ferrer', **fer))))
        sets.append((comps, cases))
    return sets


@pytest.mark.parametrize('backend,shape', [('fused', (64, 64)), ('fused', (70, 66)), ('hipfft', (64, 64)),
                                           ('hipfft', (70, 66))],
                         ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_device_against_the_contract(backend, shape):
    """Raw image per pixel by `law_error` -- relative to the pixel, to Sigma_0 of the Ferrer where that is larger -- at
    RAW_BOUND, the bound `test_gpu_radial_laws.test_device_against_the_contract` holds the untruncated forms to
    (MEASURED worst of the truncated forms: DESIGN.md section 26); the five images to 1e-12 of the image maximum; the
    log-posterior through raw vectors and the log-likelihood through the host path's rows and auxiliary rows against
    the contract (1e-9).  70 x 66: a second 64-lane chunk in every row, an embedded image."""
    fld = make_field(*shape, seed=1)
    field = oracle_field(fld)
    worst = 0.0
    for n_set, (comps, cases) in enumerate(contract_sets(fld)):
        model = build(fld, comps, backend=backend, degrees=True, slope=(n_set % 2 == 1))
        assert model.aux_rows(np.zeros((1, model.num_params))).shape[1] == 2 + 25 * 3
        thetas = np.array([vector(model, fld, v, adu=0.05 + 0.002 * i) for i, v in enumerate(cases)])
        want_all = []
        for i, t in enumerate(thetas):                                 # the host first: the condition on the inputs
            want_all.append(contract_evaluate(model, field, t))
            sigma0, margin = ferrer_state(model)
            assert margin >= EDGE_MARGIN, (shape, n_set, i, margin)
            want_all[-1] += (sigma0,)
        imgs = model.sample_images(thetas)
        lp = model.log_posterior_batch(thetas)
        ll_rows = model.log_likelihood_batch(thetas)
        prior = model.log_priors_batch(thetas)
        for i, (want_ll, want, sigma0) in enumerate(want_all):
            tag = '%s %dx%d set %d case %d' % ((backend,) + shape + (n_set, i))
            err = law_error(imgs['raw_model'][i], want['raw_model'], sigma0, tag)
            worst = max(worst, err)
            for kind in want:
                scale = np.max(np.abs(want[kind]))
                assert np.max(np.abs(imgs[kind][i] - want[kind])) <= 1e-12 * scale, (kind, tag)
            assert np.isfinite(want_ll) and np.isfinite(prior[i])
            assert abs(ll_rows[i] - want_ll) <= 1e-9 * abs(want_ll), (tag, ll_rows[i], want_ll)
            assert abs(lp[i] - (want_ll + prior[i])) <= 1e-9 * abs(want_ll), (tag, lp[i], want_ll + prior[i])
        model.close()
    print('%s %dx%d: worst raw-model error %.2e' % ((backend,) + shape + (worst,)))
    assert worst <= RAW_BOUND


# Sky + PS (a fixed position) + an exponential ring with 8 free parameters: adu, the point source's mag, the
# Sersic's mag, reff, x, y, trunc_in_hi, trunc_out_lo
RING = [(Sersic, dict(index=1.0, reff_b=7.0, truncation={'inner': (3.0, TR()), 'outer': (TR(), 26.0)}))]
RING_TRUTH = dict(mag=17.5, reff=12.0, xy=(32.3, 30.8), trunc_in_hi=9.0, trunc_out_lo=16.0)


def _ring_start(fld, model, n_w, seed, scale=1e-2):
    base = vector(model, fld, named(2, 'Sersic', **RING_TRUTH), ps_mag=19.0)
    return base + np.random.RandomState(seed).normal(size=(n_w, len(base))) * scale


def _law_reference():
    """Log-posteriors of a Moffat + Ferrer model (a context with laws, none with truncations)."""
    fld = make_field(64, 64, seed=7)
    model = build(fld, tgr.LEAN, max_walkers=16, ps_free=False)
    lp = model.log_posterior_batch(tgr._lean_start(fld, model, 16, 2))
    model.close()
    return (lp,)


def test_models_without_truncations_are_untouched_by_truncation_contexts():
    """Plain, boxiness-only, Fourier, spiral and radial-law models: bit-identical log-posteriors (and 20-iteration
    device chains) before and after contexts with truncations lived and died in the process."""
    refs = lambda: (tgg._plain_reference()[2], tgf._boxiness_reference(), tgs._fourier_reference(),
                    tgr._spiral_reference(), _law_reference())
    before = refs()
    fld = make_field(64, 64, seed=3)
    alive = []
    for comps, cases in contract_sets(fld)[:2]:
        alive.append(build(fld, comps))
        thetas = np.array([vector(alive[-1], fld, v) for v in cases])
        assert np.all(np.isfinite(alive[-1].log_posterior_batch(thetas)))
    alive.pop().close()
    after = refs()
    for m in alive:
        m.close()
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            assert np.array_equal(a, b)
        assert np.all(np.isfinite(y[0]))


def test_a_field_without_truncations_in_a_context_that_has_them_and_removal():
    """The field of a two-field context that has no truncation evaluates bit-identically to the same field beside a
    second field without truncations (a context that never saw the call).  All-zero flags: the slot renders what the
    same component without the keyword renders, bit for bit."""
    from psfmc_amd.models import FieldSet
    fa, fb = make_field(64, 64, seed=10), make_field(64, 64, seed=11)
    boxy = [(Sersic, dict(angle='free', boxiness='free'))]
    ring = [(Sersic, dict(angle='free', boxiness=0.2, truncation={'inner': (TR(), 9.0)}))]     # (as many free parameters)
    value = named(2, 'Sersic', angle=30.0, boxiness=0.3, index=1.5, mag=18.0, reff=8.0, reff_b=5.0, xy=(32.3, 30.8))
    got = []
    for second in (ring, boxy):
        fs = FieldSet([build(fa, boxy, max_walkers=1), build(fb, second, max_walkers=1)], max_walkers=8)
        theta = np.array([vector(fs.models[0], fa, value, adu=0.05 + 0.01 * i) for i in range(3)])
        got.append(fs.log_posterior_batch([theta, None])[0])
        got.append(fs.models[0].sample_images(theta[:2], ('raw_model',))['raw_model'])
        fs.close()
    assert np.all(np.isfinite(got[0])) and np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3])
    fld = make_field(64, 64, seed=17)
    trunc = build(fld, [(Moffat, dict(boxiness='free', truncation={'inner': (2.0, 6.0), 'outer': (8.0, 14.0)}))],
                  max_walkers=4)
    plain = build(fld, [(Moffat, dict(boxiness='free'))], max_walkers=4)
    assert trunc.param_names == plain.param_names
    t = vector(plain, fld, named(2, 'Moffat', beta=2.5, boxiness=0.3, fwhm=9.0, fwhm_b=6.5, mag=18.5, xy=(32.3, 30.8)))[None]
    want, first = plain.log_posterior_batch(t)[0], trunc.log_posterior_batch(t)[0]
    trunc.engine.set_truncation_layout([0], [-1] * 4, [0.0, 1.0, 0.0, 1.0])
    again = trunc.log_posterior_batch(t)[0]
    print('truncated %.6f, the slot without its flags %.6f, the plain Moffat %.6f' % (first, again, want))
    assert np.isfinite(first) and first != want and again == want
    trunc.close()
    plain.close()


def test_batch_independence_and_the_support():
    """A walker's log-posterior bits are the same alone, in a batch of 16 and in permuted order; lo = hi, lo < 0, NaN
    and inf are -inf from raw vectors on the device and on the host, leave the other walkers' bits unchanged, and are
    NaN through a row-based call (no writable flags there); lo = 0 is inside."""
    fld = make_field(64, 64, seed=4)
    comps = [(Sersic, dict(angle='free', truncation=cut(BOTH))), (Ferrer, dict(angle='free', truncation=cut(OUT)))]
    model = build(fld, comps, max_walkers=16)
    base = vector(model, fld, dict(
        named(2, 'Sersic', angle=30.0, index=1.5, mag=18.0, reff=9.0, reff_b=6.0, xy=(32.3, 30.8), trunc_in_lo=2.0,
              trunc_in_hi=6.0, trunc_out_lo=12.0, trunc_out_hi=20.0),
        **named(3, 'Ferrer', alpha=1.5, angle=70.0, beta=0.5, mag=18.3, r_out=18.3, r_out_b=7.1, xy=(30.31, 33.73),
                trunc_out_lo=8.0, trunc_out_hi=13.0)))
    thetas = base + np.random.RandomState(5).normal(size=(16, len(base))) * 1e-3
    thetas[15, column(model, '2_Sersic_trunc_in_lo')] = 0.0                        # lo = 0: inside
    full = model.log_posterior_batch(thetas)
    assert np.all(np.isfinite(full))
    for i in (0, 7, 15):
        assert model.log_posterior_batch(thetas[i:i + 1])[0] == full[i]
    perm = np.random.RandomState(6).permutation(16)
    assert np.array_equal(model.log_posterior_batch(thetas[perm]), full[perm])
    # ('lo': the side's own lo, hi = lo)
    bad = [('2_Sersic_trunc_in_hi', 'lo'), ('2_Sersic_trunc_in_lo', -0.1), ('2_Sersic_trunc_out_lo', np.nan),
           ('2_Sersic_trunc_out_hi', np.inf), ('3_Ferrer_trunc_out_hi', 'lo'), ('3_Ferrer_trunc_out_lo', np.nan),
           ('2_Sersic_trunc_in_hi', np.nan)]
    where = [1 + 2 * k for k in range(len(bad))]
    mixed = thetas.copy()
    for k, (name, val) in zip(where, bad):
        mixed[k, column(model, name)] = mixed[k, column(model, name.replace('_hi', '_lo'))] if val == 'lo' else val
    got = model.log_posterior_batch(mixed)
    keep = np.ones(16, dtype=bool)
    keep[where] = False
    for k, what in zip(where, bad):
        assert got[k] == -np.inf, what
    assert np.array_equal(got[keep], full[keep])
    assert np.all(model.log_posterior_batch_host(mixed)[where] == -np.inf)
    rows = model.engine.loglike(model.derived_rows(mixed[where]), aux=model.aux_rows(mixed[where]))
    for what, r in zip(bad, rows):
        assert np.isnan(r), what
    assert np.isfinite(model.engine.loglike(model.derived_rows(thetas[:1]), aux=model.aux_rows(thetas[:1]))[0])
    model.close()


@pytest.mark.parametrize('backend', ['fused', 'hipfft'])
def test_pixel_mean_of_truncated_components(backend):
    """pixel_mean=True with a truncation against `general_mean_image(..., truncation)` at the mode's bound
    (RAW_BOUND by `law_error`, tests/test_gpu_general_mean.py): a ring of the Sersic law on a pixel centre (finite),
    an inner-truncated Moffat with modes, an outer-truncated wound Ferrer; 70 x 66."""
    fld = make_field(70, 66, seed=6)
    field = oracle_field(fld)
    comps = [(Sersic, dict(angle='free', pixel_mean=True, truncation=cut(BOTH))),
             (Moffat, dict(angle='free', pixel_mean=True, truncation=cut(IN), **DRESS[1])),
             (Ferrer, dict(angle='free', pixel_mean=True, truncation=cut(OUT), **DRESS[2]))]
    model = build(fld, comps, backend=backend, max_walkers=4)
    assert model.sersic_general_mean == [True] * 3 and model.sersic_truncation_flags == [3, 1, 2]
    values = dict(named(2, 'Sersic', angle=30.0, index=1.5, mag=18.0, reff=9.0, reff_b=6.0, xy=(33.0, 35.0),
                        trunc_in_lo=1.0, trunc_in_hi=5.0, trunc_out_lo=6.0, trunc_out_hi=14.0),
                  **dict(named(3, 'Moffat', angle=110.0, beta=2.5, fwhm=6.0, fwhm_b=4.0, mag=18.8, xy=(28.25, 40.4),
                               trunc_in_lo=0.5, trunc_in_hi=3.0, **DRESS_VALUES[1]),
                         **named(4, 'Ferrer', alpha=2.0, angle=30.0, beta=0.0, mag=18.0, r_out=19.84, r_out_b=8.9,
                                 xy=(31.6, 33.7), trunc_out_lo=9.0, trunc_out_hi=15.0, **DRESS_VALUES[2])))
    thetas = np.array([vector(model, fld, values)])
    want_ll, want = contract_evaluate(model, field, thetas[0])
    sigma0, margin = tgm.mean_ferrer_state(model)
    assert margin >= EDGE_MARGIN, margin
    imgs = model.sample_images(thetas, ('raw_model',))['raw_model']
    lp, prior = model.log_posterior_batch(thetas), model.log_priors_batch(thetas)
    assert law_error(imgs[0], want['raw_model'], sigma0, '%s pixel mean' % backend) <= RAW_BOUND
    assert np.isfinite(want_ll) and abs(lp[0] - (want_ll + prior[0])) <= 1e-9 * abs(want_ll)
    model.close()


@pytest.mark.parametrize('n_w', [22, 64])
def test_device_sampler_equals_the_host_sampler(n_w):
    """The device-resident chain equals the host loop's fed the device's own log-posteriors, bit for bit (22 walkers:
    the whole-iteration route of small ensembles; 64: half-steps)."""
    from psfmc_amd.sampler import EnsembleSampler, DeviceEnsembleSampler
    fld = make_field(64, 64, seed=7)
    model = build(fld, RING, max_walkers=n_w, ps_free=False)
    assert model.num_params == 8
    p0 = _ring_start(fld, model, n_w, 2)
    host = EnsembleSampler(n_w, model.num_params, batch_lnpostfn=model.log_posterior_batch)
    dev = DeviceEnsembleSampler(n_w, model, block=7)
    for s in (host, dev):
        s.random_state = np.random.RandomState(8).get_state()
    list(host.sample(p0, iterations=20))
    list(dev.sample(p0, iterations=20))
    assert np.array_equal(dev.chain, host.chain) and np.array_equal(dev.naccepted, host.naccepted)
    assert np.array_equal(dev.lnprobability, host.lnprobability)
    assert dev.naccepted.sum() > 0 and np.all(np.isfinite(dev.lnprobability))
    model.close()


def test_tempered_sampler_equals_the_host_contract():
    """Three rungs, eight iterations: chain, log-probabilities, log-likelihoods, acceptances and swaps equal the host
    contract's."""
    from psfmc_amd.sampler import TemperedEnsembleSampler, DeviceTemperedSampler, default_betas
    fld = make_field(64, 64, seed=8)
    model = build(fld, RING, max_walkers=3 * 18, ps_free=False)
    betas = default_betas(3, 50.0)
    p0 = _ring_start(fld, model, 3 * 18, 3).reshape(3, 18, -1)
    host = TemperedEnsembleSampler(18, model.num_params, betas, model.log_likelihood_and_prior_batch)
    dev = DeviceTemperedSampler(18, model, betas=betas, block=4)
    for s in (host, dev):
        s.random_state = np.random.RandomState(11).get_state()
    list(host.sample(p0, iterations=8))
    list(dev.sample(p0, iterations=8))
    assert np.array_equal(dev.chain, host.chain)
    assert np.array_equal(dev.lnprobability, host.lnprobability)
    assert np.array_equal(dev.lnlikelihood, host.lnlikelihood)
    assert np.array_equal(dev.naccepted_t, host.naccepted_t) and np.array_equal(dev.nswap, host.nswap)
    assert np.all(np.isfinite(dev.lnlikelihood)) and dev.naccepted_t.sum() > 0
    model.close()


def test_sharded_half_steps_equal_one_context_and_the_contract():
    """The half-step API of multi-GPU fits (tests/shard_driver.py: three ranks inside one process, 20 walkers in blocks
    of 4, 3, 3 on an embedded 70 x 66 field): `psfmc_stretch_half_eval` runs the pipeline with a walker offset, so a
    wrong offset of the truncations' per-walker constants would evaluate a walker with another walker's radii.  Every
    rank's chain is bit-identical to one `DeviceEnsembleSampler`'s on one more context, and every gathered
    log-posterior of a proposal equals the contract's to 1e-9 |ll|."""
    import shard_driver as sd
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(70, 66, seed=18)
    field = oracle_field(fld)
    ranks, n_w, seed = 3, 20, 7
    models = [build(fld, RING, max_walkers=n_w, ps_free=False) for _ in range(ranks + 1)]
    single, models = models[-1], models[:-1]
    p0 = _ring_start(fld, single, n_w, seed, scale=0.05)
    draws = sd.draw(sd.random_state(seed), sd.N_ITER, n_w, single.num_params)
    lnp0 = models[0].log_posterior_batch(p0)
    samp = DeviceEnsembleSampler(n_w, single)
    samp.random_state = sd.random_state(seed)
    list(samp.sample(p0, iterations=sd.N_ITER))
    res = sd.run_blocks(models, p0, lnp0, draws)
    for r in range(ranks):
        assert np.array_equal(res['chain'][r], samp.chain), r
        assert np.array_equal(res['lnchain'][r], samp.lnprobability), r
        assert np.array_equal(res['nacc'][r], samp.naccepted.astype(np.int64)), r
    q, acc = sd.replay(p0, res['chain'][0], draws[0], draws[2])
    assert acc.sum() > 0 and np.all(np.isfinite(res['gathered']))
    for it in (0, sd.N_ITER - 1):
        for h in range(2):
            for j in (0, 4, 9):                                        # one walker of every rank's block
                want = contract_evaluate(single, field, q[it, h, j])[0] + single.log_priors_batch(q[it, h, j][None])[0]
                assert abs(res['gathered'][it, h, j] - want) <= 1e-9 * abs(want), (it, h, j)
    for m in models + [single]:
        m.close()


def test_accumulated_images_against_the_contract():
    fld = make_field(70, 66, seed=9)
    comps, cases = contract_sets(fld)[1]
    model = build(fld, comps)
    thetas = np.array([vector(model, fld, v) for v in cases])
    field = oracle_field(fld)
    model.accumulate_samples(thetas)
    got = model.collect_posterior_images()
    want = [contract_evaluate(model, field, t)[1] for t in thetas]
    for kind in ('raw_model', 'convolved_model', 'residual', 'point_source_subtracted'):
        mean = np.mean([w[kind] for w in want], axis=0)
        assert np.max(np.abs(got[kind] - mean)) <= 1e-11 * np.max(np.abs(mean)), kind
    var = np.mean([1 / w['composite_ivm'] for w in want], axis=0)
    assert np.max(np.abs(1 / got['composite_ivm'] - var)) <= 1e-11 * np.max(np.abs(var))
    model.close()


RING_FULL = [(Sersic, dict(angle='free', boxiness='free', truncation=cut(BOTH)))]


def _ring_full(fld, model, n_w, seed, scale=0.05, idx=2):
    ny, nx = fld['shape']
    base = vector(model, fld, named(idx, 'Sersic', angle=30.0, boxiness=0.3, index=1.2, mag=17.8, reff=10.0, reff_b=6.5,
                                    xy=(nx / 2 + 0.31, ny / 2 - 0.27), trunc_in_lo=2.0, trunc_in_hi=8.0,
                                    trunc_out_lo=14.0, trunc_out_hi=24.0))
    return base + np.random.RandomState(seed).normal(size=(n_w, len(base))) * scale


@pytest.mark.parametrize('order', [(0, 1), (1, 0)], ids=['truncated-first', 'truncated-last'])
def test_field_set_keeps_the_truncations_per_field(order):
    """A 64x64 field with a boxy ring and a 70x66 field with a boxy Sersic with two modes (as many free parameters),
    registered in either order, against each field's own context: within 1e-12 of the largest value, bit-identical
    where the own context has the set's transform."""
    from psfmc_amd.models import FieldSet
    flds = [make_field(64, 64, seed=10), make_field(70, 66, seed=11)]
    specs = [RING_FULL, [(Sersic, dict(angle='free', boxiness='free', fourier={2: ('free', 'free'), 3: ('free', 'free')}))]]
    flds, specs = [flds[i] for i in order], [specs[i] for i in order]
    fs = FieldSet([build(f, s, max_walkers=1) for f, s in zip(flds, specs)], max_walkers=16)
    own = [build(f, s, max_walkers=8) for f, s in zip(flds, specs)]
    thetas = []
    for f, m in zip(flds, own):
        if any(m.sersic_truncation_flags):
            thetas.append(_ring_full(f, m, 4, 12))
        else:
            ny, nx = f['shape']
            thetas.append(np.array([vector(m, f, named(
                2, 'Sersic', angle=30.0 + 10 * i, boxiness=-0.4 + 0.3 * i, index=1.0 + i, mag=18.0, reff=6.0, reff_b=4.0,
                xy=(nx / 2 + 0.31 + i, ny / 2 - 0.27), f2_amp=0.1 * i, f2_phase=20.0, f3_amp=-0.1, f3_phase=50.0))
                for i in range(4)]))
    got = fs.log_posterior_batch(thetas)
    transform = fs.context.get_option('transform_ny'), fs.context.get_option('transform_nx')
    for f in range(2):
        alone = [None, None]
        alone[f] = thetas[f]
        assert np.array_equal(fs.log_posterior_batch(alone)[f], got[f]), f
        mine = own[f].log_posterior_batch(thetas[f])
        assert np.all(np.isfinite(got[f])) and np.abs(got[f] - mine).max() <= 1e-12 * np.abs(mine).max(), f
        a = fs.models[f].sample_images(thetas[f][:2], ('raw_model',))['raw_model']
        b = own[f].sample_images(thetas[f][:2], ('raw_model',))['raw_model']
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), f
        if (own[f].engine.get_option('transform_ny'), own[f].engine.get_option('transform_nx')) == transform:
            assert np.array_equal(got[f], mine) and np.array_equal(a, b), f
    fs.close()
    for m in own:
        m.close()


def test_joint_model_shared_inner_radius_and_own_outer_radius():
    from psfmc_amd import JointModel
    fa, fb = make_field(64, 64, seed=12), make_field(70, 66, seed=13)
    make = lambda f: build(f, RING_FULL, max_walkers=1, extent=70)
    joint = JointModel([make(fa), make(fb)], per_field=['2_Sersic_trunc_out_hi', '1_PointSource_xy', '2_Sersic_xy'],
                       max_walkers=16)
    names = joint.param_names
    assert names.count('2_Sersic_trunc_in_hi') == 1 and '2_Sersic_trunc_out_hi_f1' in names
    own_a, own_b = make(fa), make(fb)
    base_a, base_b = _ring_full(fa, own_a, 3, 14, scale=0.02), _ring_full(fb, own_b, 3, 14, scale=0.02)
    base_b[:, column(own_b, '2_Sersic_trunc_out_hi')] += 3.0
    thetas = np.zeros((3, joint.num_params))
    thetas[:, joint.field_columns(1)] = base_b
    thetas[:, joint.field_columns(0)] = base_a
    got = joint.log_posterior_batch(thetas)
    prior = joint.log_priors_batch(thetas)
    field_a, field_b = oracle_field(fa), oracle_field(fb)
    for i, t in enumerate(thetas):
        ta, tb = joint.field_theta(t, 0)[0], joint.field_theta(t, 1)[0]
        assert ta[column(own_a, '2_Sersic_trunc_in_hi')] == tb[column(own_b, '2_Sersic_trunc_in_hi')]
        assert abs(tb[column(own_b, '2_Sersic_trunc_out_hi')] - ta[column(own_a, '2_Sersic_trunc_out_hi')] - 3.0) < 0.5
        want = (contract_evaluate(own_a, field_a, ta)[0] + contract_evaluate(own_b, field_b, tb)[0]) + prior[i]
        assert np.isfinite(want) and abs(got[i] - want) <= 1e-9 * abs(want), (i, got[i], want)
    assert joint.log_posterior_batch(thetas[1:2])[0] == got[1]
    bad = thetas[:1].copy()
    bad[0, joint.field_columns(0)[column(own_a, '2_Sersic_trunc_in_hi')]] = 1.0     # the shared in_hi <= in_lo
    assert joint.log_posterior_batch(bad)[0] == -np.inf
    joint.close()
    own_a.close()
    own_b.close()


def test_f32_storage_and_context_group():
    """storage='f32' within its documented 2e-6; a ContextGroup on one device equals the plain context through raw
    vectors."""
    fld = make_field(64, 64, seed=14)
    field = oracle_field(fld)
    f32 = build(fld, RING_FULL, storage='f32')
    thetas = _ring_full(fld, f32, 3, 15, scale=0.02)
    ll = f32.log_likelihood_batch(thetas)
    lp32 = f32.log_posterior_batch(thetas)
    prior = f32.log_priors_batch(thetas)
    for i, t in enumerate(thetas):
        want_ll, _ = contract_evaluate(f32, field, t)
        assert abs(ll[i] - want_ll) <= 2e-6 * abs(want_ll) and abs(lp32[i] - want_ll - prior[i]) <= 2e-6 * abs(want_ll)
    f32.close()
    model = build(fld, RING_FULL)
    grp = model.device_group([0], max_walkers=16)
    got = grp.logpost_theta(thetas)
    assert np.all(np.isfinite(got)) and np.array_equal(got, model.log_posterior_batch(thetas))
    grp.close()
    model.close()


def test_the_library_refuses_what_the_header_says():
    from psfmc_amd.engine import NativeError
    fld = make_field(64, 64, seed=15)
    model = build(fld, [(Moffat, {}), (Sersic, dict(boxiness=0.3)), (Sersic, {})], max_walkers=4)
    eng = model.engine
    t = vector(model, fld, dict(named(2, 'Moffat', beta=2.5, fwhm=5.0, fwhm_b=3.5, mag=18.5, xy=(32.3, 30.8)), **dict(
        named(3, 'Sersic', index=1.5, mag=18.5, reff=6.0, reff_b=3.5, xy=(30.3, 33.8)),
        **named(4, 'Sersic', index=2.0, mag=19.0, reff=4.0, reff_b=3.0, xy=(35.3, 28.8)))))[None]
    before = model.log_posterior_batch(t)[0]
    neutral = [0.0, 1.0] * 6
    with pytest.raises(NativeError, match='truncation flags 4 outside 0 ... 3'):
        eng.set_truncation_layout([4, 0, 0], [-1] * 12, neutral)
    with pytest.raises(NativeError, match='truncation flags -1 outside'):
        eng.set_truncation_layout([-1, 0, 0], [-1] * 12, neutral)
    with pytest.raises(NativeError, match='has a truncation but is not flagged general'):
        eng.set_truncation_layout([1, 0, 2], [-1] * 12, neutral)               # the third slot is a plain Sersic
    with pytest.raises(NativeError, match='n_sersic=2, the context has 3'):
        eng.set_truncation_layout([1, 0], [-1] * 8, neutral[:8])
    with pytest.raises(NativeError, match='column'):
        eng.set_truncation_layout([1, 0, 0], [model.num_params] + [-1] * 11, neutral)
    assert model.log_posterior_batch(t)[0] == before                          # nothing changed
    eng.set_truncation_layout([3, 2, 0], [-1] * 12, [2.0, 5.0, 8.0, 12.0, 0.0, 1.0, 6.0, 9.0, 0.0, 1.0, 0.0, 1.0])
    cut_lp = model.log_posterior_batch(t)[0]
    assert np.isfinite(cut_lp) and cut_lp != before
    eng.set_general_mean([False, False, False])                                # keeps the flags
    assert model.log_posterior_batch(t)[0] == cut_lp
    eng.set_truncation_layout([0, 0, 0], [-1] * 12, neutral)                   # all-zero flags remove them
    assert model.log_posterior_batch(t)[0] == before
    model.close()
    plain = build(fld, [(Sersic, {})], max_walkers=4)
    with pytest.raises(NativeError, match='has no aux layout'):
        plain.engine.set_truncation_layout([1], [-1] * 4, neutral[:4])
    plain.close()
    integ = build(fld, [(Sersic, dict(integrate=True))], max_walkers=4, slope=True)          # (a tilted sky: an aux layout)
    with pytest.raises(NativeError, match='pixel-integrated: truncation and integrate exclude each other'):
        integ.engine.set_truncation_layout([2], [-1] * 4, neutral[:4])
    integ.close()


def test_a_planted_ring_is_recovered():
    """sci = the contract's convolved image of an exponential ring (inner (3, 9), outer (16, 26) on reff 12 / 7) plus
    the helper's fixed-seed noise: the log-posterior at the planted vector exceeds the one with trunc_in_hi off by 3
    pixels, and the truth of trunc_in_hi lies inside the central 95 % of the last 100 iterations of a 200-iteration,
    32-walker device chain started in a ball about trunc_in_hi = 8."""
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(64, 64, seed=16)
    noise = fld['sci'].astype(np.float64) - 0.05
    first = build(fld, RING, max_walkers=1, ps_free=False)
    planted = vector(first, fld, named(2, 'Sersic', **RING_TRUTH))
    conv = contract_evaluate(first, oracle_field(fld), planted)[1]['convolved_model']
    first.close()
    model = build(dict(fld, sci=(conv + noise).astype(np.float32)), RING, max_walkers=32, ps_free=False)
    col = column(model, '2_Sersic_trunc_in_hi')
    off = planted.copy()
    off[col] = 12.0
    lp = model.log_posterior_batch(np.array([planted, off]))
    print('log-posterior at the planted vector %.2f, with trunc_in_hi = 12: %.2f' % (lp[0], lp[1]))
    assert np.isfinite(lp[1]) and lp[0] > lp[1]
    rng = np.random.RandomState(4)
    start = planted.copy()
    start[col] = 8.0
    scale = np.full(len(start), 1e-2)
    scale[0], scale[col] = 1e-3, 0.3
    p0 = start + rng.normal(size=(32, len(start))) * scale
    s = DeviceEnsembleSampler(32, model, block=50)
    s.random_state = np.random.RandomState(5).get_state()
    list(s.sample(p0, iterations=200))
    lo, med, hi = np.percentile(s.chain[:, -100:, col], [2.5, 50.0, 97.5])
    print('trunc_in_hi of the last 100 iterations: 2.5 %% %.3f, median %.3f, 97.5 %% %.3f' % (lo, med, hi))
    assert lo <= 9.0 <= hi
    model.close()
