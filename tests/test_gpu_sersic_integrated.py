"""The pixel-integrated Sersic profile on the device, held to its numpy definition (`Sersic.integrated_image`)
composed with the oracle's convolution and likelihood: raw images per pixel, the five images and the
log-posterior on every row-kernel family of both back ends, batch independence, the samplers, posterior sums, joint
fits with the flag on one exposure, and the untouched default."""
import numpy as np
import pytest

import helpers
import psfmc_oracle as orc
import synth_field
from psfmc_amd import MultiComponentModel
from psfmc_amd.ModelComponents import Configuration, PointSource, Sersic
from psfmc_amd.distributions import Uniform, WeibullMinimum

pytestmark = pytest.mark.gpu

ABSENT = object()


def make_model(n_side, flags, backend='auto', max_walkers=32, seed=0, storage='f64'):
    """test_gpu_fullsize.make_model's field and priors; flags: per Sersic True / False / ABSENT (keyword not given)."""
    fld = synth_field.make_field(n_side, len(flags), seed=seed)
    c = np.array((n_side / 2 + 0.5,) * 2)
    comps = [Configuration(fld['sci'], fld['ivm'], fld['psf'], fld['psf_ivm'], mag_zeropoint=fld['mag_zp']),
             PointSource(xy=Uniform(loc=c - 8, scale=16 * np.ones(2)), mag=Uniform(loc=18.0, scale=2.0))]
    for flag in flags:
        kw = {} if flag is ABSENT else {'integrate': flag}
        comps.append(Sersic(xy=Uniform(loc=c - 8, scale=16 * np.ones(2)), mag=Uniform(loc=19.0, scale=5.0),
                            reff=Uniform(loc=2.0, scale=n_side / 16.0), reff_b=Uniform(loc=2.0, scale=n_side / 16.0),
                            index=WeibullMinimum(c=1.5, scale=4), angle=Uniform(loc=0, scale=180),
                            angle_degrees=True, **kw))
    return MultiComponentModel(comps, backend=backend, max_walkers=max_walkers, storage=storage), fld


def oracle_field(fld):
    return orc.make_field(fld['sci'], fld['ivm'], [fld['psf']], [fld['psf_ivm']], mag_zp=fld['mag_zp'])


def contract_raw(field, theta, flags):
    """Raw model of one vector: the oracle's rasteriser for the sky, the point sources and the plain Sersics, the
    numpy definition for the integrated ones."""
    comps, _ = helpers.comps_from_theta(helpers.synth_layout(len(flags)), theta)
    sersics = [c for c in comps if c['type'] == 'sersic']
    plain = [c for c in comps if c['type'] != 'sersic'] + [c for c, f in zip(sersics, flags) if f is not True]
    raw = orc.raw_model(field, plain, np.float64)
    for c, f in zip(sersics, flags):
        if f is True:
            comp = Sersic(xy=c['xy'], mag=c['mag'], reff=c['reff'], reff_b=c['reff_b'], index=c['index'],
                          angle=c['angle'], angle_degrees=c['angle_degrees'], integrate=True)
            comp.add_to_array(raw, field.mag_zp)
    return raw


def contract_evaluate(field, theta, flags):
    """(log-likelihood, images) from the contract's raw model through the oracle's own convolution and likelihood
    (oracle.evaluate's lines, which take no raw image)."""
    comps, _ = helpers.comps_from_theta(helpers.synth_layout(len(flags)), theta)
    raw = contract_raw(field, theta, flags)
    with np.errstate(all='ignore'):
        conv = orc.convolve(raw, field.psf_spec[0])
        resid = field.sci - conv
        ivm = 1 / (orc.convolve(raw ** 2, field.var_spec[0]) + field.obs_var)
        ps = orc.raw_model(field, comps, np.float64, only='ps')
        images = {'raw_model': raw, 'convolved_model': conv, 'residual': resid, 'composite_ivm': ivm,
                  'point_source_subtracted': field.sci - orc.convolve(ps, field.psf_spec[0])}
        good = ~field.bad_px
        ll = -0.5 * np.sum(resid[good] ** 2 * ivm[good] - np.log(0.5 / np.pi * ivm[good]))
    return (ll if np.isfinite(ll) else -np.inf), images


def vary(truth, k, **kw):
    """truth with Sersic k's angle / index / mag / reff / reff_b / x / y replaced."""
    names = ('angle', 'index', 'mag', 'reff', 'reff_b', 'x', 'y')
    t = truth.copy()
    for key, val in kw.items():
        t[3 + 7 * k + names.index(key)] = val
    return t


def profile_cases(truth, side, k=0):
    c = side // 2
    cases = [vary(truth, k, index=n, reff=re, reff_b=re * ar, x=x, y=y) for n, re, ar, x, y in [
        (0.3, 6.0, 0.8, c + 0.31, c - 0.27),            # inside a pixel
        (1.0, 1.5, 0.9, c + 0.5, c + 0.13),             # on an edge
        (4.0, 2.0, 0.6, c + 0.5, c - 0.5),              # on a corner
        (2.5, 12.0, 0.5, float(c), float(c + 1)),       # on a pixel centre
        (8.0, 40.0, 0.7, c - 3.4, c + 2.2),
        (6.5, 4.0, 0.5, 0.3, 1.8),                      # near the border: the box is clipped
        (1.5, 9.0, 0.9, -2.6, c + 0.4),                 # beyond it
        (3.1, 20.0, 0.4, side + 5.0, side - 0.5),
        (0.5, 3.0, 1.0, c + 0.25, float(c)),
    ]]
    return np.array(cases)


def assert_raw_matches(got, want, tag):
    """Per pixel: relative on every pixel above 1e-12 of the peak (the default rasteriser's bound is 1e-11, the
    integrated pixels add up to a few thousand samples in another order than numpy: no looser than 1e-10)."""
    assert np.all(np.isfinite(got)), tag
    big = np.abs(want) > 1e-12 * np.abs(want).max()
    err = np.max(np.abs(got[big] - want[big]) / np.abs(want[big]))
    print('%s: raw model max relative error %.2e' % (tag, err))
    assert err <= 1e-10, (tag, err)
    assert np.max(np.abs(got[~big] - want[~big])) <= 1e-20 * np.abs(want).max() if (~big).any() else True, tag


@pytest.mark.parametrize('backend', ['fused', 'hipfft'])
@pytest.mark.parametrize('side', [128, 150, 146, 1152])
def test_device_against_the_contract(side, backend):
    """Power-of-two, general built, embedded and above-1024 sides (every row-kernel family), both back ends: raw image
    per pixel over the profile cases, then the five images (1e-12 of the image maximum) and the log-likelihood
    (1e-9) as tests/test_gpu_parity.py holds the default to the oracle."""
    flags = [True]
    model, fld = make_model(side, flags, backend, max_walkers=16)
    field = oracle_field(fld)
    thetas = profile_cases(fld['truth'], side)
    if side > 1024:
        thetas = thetas[[1, 2, 3, 5]]
    imgs = model.sample_images(thetas)
    ll = model.log_likelihood_batch(thetas)
    for i, t in enumerate(thetas):
        want_ll, want = contract_evaluate(field, t, flags)
        assert_raw_matches(imgs['raw_model'][i], want['raw_model'], '%s %d case %d' % (backend, side, i))
        for kind in want:
            scale = np.max(np.abs(want[kind]))
            assert np.max(np.abs(imgs[kind][i] - want[kind])) <= 1e-12 * scale, (kind, i)
        assert np.isfinite(want_ll) and abs(ll[i] - want_ll) <= 1e-9 * abs(want_ll), (i, ll[i], want_ll)
    model.close()


@pytest.mark.parametrize('backend', ['fused', 'hipfft'])
def test_mixed_and_two_integrated_components(backend):
    """Two integrated components; an integrated one beside a plain one (either order) and the point source."""
    side = 128
    for flags in ([True, True], [False, True], [True, ABSENT]):
        model, fld = make_model(side, flags, backend, max_walkers=16)
        field = oracle_field(fld)
        base = synth_field.draw_walkers(side, 2, 3, seed=3, near_truth=fld['truth'])
        thetas = np.vstack([base, vary(vary(fld['truth'], 0, x=64.0, y=63.5), 1, x=64.5, y=64.0, index=5.0, reff=3.0,
                                       reff_b=2.0)])
        imgs = model.sample_images(thetas, ('raw_model',))['raw_model']
        lp = model.log_posterior_batch(thetas)
        prior = model.log_priors_batch(thetas)
        for i, t in enumerate(thetas):
            want_ll, want = contract_evaluate(field, t, flags)
            assert_raw_matches(imgs[i], want['raw_model'], '%s flags %s case %d' % (backend, flags, i))
            assert abs(lp[i] - (want_ll + prior[i])) <= 1e-9 * abs(want_ll), (flags, i)
        model.close()


def test_f32_storage_and_small_ensemble_route():
    """storage='f32' serves the keyword (the same rasteriser, complex64 intermediates: 1e-6 as for the default), and
    so does the whole-iteration route of small ensembles (covered by the sampler test below)."""
    model, fld = make_model(128, [True], 'fused', max_walkers=16, storage='f32')
    field = oracle_field(fld)
    thetas = profile_cases(fld['truth'], 128)[:4]
    ll = model.log_likelihood_batch(thetas)
    for i, t in enumerate(thetas):
        want_ll, _ = contract_evaluate(field, t, [True])
        assert abs(ll[i] - want_ll) <= 1e-6 * abs(want_ll)
    model.close()


@pytest.mark.parametrize('side', [128, 288])
def test_batch_independence_and_on_pixel_centre(side):
    """A walker's integrated log-posterior is bit-identical alone, in a full batch and beside skipped walkers
    (prior -inf); an on-pixel centre is finite with the keyword and -inf without."""
    n_w = 64
    model, fld = make_model(side, [True], 'fused', max_walkers=n_w)
    thetas = synth_field.draw_walkers(side, 1, n_w, seed=5, near_truth=fld['truth'])
    thetas[7, 8:10] = (side // 2, side // 2 + 1)                   # an on-pixel centre
    full = model.log_posterior_batch(thetas)
    assert np.all(np.isfinite(full))
    for i in (0, 7, n_w - 1):
        assert model.log_posterior_batch(thetas[i:i + 1])[0] == full[i]
    assert np.array_equal(model.log_posterior_batch(thetas[:5]), full[:5])
    out = thetas.copy()
    out[::2, 0] = 99.0                                             # outside the magnitude prior: skipped
    mixed = model.log_posterior_batch(out)
    assert np.all(mixed[::2] == -np.inf) and np.array_equal(mixed[1::2], full[1::2])
    plain, _ = make_model(side, [ABSENT], 'fused', max_walkers=n_w)
    assert plain.log_posterior_batch(thetas[7:8])[0] == -np.inf and np.isfinite(full[7])
    plain.close()
    model.close()


def test_default_is_untouched():
    """The keyword absent and spelled integrate=False: bit-equal log-posteriors and images."""
    absent, fld = make_model(128, [ABSENT, ABSENT], 'fused', max_walkers=16)
    spelled, _ = make_model(128, [False, False], 'fused', max_walkers=16)
    thetas = synth_field.draw_walkers(128, 2, 16, seed=6, near_truth=fld['truth'])
    assert np.array_equal(absent.log_posterior_batch(thetas), spelled.log_posterior_batch(thetas))
    a, b = absent.sample_images(thetas[:4]), spelled.sample_images(thetas[:4])
    for kind in a:
        assert np.array_equal(a[kind], b[kind]), kind
    assert absent.engine.get_option('pow_tabs') == spelled.engine.get_option('pow_tabs')
    absent.close()
    spelled.close()


@pytest.mark.parametrize('n_w', [24, 600])
def test_device_sampler_equals_the_host_sampler(n_w):
    """The device-resident chain of an integrated model equals the host loop's fed the device's log-posteriors (24
    walkers: the whole-iteration route of small ensembles; 600: half-steps)."""
    from psfmc_amd.sampler import EnsembleSampler, DeviceEnsembleSampler
    model, fld = make_model(128, [True], 'fused', max_walkers=n_w)
    p0 = synth_field.draw_walkers(128, 1, n_w, seed=4, near_truth=fld['truth'])
    host = EnsembleSampler(n_w, model.num_params, batch_lnpostfn=model.log_posterior_batch)
    dev = DeviceEnsembleSampler(n_w, model, block=4)
    for s in (host, dev):
        s.random_state = np.random.RandomState(8).get_state()
    list(host.sample(p0, iterations=8))
    list(dev.sample(p0, iterations=8))
    assert np.array_equal(dev.chain, host.chain) and np.array_equal(dev.naccepted, host.naccepted)
    assert np.array_equal(dev.lnprobability, host.lnprobability)
    assert dev.naccepted.sum() > 0
    model.close()


@pytest.mark.parametrize('backend,side', [('fused', 128), ('fused', 146), ('hipfft', 128)])
def test_accumulated_images_against_the_contract(backend, side):
    flags = [True]
    model, fld = make_model(side, flags, backend, max_walkers=16)
    field = oracle_field(fld)
    thetas = synth_field.draw_walkers(side, 1, 12, seed=7, near_truth=fld['truth'])
    thetas[3, 8:10] = (side // 2 + 0.5, side // 2)
    model.accumulate_samples(thetas)
    got = model.collect_posterior_images()
    want = [contract_evaluate(field, t, flags)[1] for t in thetas]
    for kind in ('raw_model', 'convolved_model', 'residual', 'point_source_subtracted'):
        mean = np.mean([w[kind] for w in want], axis=0)
        assert np.max(np.abs(got[kind] - mean)) <= 1e-11 * np.max(np.abs(mean)), kind
    var = np.mean([1 / w['composite_ivm'] for w in want], axis=0)
    assert np.max(np.abs(1 / got['composite_ivm'] - var)) <= 1e-11 * np.max(np.abs(var))
    model.close()


def test_joint_model_with_the_flag_on_one_exposure():
    from psfmc_amd import JointModel
    a, fld_a = make_model(128, [True], 'fused', max_walkers=1, seed=0)
    b, fld_b = make_model(128, [False], 'fused', max_walkers=1, seed=1)
    joint = JointModel([a, b], max_walkers=32)                   # (every parameter shared)
    rng = np.random.RandomState(3)
    thetas = fld_a['truth'] + rng.normal(size=(6, joint.num_params)) * 1e-2
    thetas[:, 7] = np.minimum(thetas[:, 7], thetas[:, 6] - 1e-3)
    thetas[2, 8:10] = (64.0, 65.0)                               # an on-pixel centre in both exposures
    got = joint.log_posterior_batch(thetas)
    prior = joint.log_priors_batch(thetas)
    fa, fb = oracle_field(fld_a), oracle_field(fld_b)
    for i, t in enumerate(thetas):
        ll_a = contract_evaluate(fa, t, [True])[0]
        ll_b = contract_evaluate(fb, t, [False])[0]
        if i == 2:                                               # the plain exposure is NaN there
            assert np.isfinite(ll_a) and ll_b == -np.inf and got[i] == -np.inf
            continue
        want = (ll_a + ll_b) + prior[i]
        assert np.isfinite(want) and abs(got[i] - want) <= 1e-9 * abs(want), (i, got[i], want)
    assert joint.log_posterior_batch(thetas[1:2])[0] == got[1]
    # the same scene with the flag on BOTH exposures is finite at the on-pixel centre
    both = JointModel([a, make_model(128, [True], 'fused', max_walkers=1, seed=1)[0]], max_walkers=32)
    assert np.isfinite(both.log_posterior_batch(thetas[2:3])[0])
    both.close()
    joint.close()


def test_field_set_keeps_per_field_flags():
    from psfmc_amd.models import FieldSet
    a, fld_a = make_model(128, [True], 'fused', max_walkers=1, seed=0)
    b, fld_b = make_model(128, [False], 'fused', max_walkers=1, seed=1)
    fs = FieldSet([a, b], max_walkers=16)
    ta = synth_field.draw_walkers(128, 1, 4, seed=2, near_truth=fld_a['truth'])
    tb = synth_field.draw_walkers(128, 1, 4, seed=3, near_truth=fld_b['truth'])
    got = fs.log_posterior_batch([ta, tb])
    for th, fld, flags, g, m in ((ta, fld_a, [True], got[0], fs.models[0]), (tb, fld_b, [False], got[1], fs.models[1])):
        field = oracle_field(fld)
        prior = m.log_priors_batch(th)
        for i, t in enumerate(th):
            want = contract_evaluate(field, t, flags)[0] + prior[i]
            assert abs(g[i] - want) <= 1e-9 * abs(want), (flags, i)
    fs.close()


def test_tempered_sampler_runs():
    from psfmc_amd.sampler import DeviceTemperedSampler
    model, fld = make_model(128, [True], 'fused', max_walkers=3 * 24)
    p0 = np.stack([synth_field.draw_walkers(128, 1, 24, seed=10 + t, near_truth=fld['truth']) for t in range(3)])
    pt = DeviceTemperedSampler(24, model, ntemps=3, tmax=20.0, block=3)
    pt.random_state = np.random.RandomState(2).get_state()
    list(pt.sample(p0, iterations=6))
    assert np.all(np.isfinite(pt.lnlikelihood)) and pt.naccepted.sum() > 0
    # the cold rung's values are the model's own
    last = pt.chain[:, -1, :]
    assert np.array_equal(model.log_likelihood_and_prior_batch(last)[0], pt.lnlikelihood[0, :, -1])
    model.close()
