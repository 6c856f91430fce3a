"""Boxy / disky Sersic isophotes and the tilted sky on the device, held to their numpy definitions
(`Sersic.general_image`, `Sky.tilted_image`) composed with the oracle's point source, convolution and likelihood: raw
images per pixel on every forward-kernel family of both back ends, c = 0 against the plain rasteriser, the untouched
default, batch independence, mixed models, the samplers, posterior sums, field sets, joint fits, f32 storage and
context groups."""
import numpy as np
import pytest

import psfmc_oracle as orc
import synth_field
from psfmc_amd import MultiComponentModel
from psfmc_amd.ModelComponents import Configuration, PointSource, Sersic, Sky
from psfmc_amd.distributions import Normal, Uniform

pytestmark = pytest.mark.gpu

# The per-pixel bound of the raw model against the contract: the default rasteriser's bound in this project.
# MEASURED maximum over every shape, back end and case below: 3.75e-15 (table in DESIGN.md section 15).
RAW_BOUND = 1e-11
MAG_ZP = 25.0
ABSENT = object()


def make_field(ny, nx, seed=0, psf_side=16):
    """A synthetic exposure of any shape: noise about a faint level, a Moffat PSF with its own noise map."""
    rng = np.random.RandomState(seed)
    psf = synth_field.moffat_psf(side=psf_side) * 1000.0
    psf_var = 0.01 ** 2 + np.abs(psf) / 50.0
    f32 = np.float32
    return dict(sci=(0.05 + rng.normal(size=(ny, nx)) * 0.02).astype(f32), ivm=np.full((ny, nx), 1 / 0.02 ** 2, f32),
                psf=(psf + rng.normal(size=psf.shape) * np.sqrt(psf_var)).astype(f32), psf_ivm=(1 / psf_var).astype(f32),
                mag_zp=MAG_ZP, shape=(ny, nx))


FREE = object()


LEAN = [0, 1, 2, 3, 7, 8, 9, 10, 11, 12, 13]          # the free columns of a `lean` model among the full model's


def make_model(fld, boxiness=(FREE,), slope=FREE, integrate=(), backend='fused', max_walkers=64, storage='f64',
               lean=False):
    """Sky + PointSource + one Sersic per entry of `boxiness` (a prior, a number, or ABSENT); `slope` likewise.
    Free-parameter order: adu, [slope x 2], ps mag, x, y, then per Sersic angle, [boxiness], index, mag, reff,
    reff_b, x, y.  FREE: the test's prior, a fresh object per model.  lean: the point source's position and the
    Sersics' angle are constants (11 free parameters with one Sersic: an ensemble of 22 walkers is allowed)."""
    ny, nx = fld['shape']
    c = np.array((nx / 2 + 0.5, ny / 2 + 0.5))
    if slope is FREE:
        slope = Normal(loc=(0, 0), scale=(1e-3, 1e-3))
    boxiness = [Uniform(loc=-1.5, scale=4.0) if b is FREE else b for b in boxiness]
    wide = lambda: Uniform(loc=c - 2.0 * max(ny, nx), scale=4.0 * max(ny, nx) * np.ones(2))
    comps = [Configuration(fld['sci'], fld['ivm'], fld['psf'], fld['psf_ivm'], mag_zeropoint=fld['mag_zp']),
             Sky(adu=Normal(loc=0.05, scale=0.05), **({} if slope is ABSENT else {'slope': slope})),
             PointSource(xy=(nx / 2 + 1.3, ny / 2 - 0.8) if lean else wide(), mag=Uniform(loc=16.0, scale=8.0))]
    for k, box in enumerate(boxiness):
        kw = {} if box is ABSENT else {'boxiness': box}
        if k < len(integrate) and integrate[k]:
            kw['integrate'] = True
        comps.append(Sersic(xy=wide(), mag=Uniform(loc=15.0, scale=10.0), reff=Uniform(loc=0.5, scale=40.0),
                            reff_b=Uniform(loc=0.5, scale=40.0), index=Uniform(loc=0.2, scale=8.0),
                            angle=30.0 if lean else Uniform(loc=-360, scale=720), angle_degrees=True, **kw))
    return MultiComponentModel(comps, backend=backend, max_walkers=max_walkers, storage=storage)


def theta_of(fld, sersics, adu=0.05, slope=(4e-4, -3e-4), ps=(19.0, None, None)):
    """One parameter vector; sersics: dicts with angle, [boxiness], index, mag, reff, reff_b, x, y."""
    ny, nx = fld['shape']
    t = [adu] + ([] if slope is None else list(slope))
    t += [ps[0], nx / 2 + 1.3 if ps[1] is None else ps[1], ny / 2 - 0.8 if ps[2] is None else ps[2]]
    for s in sersics:
        t += [s['angle']] + ([s['boxiness']] if 'boxiness' in s else []) + [s['index'], s['mag'], s['reff'], s['reff_b'],
                                                                         s['x'], s['y']]
    return np.array(t, dtype=np.float64)


def contract_cases(fld):
    """c in {-1, 0, 0.7, 2} and more, n in {0.5, 1, 4}, a centre at x + 0.5 on a pixel row with the axes along the
    pixel grid (u or v exactly 0 along a pixel line), a centre on a pixel corner, centres outside the image."""
    ny, nx = fld['shape']
    cx, cy = nx // 2, ny // 2
    rows = [
        dict(boxiness=-1.0, index=0.5, reff=6.0, reff_b=4.0, angle=30.0, x=cx + 0.31, y=cy - 0.27),
        dict(boxiness=0.0, index=1.0, reff=5.0, reff_b=4.5, angle=75.0, x=cx - 2.4, y=cy + 1.7),
        dict(boxiness=0.7, index=4.0, reff=3.0, reff_b=1.5, angle=110.0, x=cx + 0.25, y=cy + 0.4),
        dict(boxiness=2.0, index=1.0, reff=8.0, reff_b=3.0, angle=-20.0, x=cx + 3.2, y=cy - 1.1),
        dict(boxiness=0.7, index=1.0, reff=4.0, reff_b=3.0, angle=-90.0, x=cx + 0.5, y=float(cy)),     # v = 0 on row cy
        dict(boxiness=-1.0, index=4.0, reff=5.0, reff_b=2.0, angle=0.0, x=float(cx), y=cy + 0.5),      # u = 0 on col cx
        dict(boxiness=2.0, index=0.5, reff=7.0, reff_b=6.0, angle=45.0, x=cx + 0.5, y=cy - 0.5),       # a pixel corner
        dict(boxiness=-0.5, index=1.0, reff=12.0, reff_b=9.0, angle=10.0, x=-3.6, y=cy + 0.4),         # outside
        dict(boxiness=1.3, index=4.0, reff=20.0, reff_b=8.0, angle=60.0, x=nx + 5.0, y=ny + 2.5),
    ]
    out = []
    for i, r in enumerate(rows):
        r['mag'] = 18.0 + 0.3 * i
        # (slopes that keep the plane positive over the image: no pixel near a zero crossing)
        out.append(theta_of(fld, [r], adu=0.05 + 0.002 * i,
                            slope=(0.02 / nx * (1 - i % 3), 0.02 / ny * (-0.75 + 0.25 * i))))
    return np.array(out)


def oracle_field(fld):
    return orc.make_field(fld['sci'], fld['ivm'], [fld['psf']], [fld['psf_ivm']], mag_zp=fld['mag_zp'])


def contract_raw(model, theta):
    """Raw model of one vector: the components' own host definitions (`add_to_array`) and the oracle's point source."""
    model.param_values = np.asarray(theta, dtype=np.float64)
    shape = model.config.obs_data.shape
    raw = np.zeros(shape)
    coords = orc.array_coords(shape)
    for comp in model.components:
        if isinstance(comp, PointSource):
            orc.add_point_source(raw, np.ravel(comp.xy), float(np.ravel(comp.mag)[0]), model.config.mag_zeropoint, coords,
                                 comp.shift_method)
        elif isinstance(comp, (Sky, Sersic)):
            comp.add_to_array(raw, model.config.mag_zeropoint)
    return raw


def contract_evaluate(model, field, theta):
    """(log-likelihood, images) from the contract's raw model through the oracle's convolution and likelihood."""
    raw = contract_raw(model, theta)
    with np.errstate(all='ignore'):
        conv = orc.convolve(raw, field.psf_spec[0])
        resid = field.sci - conv
        ivm = 1 / (orc.convolve(raw ** 2, field.var_spec[0]) + field.obs_var)
        ps = np.zeros(raw.shape)
        for comp in model.components:
            if isinstance(comp, PointSource):
                orc.add_point_source(ps, np.ravel(comp.xy), float(np.ravel(comp.mag)[0]), model.config.mag_zeropoint,
                                     orc.array_coords(raw.shape), comp.shift_method)
        images = {'raw_model': raw, 'convolved_model': conv, 'residual': resid, 'composite_ivm': ivm,
                  'point_source_subtracted': field.sci - orc.convolve(ps, field.psf_spec[0])}
        good = ~field.bad_px
        ll = -0.5 * np.sum(resid[good] ** 2 * ivm[good] - np.log(0.5 / np.pi * ivm[good]))
    return (ll if np.isfinite(ll) else -np.inf), images


def raw_error(got, want, tag):
    """Relative on every pixel above 1e-12 of the peak."""
    assert np.all(np.isfinite(got)), tag
    big = np.abs(want) > 1e-12 * np.abs(want).max()
    err = np.max(np.abs(got[big] - want[big]) / np.abs(want[big]))
    print('%s: raw model max relative error %.2e' % (tag, err))
    return err


SHAPES = [(64, 64), (96, 64), (64, 320), (70, 66), (64, 1152)]


@pytest.mark.parametrize('backend,shape', [('fused', s) for s in SHAPES] + [('hipfft', (64, 64)), ('hipfft', (70, 66))],
                         ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_device_against_the_contract(backend, shape):
    """64x64 and 96x64: the log2 + exp2 forward form; 64x320: the power-table form; 70x66: embedded (wrap window,
    ly x lx clipping); 64x1152: the k_rows3_fwd EXTRA instantiation.  Raw image per pixel (RAW_BOUND), the five images
    to 1e-12 of the image maximum, the log-posterior through raw vectors and the log-likelihood through the host
    path's rows against the contract (1e-9)."""
    fld = make_field(*shape, seed=1)
    model = make_model(fld, backend=backend, max_walkers=16)
    field = oracle_field(fld)
    thetas = contract_cases(fld)
    imgs = model.sample_images(thetas)
    lp = model.log_posterior_batch(thetas)
    ll_rows = model.log_likelihood_batch(thetas)
    prior = model.log_priors_batch(thetas)
    worst = 0.0
    for i, t in enumerate(thetas):
        want_ll, want = contract_evaluate(model, field, t)
        worst = max(worst, raw_error(imgs['raw_model'][i], want['raw_model'], '%s %dx%d case %d' % ((backend,) + shape + (i,))))
        for kind in want:
            scale = np.max(np.abs(want[kind]))
            assert np.max(np.abs(imgs[kind][i] - want[kind])) <= 1e-12 * scale, (kind, i)
        assert np.isfinite(want_ll) and np.isfinite(prior[i])
        assert abs(ll_rows[i] - want_ll) <= 1e-9 * abs(want_ll), (i, ll_rows[i], want_ll)
        assert abs(lp[i] - (want_ll + prior[i])) <= 1e-9 * abs(want_ll), (i, lp[i], want_ll + prior[i])
    print('%s %dx%d: worst raw-model relative error %.2e' % ((backend,) + shape + (worst,)))
    assert worst <= RAW_BOUND
    model.close()


def test_zero_boxiness_and_slope_against_the_plain_rasteriser():
    """The same model with and without boxiness=0.0, slope=(0, 0): log-posteriors agree to RAW_BOUND carried through
    the likelihood -- a relative change d of every model pixel moves a pixel's term r^2 w - ln(w / 2 pi) (r the
    residual, w the weight, m the convolved model) by at most d (2 |r| |m| w + 2 r^2 w + 2), so the bound is RAW_BOUND
    times the sum of those magnitudes (relative to the sum of the terms' magnitudes, as tests/fuzz_shapes.py does)."""
    fld = make_field(64, 64, seed=2)
    general = make_model(fld, boxiness=(0.0,), slope=(0.0, 0.0), max_walkers=16)
    plain = make_model(fld, boxiness=(ABSENT,), slope=ABSENT, max_walkers=16)
    assert general.param_names == plain.param_names
    thetas = np.array([t[[0, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13]] for t in contract_cases(fld)])
    a, b = general.log_posterior_batch(thetas), plain.log_posterior_batch(thetas)
    imgs = plain.sample_images(thetas, ('convolved_model', 'composite_ivm'))
    sci = fld['sci'].astype(np.float64)
    for i in range(len(thetas)):
        m, w = imgs['convolved_model'][i], imgs['composite_ivm'][i]
        r = sci - m
        bound = RAW_BOUND * 0.5 * float(np.sum(2 * np.abs(r) * np.abs(m) * w + 2 * r * r * w + 2))
        print('case %d: |difference| %.3e, bound %.3e' % (i, abs(a[i] - b[i]), bound))
        assert np.isfinite(b[i]) and abs(a[i] - b[i]) <= bound, (i, a[i], b[i])
    general.close()
    plain.close()


def _plain_reference():
    """(log-posteriors, 20-iteration device chain, its log-probabilities) of a model WITHOUT the keywords."""
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(64, 64, seed=3)
    base = np.array([t[[0, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13]] for t in contract_cases(fld)[:4]])
    rng = np.random.RandomState(1)
    thetas = base[rng.randint(0, 4, 24)] + rng.normal(size=(24, 11)) * 1e-2
    thetas[:, 8] = np.minimum(thetas[:, 8], thetas[:, 7] - 1e-3)
    plain = make_model(fld, boxiness=(ABSENT,), slope=ABSENT, max_walkers=24)
    lp = plain.log_posterior_batch(thetas)
    s = DeviceEnsembleSampler(24, plain, block=5)
    s.random_state = np.random.RandomState(3).get_state()
    list(s.sample(thetas, iterations=20))
    out = lp, s.chain.copy(), s.lnprobability.copy()
    plain.close()
    return fld, thetas, out


def test_default_is_untouched_by_aux_contexts_in_the_process(tmp_path):
    """A model without the keywords: bit-identical log-posteriors and 20-iteration device chain in a FRESH process,
    in which no aux-bearing context was ever created (a child process: that is what this test is about), and in
    this one after aux-bearing contexts lived and died in it."""
    import os
    import subprocess
    import sys
    ref = os.path.join(str(tmp_path), 'plain.npz')
    code = ('import numpy as np, test_gpu_general_components as t; _, _, out = t._plain_reference(); '
            'np.savez(%r, lp=out[0], chain=out[1], lnp=out[2])' % ref)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    subprocess.run([sys.executable, '-c', code], env=env, check=True, timeout=120)
    before = np.load(ref)
    fld, thetas, _ = _plain_reference()
    general = make_model(fld, max_walkers=16)
    general.log_posterior_batch(contract_cases(fld))
    other = make_model(fld, boxiness=(0.5,), slope=ABSENT, max_walkers=24)
    other.log_posterior_batch(thetas)
    general.close()
    after = _plain_reference()[2]
    other.close()
    for key, y in zip(('lp', 'chain', 'lnp'), after):
        assert np.array_equal(before[key], y), key
    assert np.all(np.isfinite(after[0]))


def test_batch_independence_and_the_support_of_the_boxiness():
    """A walker's log-posterior bits are the same alone, in a batch of 37 and across a pass boundary; a walker with
    boxiness <= -2 is -inf and leaves the others unchanged."""
    fld = make_field(64, 64, seed=4)
    model = make_model(fld, boxiness=(Uniform(loc=-3.0, scale=6.0),), max_walkers=64)
    base = contract_cases(fld)
    rng = np.random.RandomState(5)
    thetas = base[rng.randint(0, len(base), 37)] + rng.normal(size=(37, base.shape[1])) * 1e-3
    thetas[:, 11] = np.minimum(thetas[:, 11], thetas[:, 10] - 1e-3)
    full = model.log_posterior_batch(thetas)
    assert np.all(np.isfinite(full))
    for i in (0, 17, 36):
        assert model.log_posterior_batch(thetas[i:i + 1])[0] == full[i]
    bad = thetas.copy()
    bad[5, 7], bad[20, 7] = -2.0, -2.5
    mixed = model.log_posterior_batch(bad)
    keep = np.ones(37, dtype=bool)
    keep[[5, 20]] = False
    assert mixed[5] == -np.inf and mixed[20] == -np.inf and np.array_equal(mixed[keep], full[keep])
    assert np.array_equal(model.log_posterior_batch_host(bad) == -np.inf, ~keep)
    model.engine.set_option('chunk_walkers', 5)
    assert model.engine.pass_size(37) <= 5
    assert np.array_equal(model.log_posterior_batch(thetas), full)
    model.close()


@pytest.mark.parametrize('backend', ['fused', 'hipfft'])
def test_mixed_models(backend):
    """Two Sersics with one general (either order); one general beside one pixel-integrated (the integrated kernels
    write the extra image, the general one adds)."""
    fld = make_field(64, 64, seed=6)
    field = oracle_field(fld)
    cx = 32
    s0 = dict(index=1.0, mag=18.0, reff=6.0, reff_b=4.0, angle=30.0, x=cx + 0.3, y=cx - 1.2)
    s1 = dict(index=3.0, mag=18.5, reff=4.0, reff_b=2.0, angle=100.0, x=cx - 2.5, y=cx + 0.5)
    for boxes, integ in (((FREE, ABSENT), ()), ((ABSENT, FREE), ()),
                         ((FREE, ABSENT), (False, True))):
        model = make_model(fld, boxiness=boxes, integrate=integ, backend=backend, max_walkers=8)
        a, b = dict(s0), dict(s1)
        (a if boxes[0] is not ABSENT else b)['boxiness'] = 0.8
        thetas = np.array([theta_of(fld, [a, b]), theta_of(fld, [dict(a, x=cx + 0.5), dict(b, y=cx + 0.5)],
                                                        slope=(-2e-4, 1e-4))])
        imgs = model.sample_images(thetas, ('raw_model',))['raw_model']
        lp = model.log_posterior_batch(thetas)
        prior = model.log_priors_batch(thetas)
        for i, t in enumerate(thetas):
            want_ll, want = contract_evaluate(model, field, t)
            # (the pixel-integrated profile's own bound where it is in the model)
            assert raw_error(imgs[i], want['raw_model'], '%s mixed %d' % (backend, i)) <= (1e-10 if integ else RAW_BOUND)
            assert abs(lp[i] - (want_ll + prior[i])) <= 1e-9 * abs(want_ll)
        model.close()


@pytest.mark.parametrize('n_w', [22, 64])
def test_device_sampler_equals_the_host_sampler(n_w):
    """The device-resident chain equals the host loop's fed the device's own log-posteriors, bit for bit (22 walkers:
    the whole-iteration route of small ensembles; 64: half-steps)."""
    from psfmc_amd.sampler import EnsembleSampler, DeviceEnsembleSampler
    fld = make_field(64, 64, seed=7)
    model = make_model(fld, max_walkers=n_w, lean=True)
    base = contract_cases(fld)[:4][:, LEAN]
    rng = np.random.RandomState(2)
    p0 = base[rng.randint(0, 4, n_w)] + rng.normal(size=(n_w, base.shape[1])) * 1e-2
    p0[:, 1:3] *= 1e-1
    p0[:, 8] = np.minimum(p0[:, 8], p0[:, 7] - 1e-3)
    host = EnsembleSampler(n_w, model.num_params, batch_lnpostfn=model.log_posterior_batch)
    dev = DeviceEnsembleSampler(n_w, model, block=7)
    for s in (host, dev):
        s.random_state = np.random.RandomState(8).get_state()
    list(host.sample(p0, iterations=30))
    list(dev.sample(p0, iterations=30))
    assert np.array_equal(dev.chain, host.chain) and np.array_equal(dev.naccepted, host.naccepted)
    assert np.array_equal(dev.lnprobability, host.lnprobability)
    assert dev.naccepted.sum() > 0 and np.all(np.isfinite(dev.lnprobability))
    model.close()


def test_tempered_sampler():
    """Three rungs run and the cold rung's values are the model's own; one rung is the stretch sampler's chain."""
    from psfmc_amd.sampler import DeviceEnsembleSampler, DeviceTemperedSampler
    fld = make_field(64, 64, seed=8)
    model = make_model(fld, max_walkers=3 * 24, lean=True)
    base = contract_cases(fld)[:4][:, LEAN]
    rng = np.random.RandomState(3)
    p0 = base[rng.randint(0, 4, 3 * 24)] + rng.normal(size=(3 * 24, base.shape[1])) * 1e-2
    p0[:, 1:3] *= 1e-1
    p0[:, 8] = np.minimum(p0[:, 8], p0[:, 7] - 1e-3)
    p0 = p0.reshape(3, 24, -1)
    pt = DeviceTemperedSampler(24, model, ntemps=3, tmax=20.0, block=4)
    pt.random_state = np.random.RandomState(2).get_state()
    list(pt.sample(p0, iterations=8))
    assert np.all(np.isfinite(pt.lnlikelihood)) and pt.naccepted.sum() > 0
    last = pt.chain[:, -1, :]
    assert np.array_equal(model.log_likelihood_and_prior_batch(last)[0], pt.lnlikelihood[0, :, -1])
    ref = DeviceEnsembleSampler(24, model, block=6)
    one = DeviceTemperedSampler(24, model, betas=[1.0], block=5)
    for s in (ref, one):
        s.random_state = np.random.RandomState(8).get_state()
    list(ref.sample(p0[0], iterations=10))
    list(one.sample(p0[:1], iterations=10))
    assert np.array_equal(one.chain, ref.chain) and np.array_equal(one.lnprobability, ref.lnprobability)
    model.close()


@pytest.mark.parametrize('backend,shape', [('fused', (64, 64)), ('fused', (70, 66)), ('hipfft', (64, 64))],
                         ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_accumulated_images_against_the_contract(backend, shape):
    fld = make_field(*shape, seed=9)
    model = make_model(fld, backend=backend, max_walkers=16)
    field = oracle_field(fld)
    thetas = contract_cases(fld)
    model.accumulate_samples(thetas)
    got = model.collect_posterior_images()
    want = [contract_evaluate(model, field, t)[1] for t in thetas]
    for kind in ('raw_model', 'convolved_model', 'residual', 'point_source_subtracted'):
        mean = np.mean([w[kind] for w in want], axis=0)
        assert np.max(np.abs(got[kind] - mean)) <= 1e-11 * np.max(np.abs(mean)), kind
    var = np.mean([1 / w['composite_ivm'] for w in want], axis=0)
    assert np.max(np.abs(1 / got['composite_ivm'] - var)) <= 1e-11 * np.max(np.abs(var))
    model.close()


def test_field_set_keeps_per_field_keywords():
    """One field with the keywords (fixed values: the same free parameters) and one without: each bit-identical to
    its own context."""
    from psfmc_amd.models import FieldSet
    fa, fb = make_field(64, 64, seed=10), make_field(64, 64, seed=11)
    kw_a = dict(boxiness=(0.6,), slope=(3e-4, -2e-4))
    kw_b = dict(boxiness=(ABSENT,), slope=ABSENT)
    a, b = make_model(fa, max_walkers=1, **kw_a), make_model(fb, max_walkers=1, **kw_b)
    own_a, own_b = make_model(fa, max_walkers=16, **kw_a), make_model(fb, max_walkers=16, **kw_b)
    fs = FieldSet([a, b], max_walkers=32)
    thetas = np.array([t[[0, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13]] for t in contract_cases(fa)])
    got = fs.log_posterior_batch([thetas, thetas[::-1]])
    assert np.array_equal(got[0], own_a.log_posterior_batch(thetas))
    assert np.array_equal(got[1], own_b.log_posterior_batch(thetas[::-1]))
    assert np.all(np.isfinite(got[0])) and not np.array_equal(got[0], got[1][::-1])
    # the field's images go through its view of the shared context, aux rows included
    assert np.array_equal(fs.models[0].sample_images(thetas[:2], ('raw_model',))['raw_model'],
                          own_a.sample_images(thetas[:2], ('raw_model',))['raw_model'])
    fs.close()
    own_a.close()
    own_b.close()


def test_joint_model_shared_boxiness_and_own_slopes():
    from psfmc_amd import JointModel
    fa, fb = make_field(64, 64, seed=12), make_field(70, 66, seed=13)
    a, b = make_model(fa, max_walkers=1), make_model(fb, max_walkers=1)
    joint = JointModel([a, b], per_field=['0_Sky_slope', '1_PointSource_xy', '2_Sersic_xy'], max_walkers=32)
    names = joint.param_names
    assert names.count('2_Sersic_boxiness') == 1 and '0_Sky_slope_f1' in names
    base = contract_cases(fa)[:4]
    own_b = contract_cases(fb)[:4]
    thetas = np.zeros((4, joint.num_params))
    thetas[:, joint.field_columns(1)] = own_b
    thetas[:, joint.field_columns(0)] = base
    shared = np.intersect1d(joint.field_columns(0), joint.field_columns(1))
    got = joint.log_posterior_batch(thetas)
    prior = joint.log_priors_batch(thetas)
    field_a, field_b = oracle_field(fa), oracle_field(fb)
    own_a_model, own_b_model = make_model(fa, max_walkers=1), make_model(fb, max_walkers=1)
    for i, t in enumerate(thetas):
        ll_a = contract_evaluate(own_a_model, field_a, joint.field_theta(t, 0)[0])[0]
        ll_b = contract_evaluate(own_b_model, field_b, joint.field_theta(t, 1)[0])[0]
        want = (ll_a + ll_b) + prior[i]
        assert np.isfinite(want) and abs(got[i] - want) <= 1e-9 * abs(want), (i, got[i], want)
    assert len(shared) and joint.log_posterior_batch(thetas[1:2])[0] == got[1]
    bad = thetas[:1].copy()
    bad[0, joint.field_columns(0)[7]] = -2.0                      # (field 0's own column 7: the boxiness)
    assert joint.log_posterior_batch(bad)[0] == -np.inf
    joint.close()


def test_f32_storage_and_context_group():
    """storage='f32' within its documented 2e-6; a ContextGroup on one device equals the plain context."""
    fld = make_field(64, 64, seed=14)
    field = oracle_field(fld)
    thetas = contract_cases(fld)[:5]
    f32 = make_model(fld, max_walkers=16, storage='f32')
    ll = f32.log_likelihood_batch(thetas)
    lp32 = f32.log_posterior_batch(thetas)
    prior = f32.log_priors_batch(thetas)
    for i, t in enumerate(thetas):
        want_ll, _ = contract_evaluate(f32, field, t)
        assert abs(ll[i] - want_ll) <= 2e-6 * abs(want_ll) and abs(lp32[i] - want_ll - prior[i]) <= 2e-6 * abs(want_ll)
    f32.close()
    model = make_model(fld, max_walkers=16)
    grp = model.device_group([0], max_walkers=16)
    assert np.array_equal(grp.logpost_theta(thetas), model.log_posterior_batch(thetas))
    with pytest.raises(NotImplementedError, match='boxiness'):
        grp.loglike(model.derived_rows(thetas), aux=model.aux_rows(thetas))
    grp.close()
    model.close()


def test_row_calls_without_aux_rows_are_refused():
    """The library never evaluates derived rows of such a context without their auxiliary vectors."""
    from psfmc_amd.engine import NativeError
    fld = make_field(64, 64, seed=15)
    model = make_model(fld, max_walkers=8)
    thetas = contract_cases(fld)[:3]
    rows = model.derived_rows(thetas)
    with pytest.raises(NativeError, match='psfmc_set_aux_rows'):
        model.engine.loglike(rows)
    assert np.all(np.isfinite(model.engine.loglike(rows, aux=model.aux_rows(thetas))))
    with pytest.raises(NativeError, match='psfmc_set_aux_rows'):      # (the rows served one call)
        model.engine.images(rows, ('raw_model',))
    model.close()
