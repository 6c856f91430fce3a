"""Spiral arms on Sersic components by coordinate rotation on the device, held to the numpy definition
(`Sersic.spiral_image`) composed with the oracle's point source, convolution and likelihood: raw images per pixel on
every forward-kernel family of both back ends, zero winding against the model without the keyword, batch independence
and the support, the untouched default, boxiness-only and Fourier models, the samplers, mixed models, posterior sums,
field sets, joint fits, f32 storage, context groups, the library's refusals and a planted two-armed host.  Field and
contract helpers are those of tests/test_gpu_general_components.py."""
import numpy as np
import pytest

import test_gpu_fourier_modes as tgf
import test_gpu_general_components as tgg
from test_gpu_general_components import ABSENT, FREE, RAW_BOUND, contract_evaluate, make_field, oracle_field, raw_error
from psfmc_amd import MultiComponentModel
from psfmc_amd.ModelComponents import Configuration, PointSource, Sersic, Sky
from psfmc_amd.distributions import Normal, Uniform

pytestmark = pytest.mark.gpu

KEYS = ('r_in', 'r_out', 'winding', 'alpha', 'inclination', 'sky_angle')
PACKED = ('alpha', 'inclination', 'r_in', 'r_out', 'sky_angle', 'winding')      # the attributes' alphabetical order
ALL_FREE = {k: FREE for k in KEYS}


def make_model(fld, spiral, fourier=None, boxiness=ABSENT, slope=ABSENT, degrees=True, backend='fused', max_walkers=16,
               storage='f64', lean=False, second=None):
    """Sky + PointSource + one Sersic with `spiral` = {key: FREE or a value} (None: no keyword) beside `fourier`,
    `boxiness`, `slope` as in tests/test_gpu_fourier_modes.py.  Free-parameter order: adu, [slope x 2], ps mag, [x, y],
    then the Sersic's [angle], [boxiness], [f<m>_amp, f<m>_phase per mode], index, mag, reff, reff_b, [spiral_alpha,
    spiral_incl, spiral_r_in, spiral_r_out, spiral_sky, spiral_wind], x, y.  The priors of the spiral are wider than
    its support.  lean: the point source's position and the Sersic's angle are constants.  second: keywords of a
    second Sersic (all its ordinary parameters free)."""
    ny, nx = fld['shape']
    c = np.array((nx / 2 + 0.5, ny / 2 + 0.5))
    wide = lambda: Uniform(loc=c - 2.0 * max(ny, nx), scale=4.0 * max(ny, nx) * np.ones(2))
    turn = 360.0 if degrees else 2 * np.pi
    kw = {}
    if spiral is not None:
        prior = {'r_in': lambda: Uniform(loc=-5.0, scale=65.0), 'r_out': lambda: Uniform(loc=-5.0, scale=205.0),
                 'winding': lambda: Uniform(loc=-4 * turn, scale=8 * turn), 'alpha': lambda: Uniform(loc=-1.0, scale=5.0),
                 'inclination': lambda: Uniform(loc=-turn / 2, scale=turn),
                 'sky_angle': lambda: Uniform(loc=-turn, scale=2 * turn)}
        kw['spiral'] = {k: prior[k]() if v is FREE else v for k, v in spiral.items()}
    if fourier is not None:
        kw['fourier'] = {m: (Uniform(loc=-1.0, scale=2.0) if a is FREE else a,
                             Uniform(loc=-2 * turn, scale=4 * turn) if p is FREE else p) for m, (a, p) in fourier.items()}
    if boxiness is not ABSENT:
        kw['boxiness'] = Uniform(loc=-1.5, scale=4.0) if boxiness is FREE else boxiness
    sky_kw = {} if slope is ABSENT else {'slope': Normal(loc=(0, 0), scale=(1e-3, 1e-3)) if slope is FREE else slope}

    def sersic(angle, **more):
        return Sersic(xy=wide(), mag=Uniform(loc=15.0, scale=10.0), reff=Uniform(loc=0.5, scale=40.0),
                      reff_b=Uniform(loc=0.5, scale=40.0), index=Uniform(loc=0.2, scale=8.0), angle=angle,
                      angle_degrees=degrees, **more)
    comps = [Configuration(fld['sci'], fld['ivm'], fld['psf'], fld['psf_ivm'], mag_zeropoint=fld['mag_zp']),
             Sky(adu=Normal(loc=0.05, scale=0.05), **sky_kw),
             PointSource(xy=(nx / 2 + 1.3, ny / 2 - 0.8) if lean else wide(), mag=Uniform(loc=16.0, scale=8.0)),
             sersic((30.0 if degrees else 0.5) if lean else Uniform(loc=-turn, scale=2 * turn), **kw)]
    if second is not None:
        comps.append(sersic(Uniform(loc=-turn, scale=2 * turn), **second))
    return MultiComponentModel(comps, backend=backend, max_walkers=max_walkers, storage=storage)


def theta_of(fld, s, adu=0.05, slope=None, ps_mag=19.0, lean=False, second=None):
    """One parameter vector; s: angle, [boxiness], four (the free Fourier values in packing order), index, mag, reff,
    reff_b, spi (a dict of the FREE spiral values by key), x, y."""
    ny, nx = fld['shape']
    t = [adu] + list(slope or []) + [ps_mag] + ([] if lean else [nx / 2 + 1.3, ny / 2 - 0.8])
    for k, c in enumerate([s] + ([second] if second else [])):
        t += ([] if lean and k == 0 else [c['angle']]) + ([c['boxiness']] if 'boxiness' in c else [])
        t += list(c.get('four', [])) + [c['index'], c['mag'], c['reff'], c['reff_b']]
        t += [c['spi'][key] for key in PACKED if key in c.get('spi', {})] + [c['x'], c['y']]
    return np.array(t, dtype=np.float64)


def column(model, name):
    names = sum(([n] * w for n, w in zip(model.param_names, model.param_lens)), [])
    return names.index(name)


def spi(r_in, r_out, winding, alpha=None, inclination=None, sky_angle=None):
    vals = dict(r_in=r_in, r_out=r_out, winding=winding, alpha=alpha, inclination=inclination, sky_angle=sky_angle)
    return {k: v for k, v in vals.items() if v is not None}


FIXED_TILT = dict(r_in=FREE, r_out=FREE, winding=FREE, alpha=FREE, inclination=35.0, sky_angle=20.0)


def contract_sets(fld):
    """[(model keywords, [vectors])]: the spiral alone in radians; beside a free boxiness, three modes and a tilted
    sky in degrees; with a fixed inclination and sky angle.  |winding| from 2 to 12 rad in both signs, alpha in
    {0, 0.3, 1.5}, inclination up to 70 degrees, r_in = 0 once, n in {0.5, 1, 4}, an axis along the pixel grid through
    x + 0.5, a centre on a pixel corner, centres outside the image."""
    ny, nx = fld['shape']
    cx, cy = nx // 2, ny // 2
    alone = [dict(spi=spi(0.0, 8.0, 2.0, 0.0, 0.6, 0.4), index=0.5, reff=6.0, reff_b=4.0, angle=0.5, x=cx + 0.31,
                  y=cy - 0.27),
             dict(spi=spi(3.0, 12.0, -12.0, 0.3, 0.0, 0.0), index=4.0, reff=5.0, reff_b=2.0, angle=0.0, x=float(cx),
                  y=cy + 0.5),                                                                     # u = 0 on col cx
             dict(spi=spi(5.0, 20.0, 2.0, 1.5, np.deg2rad(70.0), -1.0), index=1.0, reff=12.0, reff_b=9.0, angle=0.17,
                  x=-3.6, y=cy + 0.4)]                                                             # outside
    full = [dict(boxiness=-1.0, four=[0.2, 30.0, 0.3, -0.2, 100.0], spi=spi(2.0, 10.0, 300.0, 0.3, 40.0, -30.0), index=0.5,
                 reff=6.0, reff_b=4.0, angle=30.0, x=cx - 2.4, y=cy + 1.7),
            dict(boxiness=0.0, four=[0.1, -50.0, 0.2, 0.1, 10.0], spi=spi(3.0, 7.0, -200.0, 0.0, 0.0, 0.0), index=1.0,
                 reff=4.0, reff_b=3.0, angle=-90.0, x=cx + 0.5, y=float(cy)),                      # v = 0 on row cy
            dict(boxiness=0.7, four=[0.3, 200.0, -0.3, 0.3, -120.0], spi=spi(4.0, 9.0, -690.0, 0.0, 70.0, 65.0), index=4.0,
                 reff=7.0, reff_b=6.0, angle=45.0, x=cx + 0.5, y=cy - 0.5),                        # a pixel corner
            dict(boxiness=2.0, four=[-0.2, 75.0, 0.1, -0.1, 5.0], spi=spi(10.0, 40.0, 115.0, 1.5, 20.0, 10.0), index=1.0,
                 reff=20.0, reff_b=8.0, angle=60.0, x=nx + 5.0, y=ny + 2.5)]                       # outside
    tilt = [dict(spi=spi(1.0, 6.0, 450.0, 0.3), index=1.0, reff=8.0, reff_b=3.0, angle=-20.0, x=cx + 3.2, y=cy - 1.1),
            dict(spi=spi(5.0, 15.0, -150.0, 0.0), index=4.0, reff=3.0, reff_b=1.5, angle=110.0, x=cx + 0.25, y=cy + 0.4)]
    out, i = [], 0
    for kw, cases, slope in ((dict(spiral=ALL_FREE, degrees=False), alone, False),
                             (dict(spiral=ALL_FREE, fourier=tgf.THREE, boxiness=FREE, slope=FREE), full, True),
                             (dict(spiral=FIXED_TILT), tilt, False)):
        vecs = []
        for r in cases:
            r['mag'] = 18.0 + 0.3 * i
            vecs.append(theta_of(fld, r, adu=0.05 + 0.002 * i,
                                 slope=(0.02 / nx * (1 - i % 3), 0.02 / ny * (-0.75 + 0.25 * i)) if slope else None))
            i += 1
        out.append((kw, np.array(vecs)))
    return out


@pytest.mark.parametrize('backend,shape', [('fused', s) for s in tgg.SHAPES] + [('hipfft', (64, 64)), ('hipfft', (70, 66))],
                         ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_device_against_the_contract(backend, shape):
    """The shapes of tests/test_gpu_general_components.py (log2 + exp2 form, power tables, embedded, k_rows3_fwd EXTRA,
    hipfft).  Raw image per pixel (RAW_BOUND: the worst measured error, 8.3e-14 in DESIGN.md section 17, is below a
    third of it), the five images to 1e-12 of the image maximum, the log-posterior through raw vectors and the
    log-likelihood through the host path's rows against the contract (1e-9)."""
    fld = make_field(*shape, seed=1)
    field = oracle_field(fld)
    worst = 0.0
    for n_set, (kw, thetas) in enumerate(contract_sets(fld)):
        model = make_model(fld, backend=backend, **kw)
        imgs = model.sample_images(thetas)
        lp = model.log_posterior_batch(thetas)
        ll_rows = model.log_likelihood_batch(thetas)
        prior = model.log_priors_batch(thetas)
        for i, t in enumerate(thetas):
            want_ll, want = contract_evaluate(model, field, t)
            tag = '%s %dx%d set %d case %d' % ((backend,) + shape + (n_set, i))
            worst = max(worst, raw_error(imgs['raw_model'][i], want['raw_model'], tag))
            for kind in want:
                scale = np.max(np.abs(want[kind]))
                assert np.max(np.abs(imgs[kind][i] - want[kind])) <= 1e-12 * scale, (kind, tag)
            assert np.isfinite(want_ll) and np.isfinite(prior[i])
            assert abs(ll_rows[i] - want_ll) <= 1e-9 * abs(want_ll), (tag, ll_rows[i], want_ll)
            assert abs(lp[i] - (want_ll + prior[i])) <= 1e-9 * abs(want_ll), (tag, lp[i], want_ll + prior[i])
        model.close()
    print('%s %dx%d: worst raw-model relative error %.2e' % ((backend,) + shape + (worst,)))
    assert worst <= RAW_BOUND


FIXED_MODES = {1: (0.2, 30.0), 3: (-0.15, 110.0)}


def test_zero_winding_against_the_model_without_the_keyword():
    """spiral={r_in: 2, r_out: 9, winding: 0} (no inclination, no sky angle) beside a free boxiness and two modes
    against the same model without the keyword: log-posteriors agree to RAW_BOUND carried through the likelihood
    (the bound of tests/test_gpu_fourier_modes.py); the expected difference is 0."""
    fld = make_field(64, 64, seed=2)
    wound = make_model(fld, dict(r_in=2.0, r_out=9.0, winding=0.0), fourier=FIXED_MODES, boxiness=FREE)
    flat = make_model(fld, None, fourier=FIXED_MODES, boxiness=FREE)
    assert wound.param_names == flat.param_names and wound.sersic_spiral_flags == [True]
    thetas = np.array([np.delete(t, [1, 2]) for t in tgg.contract_cases(fld)])       # (no slope here)
    a, b = wound.log_posterior_batch(thetas), flat.log_posterior_batch(thetas)
    imgs = flat.sample_images(thetas, ('convolved_model', 'composite_ivm'))
    sci = fld['sci'].astype(np.float64)
    for i in range(len(thetas)):
        m, w = imgs['convolved_model'][i], imgs['composite_ivm'][i]
        r = sci - m
        bound = RAW_BOUND * 0.5 * float(np.sum(2 * np.abs(r) * np.abs(m) * w + 2 * r * r * w + 2))
        print('case %d: |difference| %.3e, bound %.3e' % (i, abs(a[i] - b[i]), bound))
        assert np.isfinite(b[i]) and abs(a[i] - b[i]) <= bound, (i, a[i], b[i])
    wound.close()
    flat.close()


def _violations(model, good):
    """[(what, vector)]: each condition of the support violated in turn (a model in degrees)."""
    out = []
    for name, val, what in (('spiral_r_in', -0.5, 'r_in < 0'), ('spiral_r_out', 1.5, 'r_out < r_in'),
                            ('spiral_r_out', 2.0, 'r_out = r_in'), ('spiral_alpha', -0.1, 'alpha < 0'),
                            ('spiral_incl', 90.0, 'inclination = 90 degrees'), ('spiral_incl', -100.0, 'inclination < -90'),
                            ('spiral_wind', np.nan, 'winding NaN'), ('spiral_sky', np.inf, 'sky angle inf'),
                            ('spiral_r_out', np.inf, 'r_out inf'), ('spiral_alpha', np.nan, 'alpha NaN')):
        v = good.copy()
        v[column(model, '2_Sersic_' + name)] = val
        out.append((what, v))
    return out


def test_batch_independence_and_the_support_of_the_spiral():
    """A walker's log-posterior bits are the same alone, in a batch of 16 and in permuted order; every violation of
    the support is -inf from raw vectors, leaves the other walkers unchanged, and is NaN through a row-based call
    (no writable flags there)."""
    fld = make_field(64, 64, seed=4)
    kw, base = contract_sets(fld)[1]
    model = make_model(fld, max_walkers=32, **kw)
    rng = np.random.RandomState(5)
    thetas = base[rng.randint(0, len(base), 16)] + rng.normal(size=(16, base.shape[1])) * 1e-3
    re, rb = column(model, '2_Sersic_reff'), column(model, '2_Sersic_reff_b')
    thetas[:, rb] = np.minimum(thetas[:, rb], thetas[:, re] - 1e-3)
    thetas[:, column(model, '2_Sersic_spiral_alpha')] = np.abs(thetas[:, column(model, '2_Sersic_spiral_alpha')])
    thetas[:, column(model, '2_Sersic_spiral_incl')] = np.abs(thetas[:, column(model, '2_Sersic_spiral_incl')])
    full = model.log_posterior_batch(thetas)
    assert np.all(np.isfinite(full))
    for i in (0, 7, 15):
        assert model.log_posterior_batch(thetas[i:i + 1])[0] == full[i]
    perm = rng.permutation(16)
    assert np.array_equal(model.log_posterior_batch(thetas[perm]), full[perm])
    good = thetas[0].copy()
    good[column(model, '2_Sersic_spiral_r_in')] = 2.0
    good[column(model, '2_Sersic_spiral_r_out')] = 10.0
    bad = _violations(model, good)
    mixed = thetas.copy()
    where = list(range(1, 16))[:len(bad)]
    for k, (_, v) in zip(where, bad):
        mixed[k] = v
    got = model.log_posterior_batch(mixed)
    keep = np.ones(16, dtype=bool)
    keep[where] = False
    for k, (what, _) in zip(where, bad):
        assert got[k] == -np.inf, what
    assert np.array_equal(got[keep], full[keep])
    assert np.all(model.log_posterior_batch_host(mixed)[where] == -np.inf)
    vecs = np.array([v for _, v in bad])
    rows = model.engine.loglike(model.derived_rows(vecs), aux=model.aux_rows(vecs))
    for (what, _), r in zip(bad, rows):
        assert np.isnan(r), what
    assert np.isfinite(model.engine.loglike(model.derived_rows(good[None]), aux=model.aux_rows(good[None]))[0])
    model.close()


def _fourier_reference():
    """(log-posteriors, 20-iteration device chain, its log-probabilities) of a model with modes and a boxiness."""
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(64, 64, seed=7)
    model = tgf.make_model(fld, tgf.LEAN_MODES, max_walkers=32, lean=True)
    p0 = tgf._lean_start(fld, 32, 2)
    lp = model.log_posterior_batch(p0)
    s = DeviceEnsembleSampler(32, model, block=5)
    s.random_state = np.random.RandomState(3).get_state()
    list(s.sample(p0, iterations=20))
    out = lp, s.chain.copy(), s.lnprobability.copy()
    model.close()
    return out


def test_default_boxiness_and_fourier_models_are_untouched_by_spiral_contexts():
    """Models without the keyword -- plain, boxiness-only, with modes: bit-identical log-posteriors and 20-iteration
    device chains before and after spiral contexts lived and died in the process."""
    before = tgg._plain_reference()[2], tgf._boxiness_reference(), _fourier_reference()
    fld = make_field(64, 64, seed=3)
    alive = []
    for kw, thetas in contract_sets(fld):
        alive.append(make_model(fld, **kw))
        assert np.all(np.isfinite(alive[-1].log_posterior_batch(thetas)))
    alive.pop().close()
    after = tgg._plain_reference()[2], tgf._boxiness_reference(), _fourier_reference()
    for m in alive:
        m.close()
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            assert np.array_equal(a, b)
        assert np.all(np.isfinite(y[0]))


LEAN_SPIRAL = dict(r_in=2.0, r_out=FREE, winding=FREE)                  # 11 free parameters with `lean`


def _lean_start(fld, n_w, seed, winding=120.0):
    s = dict(spi=dict(r_out=9.0, winding=winding), index=1.5, mag=18.0, reff=6.0, reff_b=3.0, x=32.3, y=30.8)
    base = theta_of(fld, s, lean=True)
    rng = np.random.RandomState(seed)
    p0 = base + rng.normal(size=(n_w, len(base))) * 1e-2
    p0[:, 5] = np.minimum(p0[:, 5], p0[:, 4] - 1e-3)
    return p0


@pytest.mark.parametrize('n_w', [22, 64])
def test_device_sampler_equals_the_host_sampler(n_w):
    """The device-resident chain equals the host loop's fed the device's own log-posteriors, bit for bit (22 walkers:
    the whole-iteration route of small ensembles; 64: half-steps)."""
    from psfmc_amd.sampler import EnsembleSampler, DeviceEnsembleSampler
    fld = make_field(64, 64, seed=7)
    model = make_model(fld, LEAN_SPIRAL, max_walkers=n_w, lean=True)
    assert model.num_params == 10
    p0 = _lean_start(fld, n_w, 2)
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
    """Four rungs, ten iterations: chain, log-probabilities, log-likelihoods, acceptances and swaps equal the host
    contract's (tests/test_gpu_tempered.py compares them so)."""
    from psfmc_amd.sampler import TemperedEnsembleSampler, DeviceTemperedSampler, default_betas
    fld = make_field(64, 64, seed=8)
    model = make_model(fld, LEAN_SPIRAL, max_walkers=4 * 24, lean=True)
    betas = default_betas(4, 50.0)
    p0 = _lean_start(fld, 4 * 24, 3).reshape(4, 24, -1)
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
    model.close()


@pytest.mark.parametrize('backend', ['fused', 'hipfft'])
def test_mixed_models(backend):
    """A spiral component beside a pixel-integrated one: the integrated kernels write the extra image, the general one
    adds (1e-10 per pixel, the integrated profile's own bound); a spiral component beside a boxiness-only one: the
    other runs the loop without the rotation in the same launch (RAW_BOUND)."""
    fld = make_field(64, 64, seed=6)
    field = oracle_field(fld)
    model = make_model(fld, ALL_FREE, boxiness=FREE, backend=backend, max_walkers=8, second=dict(integrate=True))
    a = dict(boxiness=0.8, spi=spi(2.0, 10.0, 300.0, 0.3, 40.0, -30.0), index=1.0, mag=18.0, reff=6.0, reff_b=4.0,
             angle=30.0, x=32.3, y=30.8)
    b = dict(index=3.0, mag=18.5, reff=4.0, reff_b=2.0, angle=100.0, x=29.5, y=32.5)
    thetas = np.array([theta_of(fld, a, second=b), theta_of(fld, dict(a, x=32.5), second=dict(b, y=32.0))])
    imgs = model.sample_images(thetas, ('raw_model',))['raw_model']
    lp = model.log_posterior_batch(thetas)
    prior = model.log_priors_batch(thetas)
    for i, t in enumerate(thetas):
        want_ll, want = contract_evaluate(model, field, t)
        assert raw_error(imgs[i], want['raw_model'], '%s mixed %d' % (backend, i)) <= 1e-10
        assert abs(lp[i] - (want_ll + prior[i])) <= 1e-9 * abs(want_ll)
    model.close()
    model = make_model(fld, ALL_FREE, boxiness=FREE, backend=backend, max_walkers=8, second=dict(boxiness=0.4))
    imgs = model.sample_images(thetas, ('raw_model',))['raw_model']
    for i, t in enumerate(thetas):
        want = contract_evaluate(model, field, t)[1]
        assert raw_error(imgs[i], want['raw_model'], '%s two general %d' % (backend, i)) <= RAW_BOUND
    model.close()


def test_accumulated_images_against_the_contract():
    fld = make_field(70, 66, seed=9)
    kw, thetas = contract_sets(fld)[1]
    model = make_model(fld, **kw)
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


@pytest.mark.parametrize('order', [(0, 1), (1, 0)], ids=['spiral-first', 'spiral-last'])
def test_field_set_keeps_the_spiral_per_field(order):
    """A 64x64 field with a spiral (fixed values: the same free parameters) and a 96x64 field with a boxiness alone,
    registered in either order, against each field's own context as tests/test_gpu_fourier_modes.py compares them."""
    from psfmc_amd.models import FieldSet
    flds = [make_field(64, 64, seed=10), make_field(96, 64, seed=11)]
    kws = [dict(spiral=dict(r_in=2.0, r_out=9.0, winding=200.0, alpha=0.3, inclination=35.0, sky_angle=-20.0), boxiness=0.6),
           dict(spiral=None, boxiness=-0.4)]
    flds, kws = [flds[i] for i in order], [kws[i] for i in order]
    fs = FieldSet([make_model(f, max_walkers=1, **kw) for f, kw in zip(flds, kws)], max_walkers=32)
    own = [make_model(f, max_walkers=16, **kw) for f, kw in zip(flds, kws)]
    thetas = [np.array([np.delete(t, [1, 2, 7]) for t in tgg.contract_cases(f)]) for f in flds]
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


def test_joint_model_shared_winding_and_own_sky_angles():
    from psfmc_amd import JointModel
    fa, fb = make_field(64, 64, seed=12), make_field(70, 66, seed=13)
    kw = dict(spiral=ALL_FREE, fourier=tgf.THREE, boxiness=FREE)
    joint = JointModel([make_model(fa, max_walkers=1, **kw), make_model(fb, max_walkers=1, **kw)],
                       per_field=['2_Sersic_spiral_sky', '1_PointSource_xy', '2_Sersic_xy'], max_walkers=32)
    names = joint.param_names
    assert names.count('2_Sersic_spiral_wind') == 1 and '2_Sersic_spiral_sky_f1' in names
    base = contract_sets(fa)[1][1]
    own_b = contract_sets(fb)[1][1]
    keep = [i for i in range(base.shape[1]) if i not in (1, 2)]                    # (no slope in these models)
    thetas = np.zeros((len(base), joint.num_params))
    thetas[:, joint.field_columns(1)] = own_b[:, keep]
    thetas[:, joint.field_columns(0)] = base[:, keep]
    got = joint.log_posterior_batch(thetas)
    prior = joint.log_priors_batch(thetas)
    field_a, field_b = oracle_field(fa), oracle_field(fb)
    own_a_model, own_b_model = make_model(fa, max_walkers=1, **kw), make_model(fb, max_walkers=1, **kw)
    for i, t in enumerate(thetas):
        ll_a = contract_evaluate(own_a_model, field_a, joint.field_theta(t, 0)[0])[0]
        ll_b = contract_evaluate(own_b_model, field_b, joint.field_theta(t, 1)[0])[0]
        want = (ll_a + ll_b) + prior[i]
        assert np.isfinite(want) and abs(got[i] - want) <= 1e-9 * abs(want), (i, got[i], want)
    assert joint.log_posterior_batch(thetas[1:2])[0] == got[1]
    bad = thetas[:1].copy()
    bad[0, joint.field_columns(0)[column(own_a_model, '2_Sersic_spiral_alpha')]] = -0.5
    assert joint.log_posterior_batch(bad)[0] == -np.inf                           # the shared alpha: outside the support
    joint.close()
    own_a_model.close()
    own_b_model.close()


def test_f32_storage_and_context_group():
    """storage='f32' within its documented 2e-6; a ContextGroup on one device equals the plain context through raw
    vectors and refuses derived rows with the keyword named."""
    fld = make_field(64, 64, seed=14)
    field = oracle_field(fld)
    kw, thetas = contract_sets(fld)[1]
    f32 = make_model(fld, storage='f32', **kw)
    ll = f32.log_likelihood_batch(thetas)
    lp32 = f32.log_posterior_batch(thetas)
    prior = f32.log_priors_batch(thetas)
    for i, t in enumerate(thetas):
        want_ll, _ = contract_evaluate(f32, field, t)
        assert abs(ll[i] - want_ll) <= 2e-6 * abs(want_ll) and abs(lp32[i] - want_ll - prior[i]) <= 2e-6 * abs(want_ll)
    f32.close()
    for kw, thetas in (contract_sets(fld)[0], contract_sets(fld)[1]):          # (without and with the Fourier call)
        model = make_model(fld, **kw)
        grp = model.device_group([0], max_walkers=16)
        got = grp.logpost_theta(thetas)
        assert np.all(np.isfinite(got)) and np.array_equal(got, model.log_posterior_batch(thetas))
        with pytest.raises(NotImplementedError, match='spiral'):
            grp.loglike(model.derived_rows(thetas), aux=model.aux_rows(thetas))
        grp.close()
        model.close()


def test_the_library_refuses_what_the_header_says():
    from psfmc_amd.engine import NativeError
    fld = make_field(64, 64, seed=15)
    inside = [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    model = make_model(fld, dict(r_in=2.0, r_out=9.0, winding=100.0), max_walkers=4)
    with pytest.raises(NativeError, match='column'):
        model.engine.set_spiral_layout([True], [model.num_params] + [-1] * 5, inside)
    with pytest.raises(NativeError, match='n_sersic'):
        model.engine.set_spiral_layout([True, False], [-1] * 12, inside * 2)
    model.close()
    plain = make_model(fld, None, max_walkers=4)
    with pytest.raises(NativeError, match='aux layout'):
        plain.engine.set_spiral_layout([True], [-1] * 6, inside)
    plain.close()
    integ = tgg.make_model(fld, boxiness=(ABSENT,), integrate=(True,), max_walkers=4)     # (a tilted sky: an aux layout)
    with pytest.raises(NativeError, match='integrated'):
        integ.engine.set_spiral_layout([True], [-1] * 6, inside)
    integ.close()
    two = make_model(fld, None, slope=FREE, max_walkers=4)                                # (aux layout, Sersic not general)
    with pytest.raises(NativeError, match='general'):
        two.engine.set_spiral_layout([True], [-1] * 6, inside)
    two.close()


def test_a_planted_two_armed_host_is_recovered():
    """sci = the contract's convolved image of a bar (r_b / r_e = 0.3) wound by 3 rad along a wide ramp (r_in = 0,
    r_out = 20) plus the helper's fixed-seed noise: the log-posterior at the planted vector exceeds the one with
    winding 0, and a 200-iteration, 32-walker device chain started around winding 0 (scatter 0.3 rad) ends (median of
    its last 50 iterations) nearer 3 than 0.  (The wide ramp matters: a bar turned by 3 rad is nearly a bar turned
    by 3 - pi, so with a narrow ramp the outer isophotes hold the chain in a mode near -0.14 rad; with the wide one
    the inner isophotes, which turn in proportion to the winding, lead it to the planted value.)"""
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(64, 64, seed=16)
    noise = fld['sci'].astype(np.float64) - 0.05
    kw = dict(spiral=dict(r_in=0.0, r_out=FREE, winding=FREE), degrees=False, lean=True)
    truth = dict(spi=dict(r_out=20.0, winding=3.0), index=1.0, mag=18.5, reff=10.0, reff_b=3.0, x=32.3, y=30.8)
    planted = theta_of(fld, truth, lean=True)
    first = make_model(fld, max_walkers=1, **kw)
    conv = contract_evaluate(first, oracle_field(fld), planted)[1]['convolved_model']
    first.close()
    model = make_model(dict(fld, sci=(conv + noise).astype(np.float32)), max_walkers=32, **kw)
    wind = model.param_names.index('2_Sersic_spiral_wind')
    flat = planted.copy()
    flat[wind] = 0.0
    lp = model.log_posterior_batch(np.array([planted, flat]))
    print('log-posterior at the planted vector %.2f, with winding 0 %.2f' % (lp[0], lp[1]))
    assert np.isfinite(lp[1]) and lp[0] > lp[1]
    rng = np.random.RandomState(4)
    scale = np.full(len(flat), 1e-2)
    scale[0], scale[wind] = 1e-3, 0.3
    p0 = flat + rng.normal(size=(32, len(flat))) * scale
    s = DeviceEnsembleSampler(32, model, block=50)
    s.random_state = np.random.RandomState(5).get_state()
    list(s.sample(p0, iterations=200))
    med = float(np.median(s.chain[:, -50:, wind]))
    print('median winding of the last 50 iterations: %.3f' % med)
    assert abs(med - 3.0) < abs(med)
    model.close()
