"""Azimuthal Fourier modes on Sersic isophotes on the device, held to the numpy definition (`Sersic.fourier_image`)
composed with the oracle's point source, convolution and likelihood: raw images per pixel on every forward-kernel
family of both back ends, zero amplitudes against the boxiness-only model, batch independence and the support, the
untouched default, the samplers, mixed models, posterior sums, field sets, joint fits, f32 storage, context groups
and a planted lopsided host.  Field and contract helpers are those of tests/test_gpu_general_components.py."""
import numpy as np
import pytest

import test_gpu_general_components as tgg
from test_gpu_general_components import ABSENT, FREE, RAW_BOUND, contract_evaluate, make_field, oracle_field, raw_error
from psfmc_amd import MultiComponentModel
from psfmc_amd.ModelComponents import Configuration, PointSource, Sersic, Sky
from psfmc_amd.distributions import Normal, Uniform

pytestmark = pytest.mark.gpu


def make_model(fld, fourier, boxiness=ABSENT, slope=ABSENT, degrees=True, backend='fused', max_walkers=16,
               storage='f64', lean=False, second=None):
    """Sky + PointSource + one Sersic with `fourier` = {m: (amplitude, phase)}, FREE standing for the test's prior (a
    fresh object per model) and `fourier` None for no keyword; `boxiness`, `slope`: FREE, a value or ABSENT.
    Free-parameter order: adu, [slope x 2], ps mag, [x, y], then the Sersic's [angle], [boxiness], [f<m>_amp,
    f<m>_phase per mode], index, mag, reff, reff_b, x, y.  lean: the point source's position and the Sersic's angle
    are constants.  second: keywords of a second Sersic (all its ordinary parameters free)."""
    ny, nx = fld['shape']
    c = np.array((nx / 2 + 0.5, ny / 2 + 0.5))
    wide = lambda: Uniform(loc=c - 2.0 * max(ny, nx), scale=4.0 * max(ny, nx) * np.ones(2))
    turn = 360.0 if degrees else 2 * np.pi
    kw = {}
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
    reff_b, x, y."""
    ny, nx = fld['shape']
    t = [adu] + list(slope or []) + [ps_mag] + ([] if lean else [nx / 2 + 1.3, ny / 2 - 0.8])
    for k, c in enumerate([s] + ([second] if second else [])):
        t += ([] if lean and k == 0 else [c['angle']]) + ([c['boxiness']] if 'boxiness' in c else [])
        t += list(c.get('four', [])) + [c['index'], c['mag'], c['reff'], c['reff_b'], c['x'], c['y']]
    return np.array(t, dtype=np.float64)


ONE = {1: (FREE, FREE)}
THREE = {1: (FREE, FREE), 3: (FREE, 25.0), 4: (FREE, FREE)}           # one constant phase among free ones
SIX = {m: (FREE, FREE) for m in range(1, 7)}


def contract_sets(fld):
    """[(model keywords, [vectors])]: one mode in radians without boxiness, three and six modes in degrees with it --
    sum |a| up to 0.9, c in {-1, 0, 0.7, 2} and more, n in {0.5, 1, 4}, an axis along the pixel grid through
    x + 0.5 (u or v exactly 0 on a pixel line), a centre on a pixel corner, centres outside the image."""
    ny, nx = fld['shape']
    cx, cy = nx // 2, ny // 2
    one = [dict(four=[0.3, 0.8], index=0.5, reff=6.0, reff_b=4.0, angle=0.5, x=cx + 0.31, y=cy - 0.27),
           dict(four=[-0.6, 2.0], index=4.0, reff=5.0, reff_b=2.0, angle=0.0, x=float(cx), y=cy + 0.5),     # u = 0 on col cx
           dict(four=[0.9, -1.0], index=1.0, reff=12.0, reff_b=9.0, angle=0.17, x=-3.6, y=cy + 0.4)]        # outside
    three = [dict(boxiness=-1.0, four=[0.2, 30.0, 0.3, -0.2, 100.0], index=0.5, reff=6.0, reff_b=4.0, angle=30.0,
                  x=cx - 2.4, y=cy + 1.7),
             dict(boxiness=0.0, four=[0.1, -50.0, 0.2, 0.1, 10.0], index=1.0, reff=4.0, reff_b=3.0, angle=-90.0,
                  x=cx + 0.5, y=float(cy)),                                                                # v = 0 on row cy
             dict(boxiness=0.7, four=[0.3, 200.0, -0.3, 0.3, -120.0], index=4.0, reff=7.0, reff_b=6.0, angle=45.0,
                  x=cx + 0.5, y=cy - 0.5),                                                                  # a pixel corner
             dict(boxiness=2.0, four=[-0.2, 75.0, 0.1, -0.1, 5.0], index=1.0, reff=20.0, reff_b=8.0, angle=60.0,
                  x=nx + 5.0, y=ny + 2.5)]                                                                  # outside
    six = [dict(boxiness=0.7, four=[0.2, 10.0, -0.15, 40.0, 0.15, -70.0, 0.1, 130.0, -0.15, 20.0, 0.15, -160.0],
                index=1.0, reff=8.0, reff_b=3.0, angle=-20.0, x=cx + 3.2, y=cy - 1.1),                     # sum |a| = 0.9
           dict(boxiness=-0.5, four=[0.05, 300.0, 0.1, -15.0, 0.02, 45.0, 0.08, 90.0, 0.03, -33.0, 0.04, 71.0],
                index=4.0, reff=3.0, reff_b=1.5, angle=110.0, x=cx + 0.25, y=cy + 0.4),
           dict(boxiness=1.3, four=[-0.1, 0.0, 0.1, 60.0, -0.1, 120.0, 0.1, 180.0, -0.1, 240.0, 0.1, 300.0],
                index=0.5, reff=9.0, reff_b=7.0, angle=75.0, x=cx - 1.6, y=cy + 2.2)]
    out, i = [], 0
    for kw, cases, slope in ((dict(fourier=ONE, degrees=False), one, False),
                             (dict(fourier=THREE, boxiness=FREE, slope=FREE), three, True),
                             (dict(fourier=SIX, boxiness=FREE), six, False)):
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
    hipfft).  Raw image per pixel (RAW_BOUND), the five images to 1e-12 of the image maximum, the log-posterior through
    raw vectors and the log-likelihood through the host path's rows against the contract (1e-9)."""
    fld = make_field(*shape, seed=1)
    field = oracle_field(fld)
    worst = 0.0
    for kw, thetas in contract_sets(fld):
        model = make_model(fld, backend=backend, **kw)
        imgs = model.sample_images(thetas)
        lp = model.log_posterior_batch(thetas)
        ll_rows = model.log_likelihood_batch(thetas)
        prior = model.log_priors_batch(thetas)
        for i, t in enumerate(thetas):
            want_ll, want = contract_evaluate(model, field, t)
            tag = '%s %dx%d %d modes case %d' % ((backend,) + shape + (len(kw['fourier']), i))
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


def test_zero_amplitudes_against_the_boxiness_only_model():
    """fourier={1: (0, 0), 3: (0, 0.4)} beside boxiness against boxiness alone: log-posteriors agree to RAW_BOUND
    carried through the likelihood (the bound of test_zero_boxiness_and_slope_against_the_plain_rasteriser)."""
    fld = make_field(64, 64, seed=2)
    modes = make_model(fld, {1: (0.0, 0.0), 3: (0.0, 0.4)}, boxiness=FREE)
    box = make_model(fld, None, boxiness=FREE)
    assert modes.param_names == box.param_names and modes.sersic_fourier_masks == [0b101]
    thetas = np.array([np.delete(t, [1, 2]) for t in tgg.contract_cases(fld)])       # (no slope here)
    a, b = modes.log_posterior_batch(thetas), box.log_posterior_batch(thetas)
    imgs = box.sample_images(thetas, ('convolved_model', 'composite_ivm'))
    sci = fld['sci'].astype(np.float64)
    for i in range(len(thetas)):
        m, w = imgs['convolved_model'][i], imgs['composite_ivm'][i]
        r = sci - m
        bound = RAW_BOUND * 0.5 * float(np.sum(2 * np.abs(r) * np.abs(m) * w + 2 * r * r * w + 2))
        print('case %d: |difference| %.3e, bound %.3e' % (i, abs(a[i] - b[i]), bound))
        assert np.isfinite(b[i]) and abs(a[i] - b[i]) <= bound, (i, a[i], b[i])
    modes.close()
    box.close()


def _spread(fld, kw_cases, n_w, seed, scale=1e-3):
    """n_w vectors scattered about the cases of one contract set."""
    base = kw_cases[1]
    rng = np.random.RandomState(seed)
    return base[rng.randint(0, len(base), n_w)] + rng.normal(size=(n_w, base.shape[1])) * scale


def test_batch_independence_and_the_support_of_the_modes():
    """A walker's log-posterior bits are the same alone, in a batch of 37 and across a pass boundary; a walker with
    sum |a| >= 1 and one with an on-pixel centre are -inf and leave the others unchanged."""
    fld = make_field(64, 64, seed=4)
    kw, base = contract_sets(fld)[1]
    model = make_model(fld, max_walkers=64, **kw)
    thetas = _spread(fld, (kw, base), 37, 5)
    names = sum(([n] * w for n, w in zip(model.param_names, model.param_lens)), [])
    re, rb = names.index('2_Sersic_reff'), names.index('2_Sersic_reff_b')
    thetas[:, rb] = np.minimum(thetas[:, rb], thetas[:, re] - 1e-3)
    full = model.log_posterior_batch(thetas)
    assert np.all(np.isfinite(full))
    for i in (0, 17, 36):
        assert model.log_posterior_batch(thetas[i:i + 1])[0] == full[i]
    bad = thetas.copy()
    a1, a3, a4 = (names.index('2_Sersic_f%d_amp' % m) for m in (1, 3, 4))
    bad[5, [a1, a3, a4]] = 0.5, -0.3, 0.2                              # sum |a| = 1
    bad[20, a4] = 1.5
    bad[30, names.index('2_Sersic_xy'):names.index('2_Sersic_xy') + 2] = 31.0, 33.0      # an on-pixel centre
    mixed = model.log_posterior_batch(bad)
    keep = np.ones(37, dtype=bool)
    keep[[5, 20, 30]] = False
    assert np.all(mixed[~keep] == -np.inf) and np.array_equal(mixed[keep], full[keep])
    host = model.log_posterior_batch_host(bad)
    assert np.all(host[[5, 20]] == -np.inf) and np.all(np.isfinite(host[keep]))
    model.engine.set_option('chunk_walkers', 5)
    assert model.engine.pass_size(37) <= 5
    assert np.array_equal(model.log_posterior_batch(thetas), full)
    model.close()


def _boxiness_reference():
    """(log-posteriors, 20-iteration device chain, its log-probabilities) of a boxiness-only model."""
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(64, 64, seed=3)
    base = tgg.contract_cases(fld)[:4]
    rng = np.random.RandomState(1)
    thetas = base[rng.randint(0, 4, 32)] + rng.normal(size=(32, base.shape[1])) * 1e-2
    thetas[:, 1:3] *= 1e-1
    thetas[:, 11] = np.minimum(thetas[:, 11], thetas[:, 10] - 1e-3)
    model = tgg.make_model(fld, max_walkers=32)
    lp = model.log_posterior_batch(thetas)
    s = DeviceEnsembleSampler(32, model, block=5)
    s.random_state = np.random.RandomState(3).get_state()
    list(s.sample(thetas, iterations=20))
    out = lp, s.chain.copy(), s.lnprobability.copy()
    model.close()
    return out


def test_default_and_boxiness_are_untouched_by_fourier_contexts_in_the_process(tmp_path):
    """A model without the keywords: bit-identical log-posteriors and 20-iteration device chain in a FRESH process, in
    which no Fourier-bearing context was ever created (a child process: that is what this test is about), and in this
    one after Fourier-bearing contexts lived and died in it; the same for a boxiness-only model within this process."""
    import os
    import subprocess
    import sys
    ref = os.path.join(str(tmp_path), 'plain.npz')
    code = ('import numpy as np, test_gpu_general_components as t; _, _, out = t._plain_reference(); '
            'np.savez(%r, lp=out[0], chain=out[1], lnp=out[2])' % ref)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    subprocess.run([sys.executable, '-c', code], env=env, check=True, timeout=120)
    before = np.load(ref)
    box_before = _boxiness_reference()
    fld = make_field(64, 64, seed=3)
    alive = []
    for kw, thetas in contract_sets(fld):
        alive.append(make_model(fld, **kw))
        assert np.all(np.isfinite(alive[-1].log_posterior_batch(thetas)))
    alive.pop().close()
    after = tgg._plain_reference()[2]
    box_after = _boxiness_reference()
    for m in alive:
        m.close()
    for key, y in zip(('lp', 'chain', 'lnp'), after):
        assert np.array_equal(before[key], y), key
    for x, y in zip(box_before, box_after):
        assert np.array_equal(x, y)
    assert np.all(np.isfinite(after[0])) and np.all(np.isfinite(box_after[0]))


LEAN_MODES = {1: (FREE, FREE), 3: (FREE, 25.0)}                       # 11 free parameters with `lean`


def _lean_start(fld, n_w, seed):
    s = dict(four=[0.15, 40.0, 0.1], index=1.5, mag=18.0, reff=6.0, reff_b=4.0, x=32.3, y=30.8)
    base = theta_of(fld, s, lean=True)
    rng = np.random.RandomState(seed)
    p0 = base + rng.normal(size=(n_w, len(base))) * 1e-2
    p0[:, 8] = np.minimum(p0[:, 8], p0[:, 7] - 1e-3)
    return p0


@pytest.mark.parametrize('n_w', [22, 64])
def test_device_sampler_equals_the_host_sampler(n_w):
    """The device-resident chain equals the host loop's fed the device's own log-posteriors, bit for bit (22 walkers:
    the whole-iteration route of small ensembles; 64: half-steps)."""
    from psfmc_amd.sampler import EnsembleSampler, DeviceEnsembleSampler
    fld = make_field(64, 64, seed=7)
    model = make_model(fld, LEAN_MODES, max_walkers=n_w, lean=True)
    assert model.num_params == 11
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
    model = make_model(fld, LEAN_MODES, max_walkers=4 * 24, lean=True)
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
def test_mixed_model_with_a_pixel_integrated_component(backend):
    """One Sersic with modes beside one pixel-integrated Sersic: the integrated kernels write the extra image, the
    general one adds (the bounds of test_mixed_models: 1e-10 per pixel, the integrated profile's own)."""
    fld = make_field(64, 64, seed=6)
    field = oracle_field(fld)
    model = make_model(fld, THREE, boxiness=FREE, backend=backend, max_walkers=8, second=dict(integrate=True))
    a = dict(boxiness=0.8, four=[0.2, 30.0, 0.3, -0.2, 100.0], index=1.0, mag=18.0, reff=6.0, reff_b=4.0, angle=30.0,
             x=32.3, y=30.8)
    b = dict(index=3.0, mag=18.5, reff=4.0, reff_b=2.0, angle=100.0, x=29.5, y=32.5)
    thetas = np.array([theta_of(fld, a, second=b), theta_of(fld, dict(a, x=32.5), second=dict(b, y=32.0))])
    imgs = model.sample_images(thetas, ('raw_model',))['raw_model']
    lp = model.log_posterior_batch(thetas)
    prior = model.log_priors_batch(thetas)
    for i, t in enumerate(thetas):
        want_ll, want = contract_evaluate(model, field, t)
        assert raw_error(imgs[i], want['raw_model'], '%s mixed %d' % (backend, i)) <= 1e-10
        assert abs(lp[i] - (want_ll + prior[i])) <= 1e-9 * abs(want_ll)
    # two general components, one with modes: the other runs the loop without them in the same launch
    model.close()
    model = make_model(fld, THREE, boxiness=FREE, backend=backend, max_walkers=8, second=dict(boxiness=0.4))
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


@pytest.mark.parametrize('order', [(0, 1), (1, 0)], ids=['modes-first', 'modes-last'])
def test_field_set_keeps_per_field_modes(order):
    """A 64x64 field with modes (fixed values: the same free parameters) and a 96x64 field with a boxiness alone,
    registered in either order, against each field's own context as tests/test_gpu_mixed_fields.py compares them:
    within 1e-12 of the largest value, bit-identical where the own context has the set's transform (the 96x64 field),
    and a field's values do not depend on the other field being in the batch.  Row-based calls of both go through the
    shared context (the rows of the field without modes are padded to the context's width)."""
    from psfmc_amd.models import FieldSet
    flds = [make_field(64, 64, seed=10), make_field(96, 64, seed=11)]
    kws = [dict(fourier={1: (0.2, 30.0), 3: (-0.15, 110.0)}, boxiness=0.6), dict(fourier=None, boxiness=-0.4)]
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


def test_joint_model_shared_amplitude_and_own_phases():
    from psfmc_amd import JointModel
    fa, fb = make_field(64, 64, seed=12), make_field(70, 66, seed=13)
    kw = dict(fourier=THREE, boxiness=FREE)
    joint = JointModel([make_model(fa, max_walkers=1, **kw), make_model(fb, max_walkers=1, **kw)],
                       per_field=['2_Sersic_f1_phase', '1_PointSource_xy', '2_Sersic_xy'], max_walkers=32)
    names = joint.param_names
    assert names.count('2_Sersic_f1_amp') == 1 and '2_Sersic_f1_phase_f1' in names
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
    own_names = sum(([n] * w for n, w in zip(own_a_model.param_names, own_a_model.param_lens)), [])
    bad[0, joint.field_columns(0)[own_names.index('2_Sersic_f1_amp')]] = 0.9
    assert joint.log_posterior_batch(bad)[0] == -np.inf                           # the shared amplitude: sum |a| >= 1
    joint.close()


def test_f32_storage_and_context_group():
    """storage='f32' within its documented 2e-6; a ContextGroup on one device equals the plain context."""
    fld = make_field(64, 64, seed=14)
    field = oracle_field(fld)
    kw, thetas = contract_sets(fld)[2]
    f32 = make_model(fld, storage='f32', **kw)
    ll = f32.log_likelihood_batch(thetas)
    lp32 = f32.log_posterior_batch(thetas)
    prior = f32.log_priors_batch(thetas)
    for i, t in enumerate(thetas):
        want_ll, _ = contract_evaluate(f32, field, t)
        assert abs(ll[i] - want_ll) <= 2e-6 * abs(want_ll) and abs(lp32[i] - want_ll - prior[i]) <= 2e-6 * abs(want_ll)
    f32.close()
    model = make_model(fld, **kw)
    grp = model.device_group([0], max_walkers=16)
    got = grp.logpost_theta(thetas)
    assert np.all(np.isfinite(got)) and np.array_equal(got, model.log_posterior_batch(thetas))
    grp.close()
    model.close()


def test_the_library_refuses_what_the_header_says():
    from psfmc_amd.engine import NativeError
    fld = make_field(64, 64, seed=15)
    model = make_model(fld, ONE, max_walkers=4)
    eng = model.engine
    zeros = [0.0] * 12
    with pytest.raises(NativeError, match='mode'):
        eng.set_fourier_layout([1 << 6], [-1] * 12, zeros)
    with pytest.raises(NativeError, match='column'):
        eng.set_fourier_layout([1], [model.num_params] + [-1] * 11, zeros)
    model.close()
    plain = make_model(fld, None, max_walkers=4)
    with pytest.raises(NativeError, match='aux layout'):
        plain.engine.set_fourier_layout([1], [-1] * 12, zeros)
    plain.close()
    integ = tgg.make_model(fld, boxiness=(ABSENT,), integrate=(True,), max_walkers=4)     # (a tilted sky: an aux layout)
    with pytest.raises(NativeError, match='integrated'):
        integ.engine.set_fourier_layout([1], [-1] * 12, zeros)
    integ.close()


def test_a_planted_lopsided_host_is_recovered():
    """sci = the contract's convolved image of a host with a_1 = 0.25 plus the helper's fixed-seed noise: the
    log-posterior at the planted vector exceeds the one with a_1 = 0, and a 200-iteration, 32-walker device chain
    started around a_1 = 0 ends (median of its last 50 iterations) nearer 0.25 than 0."""
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(64, 64, seed=16)
    noise = fld['sci'].astype(np.float64) - 0.05
    truth = dict(four=[0.25, 40.0], index=1.0, mag=16.5, reff=7.0, reff_b=5.0, x=32.3, y=30.8)
    planted = theta_of(fld, truth, lean=True)
    first = make_model(fld, ONE, max_walkers=1, lean=True)
    conv = contract_evaluate(first, oracle_field(fld), planted)[1]['convolved_model']
    first.close()
    model = make_model(dict(fld, sci=(conv + noise).astype(np.float32)), ONE, max_walkers=32, lean=True)
    a1 = model.param_names.index('2_Sersic_f1_amp')
    flat = planted.copy()
    flat[a1] = 0.0
    lp = model.log_posterior_batch(np.array([planted, flat]))
    print('log-posterior at the planted vector %.2f, with a_1 = 0 %.2f' % (lp[0], lp[1]))
    assert np.isfinite(lp[1]) and lp[0] > lp[1]
    rng = np.random.RandomState(4)
    p0 = flat + rng.normal(size=(32, len(flat))) * np.array([1e-3, 1e-2, 1e-2, 1.0, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2])
    s = DeviceEnsembleSampler(32, model, block=50)
    s.random_state = np.random.RandomState(5).get_state()
    list(s.sample(p0, iterations=200))
    med = float(np.median(s.chain[:, -50:, a1]))
    print('median a_1 of the last 50 iterations: %.3f' % med)
    assert abs(med - 0.25) < abs(med)
    model.close()
