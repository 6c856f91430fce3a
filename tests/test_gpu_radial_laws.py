"""The radial laws `Moffat` and `Ferrer` on the device, held to the numpy definition (`Sersic.radial_image`) composed
with the oracle's point source, convolution and likelihood: raw images per pixel on every forward-kernel family of both
back ends, neutral keywords against the plain law, batch independence and the support, the untouched default,
boxiness-only, Fourier and spiral models, the samplers, mixed models, posterior sums, field sets, joint fits, f32
storage, context groups, the library's refusals and a planted boxy bar.  Field and contract helpers are those of
tests/test_gpu_general_components.py."""
import numpy as np
import pytest

import test_gpu_fourier_modes as tgf
import test_gpu_general_components as tgg
import test_gpu_spiral_arms as tgs
from extra_contract import EDGE_MARGIN, ferrer_state, law_error
from test_gpu_general_components import RAW_BOUND, contract_evaluate, make_field, oracle_field, raw_error
from psfmc_amd import MultiComponentModel
from psfmc_amd.ModelComponents import Configuration, Ferrer, Moffat, PointSource, Sersic, Sky
from psfmc_amd.distributions import Normal, Uniform

pytestmark = pytest.mark.gpu


def U(lo, hi):
    return Uniform(loc=lo, scale=hi - lo)


def build(fld, comps, backend='fused', max_walkers=16, storage='f64', degrees=True, ps_free=True, slope=False,
          extent=None):
    """Sky + PointSource + `comps`: (class, {argument: a value, or 'free' for the test's prior -- wider than the
    support where the argument has one}) per component.  The arguments not named are free except `angle`.  extent:
    the image side the priors of positions and radii are scaled to (joint fits: shared priors are equal)."""
    ny, nx = fld['shape']
    c = np.array((nx / 2 + 0.5, ny / 2 + 0.5))
    big = 4.0 * (extent or max(ny, nx))
    turn = 360.0 if degrees else 2 * np.pi
    prior = {'xy': lambda: Uniform(loc=c - 0.5 * big, scale=big * np.ones(2)), 'mag': lambda: U(15.0, 25.0),
             'fwhm': lambda: U(0.5, big), 'fwhm_b': lambda: U(0.5, big), 'r_out': lambda: U(0.5, big),
             'r_out_b': lambda: U(0.5, big), 'reff': lambda: U(0.5, 40.0), 'reff_b': lambda: U(0.5, 40.0),
             'index': lambda: U(0.2, 8.0), 'alpha': lambda: U(-1.0, 7.0), 'beta': lambda: U(-4.0, 9.0),
             'angle': lambda: U(-turn, turn), 'boxiness': lambda: U(-1.5, 2.5)}
    own = {Moffat: ('xy', 'mag', 'fwhm', 'fwhm_b', 'beta'), Ferrer: ('xy', 'mag', 'r_out', 'r_out_b', 'alpha', 'beta'),
           Sersic: ('xy', 'mag', 'reff', 'reff_b', 'index')}
    out = [Configuration(fld['sci'], fld['ivm'], fld['psf'], fld['psf_ivm'], mag_zeropoint=fld['mag_zp']),
           Sky(adu=Normal(loc=0.05, scale=0.05), **({'slope': Normal(loc=(0, 0), scale=(1e-3, 1e-3))} if slope else {})),
           PointSource(xy=prior['xy']() if ps_free else (nx / 2 + 1.3, ny / 2 - 0.8), mag=U(16.0, 24.0))]
    for cls, args in comps:
        kw = {k: prior[k]() for k in own[cls]}
        kw['angle'] = 30.0 if degrees else 0.5
        for k, v in args.items():
            if k == 'fourier':
                kw[k] = {m: (U(-1.0, 1.0) if a == 'free' else a, U(-2 * turn, 2 * turn) if p == 'free' else p)
                         for m, (a, p) in v.items()}
            elif k == 'spiral':
                kw[k] = {s: (U(-2 * turn, 2 * turn) if s == 'winding' else U(-5.0, 200.0)) if x == 'free' else x
                         for s, x in v.items()}
            else:
                kw[k] = prior[k]() if isinstance(v, str) and v == 'free' else v
        out.append(cls(angle_degrees=degrees, **kw))
    return MultiComponentModel(out, backend=backend, max_walkers=max_walkers, storage=storage)


def vector(model, fld, values, adu=0.05, ps_mag=19.0):
    """One parameter vector from {parameter name: value}; the sky and the point source have defaults."""
    ny, nx = fld['shape']
    vals = {'0_Sky_adu': adu, '1_PointSource_mag': ps_mag, '1_PointSource_xy': (nx / 2 + 1.3, ny / 2 - 0.8),
            '0_Sky_slope': (0.02 / nx, -0.01 / ny)}                    # (the plane stays positive over the image)
    vals.update(values)
    vals = {k: v for k, v in vals.items() if k in model.param_names or k in values}
    out = []
    for name in model.param_names:
        out += list(np.ravel(vals.pop(name)))
    assert not vals, sorted(vals)
    return np.array(out, dtype=np.float64)


def column(model, name):
    names = sum(([n] * w for n, w in zip(model.param_names, model.param_lens)), [])
    return names.index(name)


def named(idx, kind, **kw):
    return {'%d_%s_%s' % (idx, kind, k): v for k, v in kw.items()}


TWO = {2: ('free', 'free'), 3: ('free', 25.0)}


def contract_sets(fld):
    """[(components, build keywords, [{name: value}])]: each law alone in radians, both with a free boxiness and two
    modes in degrees, a boxy Ferrer with a spiral beside a Moffat and a plain Sersic -- nine walkers (in four models:
    "alone" is taken at its word).  Moffat beta in {1.2, 2.5, 6}; Ferrer (alpha, beta) in {(0, 0), (0.5, 1.5), (2, 0),
    (4, -2)}; r_out smaller and larger than the image; an axis along the pixel grid through x + 0.5; a centre on a
    pixel corner; a centre on a pixel centre, with modes; centres outside the image."""
    ny, nx = fld['shape']
    cx, cy = nx // 2, ny // 2
    small, large = 0.31 * min(ny, nx), 3.0 * max(ny, nx)
    sets = [
        ([(Moffat, dict(angle='free'))], dict(degrees=False), [
            named(2, 'Moffat', angle=0.5, beta=1.2, fwhm=6.0, fwhm_b=4.0, mag=18.0, xy=(cx + 0.31, cy - 0.27)),
            named(2, 'Moffat', angle=-0.5 * np.pi, beta=6.0, fwhm=9.0, fwhm_b=3.0, mag=18.3, xy=(cx + 0.5, float(cy)))]),
        ([(Ferrer, dict(angle='free'))], dict(degrees=False), [
            # (held relative to Sigma_0 on every pixel: the point source is faint and the large component bright, so
            # that the other components' own rounding stays below 1e-12 of Sigma_0)
            dict(named(2, 'Ferrer', alpha=0.0, angle=0.4, beta=0.0, mag=18.0, r_out=small, r_out_b=0.6 * small,
                       xy=(cx + 0.37, cy - 0.21)), **{'1_PointSource_mag': 23.9}),
            dict(named(2, 'Ferrer', alpha=4.0, angle=1.1, beta=-2.0, mag=15.0, r_out=large, r_out_b=0.5 * large,
                       xy=(-3.6, cy + 0.4)), **{'1_PointSource_mag': 23.9})]),
        ([(Moffat, dict(angle='free', boxiness='free', fourier=TWO)),
          (Ferrer, dict(angle='free', boxiness='free', fourier=TWO))], dict(degrees=True, slope=True), [
            dict(named(2, 'Moffat', angle=30.0, beta=2.5, boxiness=-1.0, f2_amp=0.2, f2_phase=30.0, f3_amp=0.3, fwhm=5.0,
                       fwhm_b=4.5, mag=18.0, xy=(cx + 0.5, cy - 0.5)),                              # a pixel corner
                 **named(3, 'Ferrer', alpha=0.5, angle=75.0, beta=1.5, boxiness=0.7, f2_amp=-0.2, f2_phase=100.0,
                         f3_amp=0.1, mag=18.2, r_out=small, r_out_b=0.45 * small, xy=(cx - 2.4, cy + 1.7))),
            dict(named(2, 'Moffat', angle=-20.0, beta=6.0, boxiness=2.0, f2_amp=0.1, f2_phase=-50.0, f3_amp=-0.2,
                       fwhm=8.0, fwhm_b=3.0, mag=18.6, xy=(float(cx - 3), float(cy + 2))),           # a pixel centre
                 **named(3, 'Ferrer', alpha=2.0, angle=-90.0, beta=0.0, boxiness=0.0, f2_amp=0.3, f2_phase=200.0,
                         f3_amp=-0.3, mag=18.4, r_out=1.3 * small, r_out_b=0.9 * small,
                         xy=(float(cx + 2), float(cy - 1)))),                                        # a pixel centre
            dict(named(2, 'Moffat', angle=60.0, beta=1.2, boxiness=1.3, f2_amp=-0.2, f2_phase=75.0, f3_amp=0.1,
                       fwhm=20.0, fwhm_b=8.0, mag=18.9, xy=(nx + 5.0, ny + 2.5)),                   # outside
                 **named(3, 'Ferrer', alpha=4.0, angle=10.0, beta=-2.0, boxiness=-0.5, f2_amp=0.1, f2_phase=10.0,
                         f3_amp=0.2, mag=18.7, r_out=large, r_out_b=0.7 * large, xy=(cx + 0.25, cy + 0.4)))]),
        ([(Ferrer, dict(angle='free', boxiness='free',
                        spiral=dict(r_in='free', r_out='free', winding='free', inclination=35.0, sky_angle=20.0))),
          (Moffat, dict(angle='free')), (Sersic, dict(angle='free'))], dict(degrees=True), [
            dict(named(2, 'Ferrer', alpha=2.0, angle=30.0, beta=0.0, boxiness=0.8, mag=18.0, r_out=small, r_out_b=0.35 * small,
                       spiral_r_in=2.0, spiral_r_out=10.0, spiral_wind=150.0, xy=(cx - 1.4, cy + 0.7)),
                 **dict(named(3, 'Moffat', angle=110.0, beta=2.5, fwhm=3.0, fwhm_b=1.5, mag=19.0, xy=(cx + 0.25, cy + 0.4)),
                        **named(4, 'Sersic', angle=-20.0, index=1.0, mag=18.5, reff=8.0, reff_b=3.0, xy=(cx + 3.2, cy - 1.1)))),
            dict(named(2, 'Ferrer', alpha=0.5, angle=-40.0, beta=1.5, boxiness=-0.4, mag=18.3, r_out=1.2 * small,
                       r_out_b=0.5 * small, spiral_r_in=0.0, spiral_r_out=6.0, spiral_wind=-200.0, xy=(cx + 0.5, float(cy))),
                 **dict(named(3, 'Moffat', angle=0.0, beta=1.2, fwhm=5.0, fwhm_b=5.0, mag=19.3, xy=(-2.5, -1.5)),
                        **named(4, 'Sersic', angle=45.0, index=4.0, mag=18.8, reff=3.0, reff_b=1.5, xy=(cx - 4.3, cy + 2.6))))]),
    ]
    return sets


@pytest.mark.parametrize('backend,shape', [('fused', s) for s in tgg.SHAPES] + [('hipfft', (64, 64)), ('hipfft', (70, 66))],
                         ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_device_against_the_contract(backend, shape):
    """Raw image per pixel at RAW_BOUND (MEASURED worst per shape: DESIGN.md section 18) -- a model with a Ferrer alone
    relative to Sigma_0 on every pixel, the others by `law_error` -- the five images to 1e-12 of the image maximum, the
    log-posterior through raw vectors and the log-likelihood through the host path's rows against the contract
    (1e-9)."""
    fld = make_field(*shape, seed=1)
    field = oracle_field(fld)
    worst = 0.0
    for n_set, (comps, kw, cases) in enumerate(contract_sets(fld)):
        model = build(fld, comps, backend=backend, **kw)
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
            if n_set == 1:
                assert np.all(np.isfinite(imgs['raw_model'][i]))
                err = float(np.max(np.abs(imgs['raw_model'][i] - want['raw_model'])) / sigma0)
                print('%s: raw model max error relative to Sigma_0 %.2e' % (tag, err))
            else:
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


def _moffat_cases(fld, model, idx=2):
    ny, nx = fld['shape']
    cx, cy = nx // 2, ny // 2
    rows = [dict(angle=30.0, beta=1.2, fwhm=6.0, fwhm_b=4.0, mag=18.0, xy=(cx + 0.31, cy - 0.27)),
            dict(angle=75.0, beta=2.5, fwhm=5.0, fwhm_b=4.5, mag=18.3, xy=(cx - 2.4, cy + 1.7)),
            dict(angle=-90.0, beta=6.0, fwhm=4.0, fwhm_b=3.0, mag=18.6, xy=(cx + 0.5, float(cy))),
            dict(angle=45.0, beta=3.0, fwhm=7.0, fwhm_b=6.0, mag=18.9, xy=(cx + 0.5, cy - 0.5)),
            dict(angle=10.0, beta=1.5, fwhm=12.0, fwhm_b=9.0, mag=19.2, xy=(-3.6, cy + 0.4))]
    return np.array([vector(model, fld, named(idx, 'Moffat', **r), adu=0.05 + 0.002 * i) for i, r in enumerate(rows)])


def test_neutral_keywords_against_the_plain_moffat():
    """Moffat(boxiness=0.0, zero-amplitude modes, zero winding) against the plain Moffat: log-posteriors agree to
    RAW_BOUND carried through the likelihood (the bound of the zero-winding test of tests/test_gpu_spiral_arms.py);
    the expected difference is a few rounding errors of the longer route."""
    fld = make_field(64, 64, seed=2)
    neutral = build(fld, [(Moffat, dict(angle='free', boxiness=0.0, fourier={1: (0.0, 0.0), 3: (0.0, 40.0)},
                                        spiral=dict(r_in=2.0, r_out=9.0, winding=0.0)))])
    plain = build(fld, [(Moffat, dict(angle='free'))])
    assert neutral.param_names == plain.param_names and neutral.sersic_radial_kinds == [1]
    assert neutral.sersic_spiral_flags == [True] and plain.sersic_spiral_flags == [False]
    thetas = _moffat_cases(fld, plain)
    a, b = neutral.log_posterior_batch(thetas), plain.log_posterior_batch(thetas)
    imgs = plain.sample_images(thetas, ('convolved_model', 'composite_ivm'))
    sci = fld['sci'].astype(np.float64)
    for i in range(len(thetas)):
        m, w = imgs['convolved_model'][i], imgs['composite_ivm'][i]
        r = sci - m
        bound = RAW_BOUND * 0.5 * float(np.sum(2 * np.abs(r) * np.abs(m) * w + 2 * r * r * w + 2))
        print('case %d: |difference| %.3e, bound %.3e' % (i, abs(a[i] - b[i]), bound))
        assert np.isfinite(b[i]) and abs(a[i] - b[i]) <= bound, (i, a[i], b[i])
    neutral.close()
    plain.close()


BOTH = [(Moffat, dict(angle='free', boxiness='free')), (Ferrer, dict(angle='free', boxiness='free'))]


def _both_start(fld, model, n_w, seed, scale=1e-3):
    ny, nx = fld['shape']
    base = vector(model, fld, dict(
        named(2, 'Moffat', angle=30.0, beta=2.5, boxiness=0.3, fwhm=5.0, fwhm_b=3.5, mag=18.5, xy=(nx / 2 - 2.4, ny / 2 + 1.7)),
        **named(3, 'Ferrer', alpha=1.5, angle=70.0, beta=0.5, boxiness=0.6, mag=18.0, r_out=18.3, r_out_b=7.1,
                xy=(nx / 2 + 0.31, ny / 2 - 0.27))))
    rng = np.random.RandomState(seed)
    return base + rng.normal(size=(n_w, len(base))) * scale


def test_batch_independence_and_the_support_of_the_laws():
    """A walker's log-posterior bits are the same alone, in a batch of 64 and in permuted order; a Moffat beta of 1 and
    of NaN, a Ferrer alpha < 0 and a Ferrer beta of 2 are -inf from raw vectors on the device and on the host, leave
    the other walkers' bits unchanged, and are NaN through a row-based call (no writable flags there)."""
    fld = make_field(64, 64, seed=4)
    model = build(fld, BOTH, max_walkers=64)
    thetas = _both_start(fld, model, 64, 5)
    full = model.log_posterior_batch(thetas)
    assert np.all(np.isfinite(full))
    for i in (0, 7, 63):
        assert model.log_posterior_batch(thetas[i:i + 1])[0] == full[i]
    perm = np.random.RandomState(6).permutation(64)
    assert np.array_equal(model.log_posterior_batch(thetas[perm]), full[perm])
    bad = [('2_Moffat_beta', 1.0), ('2_Moffat_beta', np.nan), ('3_Ferrer_alpha', -0.1), ('3_Ferrer_beta', 2.0),
           ('2_Moffat_beta', 0.5), ('2_Moffat_beta', np.inf), ('3_Ferrer_beta', 3.0), ('3_Ferrer_beta', np.nan),
           ('3_Ferrer_alpha', np.nan)]
    where = [3 + 5 * k for k in range(len(bad))]
    mixed = thetas.copy()
    for k, (name, val) in zip(where, bad):
        mixed[k, column(model, name)] = val
    got = model.log_posterior_batch(mixed)
    keep = np.ones(64, dtype=bool)
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


def _spiral_reference():
    """(log-posteriors, 20-iteration device chain, its log-probabilities) of a model with a spiral."""
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(64, 64, seed=7)
    model = tgs.make_model(fld, tgs.LEAN_SPIRAL, max_walkers=32, lean=True)
    p0 = tgs._lean_start(fld, 32, 2)
    lp = model.log_posterior_batch(p0)
    s = DeviceEnsembleSampler(32, model, block=5)
    s.random_state = np.random.RandomState(3).get_state()
    list(s.sample(p0, iterations=20))
    out = lp, s.chain.copy(), s.lnprobability.copy()
    model.close()
    return out


def test_models_without_the_laws_are_untouched_by_law_contexts():
    """Plain, boxiness-only, Fourier and spiral models: bit-identical log-posteriors and 20-iteration device chains
    before and after contexts with laws lived and died in the process."""
    refs = lambda: (tgg._plain_reference()[2], tgf._boxiness_reference(), tgs._fourier_reference(), _spiral_reference())
    before = refs()
    fld = make_field(64, 64, seed=3)
    alive = []
    for comps, kw, cases in contract_sets(fld):
        alive.append(build(fld, comps, **kw))
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


# Sky + PS (a fixed position) + a boxy Ferrer + a Moffat with 11 free parameters: adu, the point source's mag, the
# Ferrer's alpha, boxiness, mag, r_out, x, y, the Moffat's beta, fwhm, mag
LEAN = [(Ferrer, dict(boxiness='free', beta=0.5, r_out_b=6.0)), (Moffat, dict(xy=(33.6, 31.2), fwhm_b=2.5))]


def _lean_start(fld, model, n_w, seed):
    base = vector(model, fld, dict(named(2, 'Ferrer', alpha=1.5, boxiness=0.6, mag=18.0, r_out=18.3, xy=(32.3, 30.8)),
                                   **named(3, 'Moffat', beta=2.5, fwhm=4.0, mag=19.0)), ps_mag=19.0)
    return base + np.random.RandomState(seed).normal(size=(n_w, len(base))) * 1e-2


@pytest.mark.parametrize('n_w', [22, 64])
def test_device_sampler_equals_the_host_sampler(n_w):
    """The device-resident chain equals the host loop's fed the device's own log-posteriors, bit for bit (22 walkers:
    the whole-iteration route of small ensembles; 64: half-steps)."""
    from psfmc_amd.sampler import EnsembleSampler, DeviceEnsembleSampler
    fld = make_field(64, 64, seed=7)
    model = build(fld, LEAN, max_walkers=n_w, ps_free=False)
    assert model.num_params == 11
    p0 = _lean_start(fld, model, n_w, 2)
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
    contract's (tests/test_gpu_spiral_arms.py compares them so)."""
    from psfmc_amd.sampler import TemperedEnsembleSampler, DeviceTemperedSampler, default_betas
    fld = make_field(64, 64, seed=8)
    model = build(fld, LEAN, max_walkers=4 * 24, ps_free=False)
    betas = default_betas(4, 50.0)
    p0 = _lean_start(fld, model, 4 * 24, 3).reshape(4, 24, -1)
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
    """A plain Sersic (the default rasteriser) beside a Moffat and a Ferrer (RAW_BOUND by `law_error`); a Moffat beside
    a pixel-integrated Sersic: the integrated kernels write the extra image, the general one adds (1e-10 per pixel, the
    integrated profile's own bound)."""
    fld = make_field(64, 64, seed=6)
    field = oracle_field(fld)
    sersic = named(2, 'Sersic', angle=100.0, index=3.0, mag=18.5, reff=4.0, reff_b=2.0, xy=(29.5, 32.5))
    moffat = named(3, 'Moffat', angle=30.0, beta=2.5, fwhm=5.0, fwhm_b=3.5, mag=18.8, xy=(32.3, 30.8))
    model = build(fld, [(Sersic, dict(angle='free')), (Moffat, dict(angle='free')), (Ferrer, dict(angle='free'))],
                  backend=backend, max_walkers=8)
    assert model.sersic_general_flags == [False, True, True] and model.sersic_radial_kinds == [0, 1, 2]
    thetas = np.array([vector(model, fld, dict(sersic, **dict(moffat, **named(
        4, 'Ferrer', alpha=a, angle=70.0, beta=b, mag=18.0, r_out=18.3, r_out_b=7.1, xy=(33.31, 31.73)))))
        for a, b in ((1.5, 0.5), (0.0, 1.0))])
    want = []
    for t in thetas:
        want.append(contract_evaluate(model, field, t) + ferrer_state(model))
        assert want[-1][3] >= EDGE_MARGIN
    imgs = model.sample_images(thetas, ('raw_model',))['raw_model']
    lp = model.log_posterior_batch(thetas)
    prior = model.log_priors_batch(thetas)
    for i, (want_ll, images, sigma0, _) in enumerate(want):
        assert law_error(imgs[i], images['raw_model'], sigma0, '%s three laws %d' % (backend, i)) <= RAW_BOUND
        assert abs(lp[i] - (want_ll + prior[i])) <= 1e-9 * abs(want_ll)
    model.close()
    model = build(fld, [(Sersic, dict(angle='free', integrate=True)), (Moffat, dict(angle='free'))], backend=backend,
                  max_walkers=8)
    assert model.sersic_integrate == [True, False]
    thetas = np.array([vector(model, fld, dict(sersic, **moffat)),
                       vector(model, fld, dict(named(2, 'Sersic', angle=100.0, index=1.0, mag=18.5, reff=4.0, reff_b=2.0,
                                                     xy=(29.0, 32.0)), **moffat))])
    imgs = model.sample_images(thetas, ('raw_model',))['raw_model']
    lp = model.log_posterior_batch(thetas)
    prior = model.log_priors_batch(thetas)
    for i, t in enumerate(thetas):
        want_ll, images = contract_evaluate(model, field, t)
        assert raw_error(imgs[i], images['raw_model'], '%s beside integrate %d' % (backend, i)) <= 1e-10
        assert abs(lp[i] - (want_ll + prior[i])) <= 1e-9 * abs(want_ll)
    model.close()


def test_accumulated_images_against_the_contract():
    fld = make_field(70, 66, seed=9)
    comps, kw, cases = contract_sets(fld)[2]
    model = build(fld, comps, **kw)
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


@pytest.mark.parametrize('order', [(0, 1), (1, 0)], ids=['laws-first', 'laws-last'])
def test_field_set_keeps_the_laws_per_field(order):
    """A 64x64 field with a Moffat and a boxy Ferrer and a 96x64 field with a boxy Sersic and a Sersic with a spiral,
    registered in either order, against each field's own context: within 1e-12 of the largest value, bit-identical
    where the own context has the set's transform."""
    from psfmc_amd.models import FieldSet
    flds = [make_field(64, 64, seed=10), make_field(96, 64, seed=11)]
    specs = [BOTH, [(Sersic, dict(angle='free', boxiness='free')),           # (the same number of free parameters)
                    (Sersic, dict(angle='free', spiral=dict(r_in=2.0, r_out='free', winding='free')))]]
    flds, specs = [flds[i] for i in order], [specs[i] for i in order]
    fs = FieldSet([build(f, s, max_walkers=1) for f, s in zip(flds, specs)], max_walkers=32)
    own = [build(f, s, max_walkers=16) for f, s in zip(flds, specs)]
    thetas = []
    for f, m in zip(flds, own):
        if any(m.sersic_radial_kinds):
            thetas.append(_both_start(f, m, 4, 12, scale=0.05))
        else:
            ny, nx = f['shape']
            thetas.append(np.array([vector(m, f, dict(
                named(2, 'Sersic', angle=30.0 + 10 * i, boxiness=-0.4 + 0.3 * i, index=1.0 + i, mag=18.0, reff=6.0,
                      reff_b=4.0, xy=(nx / 2 + 0.31 + i, ny / 2 - 0.27)),
                **named(3, 'Sersic', angle=75.0, index=1.0, mag=18.5 + 0.1 * i, reff=8.0, reff_b=3.0, spiral_r_out=9.0 + i,
                        spiral_wind=200.0 - 90.0 * i, xy=(nx / 2 - 2.4, ny / 2 + 1.7 - i)))) for i in range(4)]))
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


def test_joint_model_shared_beta_and_own_r_out():
    from psfmc_amd import JointModel
    fa, fb = make_field(64, 64, seed=12), make_field(70, 66, seed=13)
    joint = JointModel([build(fa, BOTH, max_walkers=1, extent=70), build(fb, BOTH, max_walkers=1, extent=70)],
                       per_field=['3_Ferrer_r_out', '1_PointSource_xy', '2_Moffat_xy', '3_Ferrer_xy'], max_walkers=32)
    names = joint.param_names
    assert names.count('3_Ferrer_beta') == 1 and names.count('2_Moffat_beta') == 1 and '3_Ferrer_r_out_f1' in names
    own_a, own_b = build(fa, BOTH, max_walkers=1, extent=70), build(fb, BOTH, max_walkers=1, extent=70)
    base_a, base_b = _both_start(fa, own_a, 3, 14, scale=0.02), _both_start(fb, own_b, 3, 14, scale=0.02)
    base_b[:, column(own_b, '3_Ferrer_r_out')] += 3.0
    thetas = np.zeros((3, joint.num_params))
    thetas[:, joint.field_columns(1)] = base_b
    thetas[:, joint.field_columns(0)] = base_a
    got = joint.log_posterior_batch(thetas)
    prior = joint.log_priors_batch(thetas)
    field_a, field_b = oracle_field(fa), oracle_field(fb)
    for i, t in enumerate(thetas):
        ta, tb = joint.field_theta(t, 0)[0], joint.field_theta(t, 1)[0]
        assert ta[column(own_a, '3_Ferrer_beta')] == tb[column(own_b, '3_Ferrer_beta')]
        assert abs(tb[column(own_b, '3_Ferrer_r_out')] - ta[column(own_a, '3_Ferrer_r_out')] - 3.0) < 0.5
        want = (contract_evaluate(own_a, field_a, ta)[0] + contract_evaluate(own_b, field_b, tb)[0]) + prior[i]
        assert np.isfinite(want) and abs(got[i] - want) <= 1e-9 * abs(want), (i, got[i], want)
    assert joint.log_posterior_batch(thetas[1:2])[0] == got[1]
    bad = thetas[:1].copy()
    bad[0, joint.field_columns(0)[column(own_a, '3_Ferrer_beta')]] = 2.5
    assert joint.log_posterior_batch(bad)[0] == -np.inf                            # the shared beta: outside the support
    joint.close()
    own_a.close()
    own_b.close()


def test_f32_storage_and_context_group():
    """storage='f32' within its documented 2e-6; a ContextGroup on one device equals the plain context through raw
    vectors and refuses derived rows."""
    fld = make_field(64, 64, seed=14)
    field = oracle_field(fld)
    f32 = build(fld, BOTH, storage='f32')
    thetas = _both_start(fld, f32, 3, 15, scale=0.02)
    ll = f32.log_likelihood_batch(thetas)
    lp32 = f32.log_posterior_batch(thetas)
    prior = f32.log_priors_batch(thetas)
    for i, t in enumerate(thetas):
        want_ll, _ = contract_evaluate(f32, field, t)
        assert abs(ll[i] - want_ll) <= 2e-6 * abs(want_ll) and abs(lp32[i] - want_ll - prior[i]) <= 2e-6 * abs(want_ll)
    f32.close()
    model = build(fld, BOTH)
    grp = model.device_group([0], max_walkers=16)
    got = grp.logpost_theta(thetas)
    assert np.all(np.isfinite(got)) and np.array_equal(got, model.log_posterior_batch(thetas))
    with pytest.raises(NotImplementedError):
        grp.loglike(model.derived_rows(thetas), aux=model.aux_rows(thetas))
    grp.close()
    model.close()


def test_the_library_refuses_what_the_header_says():
    from psfmc_amd.engine import NativeError
    fld = make_field(64, 64, seed=15)
    model = build(fld, [(Moffat, {}), (Sersic, dict(boxiness=0.3)), (Sersic, {})], max_walkers=4)
    eng = model.engine
    with pytest.raises(NativeError, match='kind'):
        eng.set_radial_layout([3, 0, 0], [-1] * 6, [2.0, 0.0] * 3)
    with pytest.raises(NativeError, match='kind'):
        eng.set_radial_layout([-1, 0, 0], [-1] * 6, [2.0, 0.0] * 3)
    with pytest.raises(NativeError, match='general'):
        eng.set_radial_layout([1, 0, 2], [-1] * 6, [2.0, 0.0] * 3)            # the third slot is a plain Sersic
    with pytest.raises(NativeError, match='n_sersic'):
        eng.set_radial_layout([1, 0], [-1] * 4, [2.0, 0.0] * 2)
    with pytest.raises(NativeError, match='column'):
        eng.set_radial_layout([1, 0, 0], [model.num_params] + [-1] * 5, [2.0, 0.0] * 3)
    eng.set_radial_layout([1, 2, 0], [-1] * 6, [2.0, 0.0, 1.0, 0.5, 0.0, 0.0])      # a general slot may take a law
    eng.set_radial_layout([0, 0, 0], [-1] * 6, [0.0] * 6)                          # all-zero kinds remove the laws
    model.close()
    plain = build(fld, [(Sersic, {})], max_walkers=4)
    with pytest.raises(NativeError, match='aux layout'):
        plain.engine.set_radial_layout([1], [-1, -1], [2.0, 0.0])
    plain.close()
    integ = build(fld, [(Sersic, dict(integrate=True))], max_walkers=4, slope=True)          # (a tilted sky: an aux layout)
    with pytest.raises(NativeError, match='integrated'):
        integ.engine.set_radial_layout([2], [-1, -1], [1.0, 0.5])
    integ.close()


def test_removing_the_laws_gives_the_sersic_slot_back():
    """All-zero kinds: the slot is the boxy Sersic of index 1 that its layout describes, bit for bit."""
    fld = make_field(64, 64, seed=17)
    law = build(fld, [(Moffat, dict(boxiness='free'))], max_walkers=4)
    ser = build(fld, [(Sersic, dict(boxiness='free', index=1.0))], max_walkers=4)
    t = vector(law, fld, named(2, 'Moffat', beta=2.5, boxiness=0.3, fwhm=5.0, fwhm_b=3.5, mag=18.5, xy=(32.3, 30.8)))
    ts_ = vector(ser, fld, named(2, 'Sersic', boxiness=0.3, reff=5.0, reff_b=3.5, mag=18.5, xy=(32.3, 30.8)))[None]
    want = ser.log_posterior_batch(ts_)[0]
    first = law.log_posterior_batch(t[None])[0]
    law.engine.set_radial_layout([0], [-1, -1], [0.0, 0.0])
    again = law.log_posterior_batch(t[None])[0]
    print('Moffat %.6f, the slot without its law %.6f, the boxy Sersic %.6f' % (first, again, want))
    assert np.isfinite(first) and first != want
    # (the Moffat's beta column has a prior of its own: the posteriors differ by it, the likelihoods do not)
    prior_law, prior_ser = law.log_priors_batch(t[None])[0], ser.log_priors_batch(ts_)[0]
    assert abs((again - prior_law) - (want - prior_ser)) <= 1e-12 * abs(want)
    law.close()
    ser.close()


def test_a_planted_boxy_bar_is_recovered():
    """sci = the contract's convolved image of a boxy Ferrer bar (r_out 20, r_out_b 6, the size of the planted host of
    tests/test_gpu_spiral_arms.py) plus the helper's fixed-seed noise: the log-posterior at the planted vector
    exceeds the one with r_out off by 3 pixels, and the truth of r_out lies inside the central 95 % of the last 100
    iterations of a 200-iteration, 32-walker device chain started in a ball about r_out = 19."""
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(64, 64, seed=16)
    noise = fld['sci'].astype(np.float64) - 0.05
    comps = [(Ferrer, dict(boxiness='free', beta=0.5, angle=30.0))]
    truth = named(2, 'Ferrer', alpha=2.0, boxiness=0.6, mag=19.5, r_out=20.0, r_out_b=6.0, xy=(32.3, 30.8))
    first = build(fld, comps, max_walkers=1, ps_free=False)
    planted = vector(first, fld, truth)
    conv = contract_evaluate(first, oracle_field(fld), planted)[1]['convolved_model']
    first.close()
    model = build(dict(fld, sci=(conv + noise).astype(np.float32)), comps, max_walkers=32, ps_free=False)
    rout = column(model, '2_Ferrer_r_out')
    off = planted.copy()
    off[rout] = 23.0
    lp = model.log_posterior_batch(np.array([planted, off]))
    print('log-posterior at the planted vector %.2f, with r_out = 23: %.2f' % (lp[0], lp[1]))
    assert np.isfinite(lp[1]) and lp[0] > lp[1]
    rng = np.random.RandomState(4)
    start = planted.copy()
    start[rout] = 19.0
    scale = np.full(len(start), 1e-2)
    scale[0], scale[rout] = 1e-3, 0.3
    p0 = start + rng.normal(size=(32, len(start))) * scale
    s = DeviceEnsembleSampler(32, model, block=50)
    s.random_state = np.random.RandomState(5).get_state()
    list(s.sample(p0, iterations=200))
    lo, med, hi = np.percentile(s.chain[:, -100:, rout], [2.5, 50.0, 97.5])
    print('r_out of the last 100 iterations: 2.5 %% %.3f, median %.3f, 97.5 %% %.3f' % (lo, med, hi))
    assert lo <= 20.0 <= hi
    model.close()
