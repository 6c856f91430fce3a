"""Prior families 5-17 (include/psfmc_hip.h psfmc_set_priors) evaluated on the device: every family
against scipy.stats on a grid that covers the bulk, both tails, the support's edges and one ulp on either
side, points outside the support and NaN; a model of several such priors through every device path
(batched posterior, device sampler, FieldSet, evaluate_device, a device group); and the refusals of the
C ABI."""
import ctypes

import numpy as np
import pytest
import scipy.stats as st

import helpers

pytestmark = pytest.mark.gpu
EINVAL = -1                 # include/psfmc_hip.h PSFMC_EINVAL

# (family code, scipy name, parameter sets: the scipy arguments in order -- shapes, loc, scale)
FAMILIES = [
    (5, 'truncnorm', [(-1.0, 2.0, 20.0, 0.5), (-30.0, -25.0, 0.0, 1.0), (25.0, 28.0, 1.5, 2.0),
                      (-np.inf, 0.5, 0.0, 3.0), (0.5, np.inf, -2.0, 1.0)]),
    (6, 'lognorm', [(0.5, 0.0, 3.0), (1.7, -2.0, 0.25), (0.05, 1.0, 1.0)]),
    (7, 'halfnorm', [(0.0, 1.0), (-3.0, 0.02), (5.0, 7.5)]),
    (8, 'expon', [(0.0, 1.0), (2.0, 0.3), (-1.0, 40.0)]),
    (9, 'laplace', [(0.0, 1.0), (20.0, 0.1), (-4.0, 3.0)]),
    (10, 'cauchy', [(0.0, 1.0), (20.0, 0.3), (-5.0, 8.0)]),
    (11, 'halfcauchy', [(0.0, 1.0), (0.5, 0.05), (-2.0, 4.0)]),
    (12, 'logistic', [(0.0, 1.0), (22.0, 0.4), (-3.0, 6.0)]),
    (13, 't', [(1.0, 0.0, 1.0), (3.5, 20.0, 0.5), (0.4, -1.0, 2.0), (250.0, 0.0, 1.0), (5e4, 2.0, 3.0)]),
    (14, 'beta', [(1.0, 3.0, 0.0, 1.0), (0.5, 0.5, -1.0, 2.0), (2.5, 0.7, 0.3, 6.0), (4.0, 9.0, 0.0, 1.0)]),
    (15, 'reciprocal', [(0.1, 10.0, 0.0, 1.0), (1.0, 2.0, -1.0, 3.0), (1e-3, 1e3, 0.5, 0.1)]),
    (16, 'weibull_max', [(2.0, 0.0, 1.0), (0.5, 1.0, 2.0), (1.0, -3.0, 0.5), (7.0, 10.0, 4.0)]),
    (17, 'invgamma', [(2.0, 0.0, 1.0), (0.5, -1.0, 3.0), (12.0, 2.0, 0.2)]),
]


def _ulps(x):
    """x and its neighbours one ulp below and above"""
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


def prior_grid(rv):
    """Points x for a frozen continuous distribution: in units y = (x - loc) / scale the bulk of the support,
    both tails out to |y| = 30 where the support reaches that far, the support's finite edges and one ulp
    on either side of them (in x), points beyond the support, +-inf and NaN."""
    shapes, loc, scale = rv.dist._parse_args(*rv.args, **rv.kwds)
    lo, hi = rv.dist._get_support(*shapes)
    y = [np.linspace(-3.0, 3.0, 61), np.array([-30.0, -20.0, -10.0, -5.0, 5.0, 10.0, 20.0, 30.0]),
         np.geomspace(1e-12, 0.999, 40), 1.0 - np.geomspace(1e-12, 0.5, 20)]
    for e in (lo, hi):
        if np.isfinite(e):
            y.append(e + np.array([-1.0, -1e-3, 1e-9, 0.0, 1e-3]))
            if np.isfinite(lo) and np.isfinite(hi):
                y.append(lo + (hi - lo) * np.linspace(0.0, 1.0, 41))
    x = loc + scale * np.concatenate(y)
    edges = [loc + scale * e for e in (lo, hi) if np.isfinite(e)]
    edges.append(loc)
    x = np.concatenate([x, _ulps(edges), [np.inf, -np.inf, np.nan]])
    return x


@pytest.fixture(scope='module')
def one_column():
    """A model whose only free parameter is a sky level: its prior table is swapped per test."""
    from psfmc_amd import MultiComponentModel
    from psfmc_amd.ModelComponents import Configuration, Sersic, Sky
    from psfmc_amd.distributions import Normal
    case = helpers.load_case('synth128x2')
    cfg = Configuration(case['sci'], case['ivm'], case['psfs'][0], case['psf_ivms'][0], mag_zeropoint=25.0)
    model = MultiComponentModel([cfg, Sky(adu=Normal(loc=0.0, scale=0.02)),
                                 Sersic(xy=(64.2, 63.1), mag=20.0, reff=8.0, reff_b=5.0, index=2.0, angle=0.3)],
                                max_walkers=512)
    model.engine
    yield model
    model.close()


def _check_against_scipy(got, skip, want, abs_bound=None):
    assert np.array_equal(skip, ~np.isfinite(want))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isposinf(got), np.isposinf(want))
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    if abs_bound is not None:
        assert err.max() <= abs_bound, err.max()
    else:
        rel = err / np.maximum(1.0, np.abs(want[fin]))
        assert rel.max() <= 1e-13, (rel.max(), got[fin][np.argmax(rel)], want[fin][np.argmax(rel)])


@pytest.mark.parametrize('code,name,sets', FAMILIES, ids=[f[1] for f in FAMILIES])
def test_family_matches_scipy(one_column, code, name, sets):
    eng = one_column.engine
    for p in sets:
        rv = getattr(st, name)(*p[:-2], loc=p[-2], scale=p[-1])
        x = prior_grid(rv)
        eng.set_priors([code], [p])
        _, got, skip = eng.debug_theta_rows(x[:, None])
        with np.errstate(all='ignore'):
            want = rv.logpdf(x)
        _check_against_scipy(got, skip, want, 1e-10 if name == 't' and p[0] > 100 else None)


def test_loguniform_and_edges_named_in_the_header(one_column):
    """loguniform is reciprocal; a few edge values spelt out."""
    eng = one_column.engine
    cases = [(8, (0.0, 1.0), [0.0], [0.0]),                                 # expon at 0
             (6, (1.0, 0.0, 1.0), [0.0], [-np.inf]),                        # lognorm at 0
             (14, (1.0, 3.0, 0.0, 1.0), [0.0, 1.0], [np.log(3.0), -np.inf]),
             (14, (0.5, 2.0, 0.0, 1.0), [0.0], [np.inf]),
             (16, (2.0, 0.0, 1.0), [0.0], [-np.inf]),
             (5, (-1.0, 2.0, 0.0, 1.0), [-1.0, 2.0], list(st.truncnorm(-1.0, 2.0).logpdf([-1.0, 2.0]))),
             (15, (0.5, 8.0, 0.0, 1.0), [0.5, 3.0], list(st.loguniform(0.5, 8.0).logpdf([0.5, 3.0])))]
    for code, p, x, want in cases:
        eng.set_priors([code], [p])
        _, got, _ = eng.debug_theta_rows(np.array(x)[:, None])
        assert np.allclose(got, want, rtol=1e-14, atol=0) or np.array_equal(got, want), (code, p, got, want)


def test_set_priors_refusals_keep_the_previous_table(one_column):
    """Each bad input returns PSFMC_EINVAL and leaves the table in force."""
    from psfmc_amd import engine
    eng = one_column.engine
    lib = engine.load_library()
    eng.set_priors([12], [(0.5, 2.0)])
    x = np.array([[-1.0], [0.3], [4.0]])
    before = eng.debug_theta_rows(x)[1]
    assert np.allclose(before, st.logistic(0.5, 2.0).logpdf(x[:, 0]), rtol=1e-14)
    ip = ctypes.POINTER(ctypes.c_int)

    def call(n, fam, params, field=0):
        fam = np.ascontiguousarray(fam, dtype=np.int32)
        tab = np.ascontiguousarray(np.reshape(params, (-1, 4)), dtype=np.float64)
        return lib.psfmc_set_priors(eng._ctx, field, n, fam.ctypes.data_as(ip), engine._dp(tab))
    bad = [(1, [18], [0, 1, 0, 0]), (1, [-1], [0, 1, 0, 0]), (1, [7], [0, 0, 0, 0]),
           (1, [7], [0, -1, 0, 0]), (1, [5], [2, 1, 0, 1]), (1, [15], [1, 1, 0, 1]), (1, [15], [-1, 1, 0, 1]),
           (1, [6], [0, 0, 1, 0]), (1, [14], [1, -2, 0, 1]), (1, [13], [np.inf, 0, 1, 0]),
           (1, [17], [np.nan, 0, 1, 0]), (1, [8], [np.nan, 1, 0, 0]), (1, [4], [0.5, 3, 0, 0]),
           (1, [4], [3, 3, 0, 0]), (1, [1], [0, 0, 0, 0]), (2, [7, 7], [0, 1, 0, 0] * 2), (0, [7], [0, 1, 0, 0])]
    for n, fam, params in bad:
        assert call(n, fam, params) == EINVAL, (n, fam, params)
        assert np.array_equal(eng.debug_theta_rows(x)[1], before), (n, fam, params)
    assert call(1, [7], [0, 1, 0, 0], field=1) == EINVAL                   # a one-field context
    assert call(1, [7], [0, 1, 0, 0]) == 0                                 # and a good one takes effect
    assert np.allclose(eng.debug_theta_rows(x)[1], st.halfnorm(0, 1).logpdf(x[:, 0]), rtol=1e-14)


def test_set_priors_needs_a_layout():
    from psfmc_amd import engine
    case = helpers.load_case('synth128x2')
    ctx = engine.Context(case['sci'], 1.0 / case['ivm'], np.zeros(case['sci'].shape, dtype=bool),
                         case['psfs'][:1], 1.0 / case['psf_ivms'][:1], n_ps=0, n_sersic=1, max_walkers=8)
    with pytest.raises(engine.NativeError):
        ctx.set_priors([7], [(0.0, 1.0)])
    ctx.close()


# -- a model of new-family priors through every device path ---------------------------------------------
def new_family_model(max_walkers=128, shift=0.0):
    """Sky + one Sersic on the synth128x2 field; eight free columns under seven of the new families (the
    position a vector prior with per-element loc)."""
    from psfmc_amd import MultiComponentModel
    from psfmc_amd.ModelComponents import Configuration, Sersic, Sky
    from psfmc_amd import distributions as D
    case = helpers.load_case('synth128x2')
    cfg = Configuration(case['sci'], case['ivm'], case['psfs'][0], case['psf_ivms'][0], mag_zeropoint=25.0)
    comps = [cfg, Sky(adu=D.Logistic(loc=0.0, scale=0.01 + shift)),
             Sersic(xy=D.TruncatedNormal(-4.0, 4.0, loc=[64.2 + shift, 63.1], scale=[0.5, 0.6]),
                    mag=D.Cauchy(loc=20.0 + shift, scale=0.3), reff=D.LogNormal(0.3, scale=8.0),
                    reff_b=D.Reciprocal(1.0, 12.0), index=D.Beta(2.0, 3.0, loc=0.3, scale=6.0),
                    angle=D.T(4.0, loc=0.3, scale=0.5 + shift))]
    return MultiComponentModel(comps, max_walkers=max_walkers)


def start_walkers(n, seed):
    rng = np.random.RandomState(seed)
    truth = np.array([0.0, 0.3, 2.0, 20.0, 8.0, 5.0, 64.2, 63.1])      # adu, angle, index, mag, reff, reff_b, x, y
    spread = np.array([0.005, 0.1, 0.2, 0.1, 0.3, 0.3, 0.2, 0.2])
    return truth + spread * rng.randn(n, truth.size)


def test_model_of_new_families_runs_on_the_device():
    model = new_family_model()
    model.engine
    assert model._host_priors == []
    assert model.num_params == 8
    theta = start_walkers(48, 1)
    theta[3, 5] = 9.0                     # reff_b > reff: outside the support
    theta[4, 2] = 0.2                     # index below beta's support
    dev = model.log_posterior_batch(theta)
    host = model.log_posterior_batch_host(theta)
    assert np.array_equal(np.isneginf(dev), np.isneginf(host)) and np.isneginf(dev[[3, 4]]).all()
    fin = np.isfinite(host)
    assert fin.sum() >= 45
    assert helpers.rel_err(dev[fin], host[fin]) <= 1e-12
    # the device's log-priors are scipy's
    _, lnprior, skip = model.engine.debug_theta_rows(theta)
    want = model.log_priors_batch(theta)
    assert np.array_equal(skip, ~np.isfinite(want))
    assert helpers.rel_err(lnprior[~skip], want[~skip]) <= 1e-13
    model.close()


@pytest.mark.parametrize('speculate', [-1, 0])
def test_device_sampler_reproduces_host_sampler_with_new_families(speculate):
    from psfmc_amd.sampler import EnsembleSampler, DeviceEnsembleSampler
    model = new_family_model(max_walkers=64)
    p0 = start_walkers(40, 2)
    model.engine.set_option('speculate', speculate)
    host = EnsembleSampler(40, model.num_params, batch_lnpostfn=model.log_posterior_batch)
    dev = DeviceEnsembleSampler(40, model, block=7)
    for s in (host, dev):
        s.random_state = np.random.RandomState(11).get_state()
    out_h = list(host.sample(p0, iterations=20))
    out_d = list(dev.sample(p0, iterations=20))
    assert np.array_equal(dev.chain, host.chain)
    assert np.array_equal(dev.naccepted, host.naccepted)
    assert np.array_equal(dev.lnprobability, host.lnprobability)
    assert np.array_equal(out_d[-1][0], out_h[-1][0])
    assert 0.02 < dev.acceptance_fraction.mean() < 0.95
    if speculate == 0:
        assert model.engine.get_option('speculated_runs') == 0
    else:
        assert model.engine.get_option('speculated_runs') > 0
    model.close()


def test_model_galaxy_mcmc_picks_the_device_sampler(tmp_path, monkeypatch):
    from psfmc_amd import fitting
    from psfmc_amd.sampler import DeviceEnsembleSampler
    made = []

    class Recording(DeviceEnsembleSampler):
        def __init__(self, *args, **kwargs):
            made.append(self)
            super().__init__(*args, **kwargs)

    def no_host(*args, **kwargs):
        raise AssertionError('the host sampler was chosen')
    monkeypatch.setattr(fitting, 'DeviceEnsembleSampler', Recording)
    monkeypatch.setattr(fitting, 'EnsembleSampler', no_host)
    model = new_family_model(max_walkers=64)
    np.random.seed(5)
    fitting.model_galaxy_mcmc(model, output_name=str(tmp_path / 'out'), iterations=6, burn=4, chains=18,
                              random_state=3, quiet=True, write_fits=[])
    assert len(made) == 1 and made[0].chain.shape[0] == 18
    model.close()


def test_field_set_of_new_family_models():
    """Two fields with different prior parameters: the FieldSet builds, and each field's log-posteriors are
    its own model's."""
    from psfmc_amd import FieldSet
    a, b = new_family_model(max_walkers=64), new_family_model(max_walkers=64, shift=0.05)
    theta = start_walkers(24, 3)
    want = [a.log_posterior_batch(theta), b.log_posterior_batch(theta)]
    assert not np.array_equal(want[0], want[1])
    fs = FieldSet([a, b], max_walkers=64)
    got = fs.log_posterior_batch([theta, theta])
    for g, w in zip(got, want):
        fin = np.isfinite(w)
        assert np.array_equal(fin, np.isfinite(g)) and fin.sum() >= 20
        assert helpers.rel_err(g[fin], w[fin]) <= 1e-12
    fs.close()
    a.close()
    b.close()


def test_evaluate_device_and_device_group_take_the_model():
    import torch
    from psfmc_amd.parallel import ShardedLogPosterior
    model = new_family_model(max_walkers=64)
    theta = start_walkers(32, 4)
    want = model.log_posterior_batch(theta)
    sharded = ShardedLogPosterior(model)
    got = sharded.evaluate_device(torch.from_numpy(theta).to('cuda:%d' % model._device)).cpu().numpy()
    assert np.array_equal(got, want)
    grp = model.device_group([0, 0], max_walkers=64)
    assert np.array_equal(grp.logpost_theta(theta), want)
    grp.close()
    model.close()
