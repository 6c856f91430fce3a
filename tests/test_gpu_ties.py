"""Ties, `Tied(source, ratio, offset)`, on the device.  Every tied model is held to its UNTIED TWIN (the same
components, a wide `Uniform` in place of each `Tied`) at vectors the test expands itself with plain numpy
`ratio * source + offset` (tests/test_ties.py `expand`): derived rows, skip flags and log-likelihoods BIT FOR BIT, the
log-prior against scipy, four walkers of each evaluation against the numpy contract of the twin, every device sampler
against its host contract, the Fisher entry against the definition, a planted co-centred quasar + host found by
`find_mode`, the library's refusals, and neutrality towards contexts that never saw a tie.  Shapes: 64 x 64 and one
embedded 70 x 66; evaluations of 70 walkers (a second, partly filled workgroup of k_theta_prep), ensembles of at most
32 walkers and 8 iterations."""
import numpy as np
import pytest

import test_gpu_general_components as tgg
import test_ties as tt
from psfmc_amd import JointModel, MultiComponentModel, Tied
from psfmc_amd.ModelComponents import PointSource, Sersic, Sky

pytestmark = pytest.mark.gpu

N_EVAL = 70
CONTRACT_WALKERS = (0, 1, 64, 69)            # two of the first workgroup of k_theta_prep, two of the second
make_field, oracle_field, contract_evaluate = tgg.make_field, tgg.oracle_field, tgg.contract_evaluate

_PAIRS = {}


def pair(which, shape=(64, 64)):
    """(field, ties, theta [70, P] of the tied model, the twin's expansion, the twin's contract log-likelihoods of
    CONTRACT_WALKERS) of the quasar (0) or the general (1) model on a shape: computed once, shared, left unchanged.
    Walker 5's ratio puts reff_b above reff -- outside the support through a resolved value only; walker 66's point
    source magnitude is outside its own prior."""
    key = (which, shape)
    if key not in _PAIRS:
        components, ties, draw = tt.MODELS[which]
        fld = make_field(*shape, seed=21 + which)
        tied, twin = tt.build(components, fld, True), tt.build(components, fld, False)
        theta = draw(tied, fld, N_EVAL, seed=22)
        if which == 0:
            theta[5, tt.columns_of(tied, '2_Sersic_reff_b_ratio')[0]] = 1.15
            theta[66, tt.columns_of(tied, '1_PointSource_mag')[0]] = 30.0
        else:
            theta[5, tt.columns_of(tied, '3_Sersic_trunc_out_lo')[0]] = 19.5
            theta[66, tt.columns_of(tied, '2_PointSource_mag')[0]] = 30.0
        full = tt.expand(tied, twin, ties, theta)
        field = oracle_field(fld)
        want = [contract_evaluate(twin, field, full[i])[0] for i in CONTRACT_WALKERS]
        _PAIRS[key] = (fld, ties, theta, full, want)
    return _PAIRS[key]


def models(which, fld, **kw):
    components = tt.MODELS[which][0]
    return tt.build(components, fld, True, **kw), tt.build(components, fld, False, **kw)


# -- 1. the records -------------------------------------------------------------------------------------------------
def test_device_rows_equal_the_twins():
    fld, ties, theta, full, _ = pair(0)
    tied, twin = models(0, fld, max_walkers=N_EVAL)
    rows, lnprior, skip = tied.engine.debug_theta_rows(theta)
    rows2, _, skip2 = twin.engine.debug_theta_rows(full)
    assert np.array_equal(skip, skip2) and list(np.flatnonzero(skip)) == [5, 66]
    assert np.array_equal(rows, rows2) and np.all(np.isfinite(rows[~skip])) and np.any(rows[~skip] != 0)
    want = tt.scipy_prior_sum(tied, theta)
    assert np.isfinite(want[5]) and want[66] == -np.inf           # walker 5 is outside through its resolved reff_b only
    ok = ~skip
    err = np.max(np.abs(lnprior[ok] - want[ok]) / np.abs(want[ok]))
    print('device log-prior against scipy: %.2e relative' % err)
    assert err <= 5e-14 and np.all(lnprior[skip] == -np.inf)
    tied.close()
    twin.close()


def test_the_tie_is_two_roundings_not_a_fused_multiply_add():
    """A centre tied with a ratio prior AND an offset prior: the device's row holds x0, y0 = fl(fl(ratio * source) +
    offset), numpy's bits, for all 70 walkers -- and the vectors are such that the single rounding of a fused
    multiply-add (the exact value, from rationals, rounded once) differs for some of them, so a contracted kernel
    fails here."""
    from fractions import Fraction
    fld = pair(0)[0]
    U, N = tt.U, tt.N
    centre = U((24.0, 24.0), (40.0, 40.0))
    model = MultiComponentModel([
        tt._config(fld), Sky(adu=N(0.05, 0.05)), PointSource(xy=centre, mag=U(17.0, 21.0)),
        Sersic(xy=Tied(centre, ratio=U(0.9, 1.1), offset=N((0.0, 0.0), (0.5, 0.5))), mag=18.0, reff=8.0, reff_b=5.0,
               index=1.5, angle=0.3)], max_walkers=N_EVAL)
    assert model.param_names == ['0_Sky_adu', '1_PointSource_mag', '1_PointSource_xy', '2_Sersic_xy_offset',
                                 '2_Sersic_xy_ratio']
    rng = np.random.RandomState(81)
    theta = np.column_stack([rng.uniform(0.04, 0.06, N_EVAL), rng.uniform(18.0, 20.0, N_EVAL),
                             rng.uniform(28.0, 36.0, (N_EVAL, 2)), rng.uniform(-0.7, 0.7, (N_EVAL, 2)),
                             rng.uniform(0.95, 1.05, N_EVAL)])
    src, off, ratio = theta[:, 2:4], theta[:, 4:6], theta[:, 6:7]
    want = ratio * src + off
    fused = np.array([[float(Fraction(r) * Fraction(s) + Fraction(o)) for s, o in zip(ss, oo)]
                      for r, ss, oo in zip(ratio[:, 0], src, off)])
    differ = int(np.sum(fused != want))
    print('%d of %d resolved values differ between two roundings and one' % (differ, want.size))
    assert differ >= 10
    rows, _, skip = model.engine.debug_theta_rows(theta)
    assert not skip.any()
    x0 = 1 + 4                                                      # sky | flux, x, y, method | x0, y0, ...
    assert np.array_equal(rows[:, x0:x0 + 2], want)
    assert np.array_equal(np.reshape(model.tied_values(theta)['2_Sersic_xy'], (N_EVAL, 2)), want)
    model.close()


# -- 2., 3. the log-likelihoods ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend,shape', [('fused', (64, 64)), ('hipfft', (64, 64)), ('fused', (70, 66))],
                         ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
@pytest.mark.parametrize('which', [0, 1], ids=['qso', 'general'])
def test_loglike_equals_the_twins_and_the_contract(which, backend, shape):
    fld, ties, theta, full, want = pair(which, shape)
    tied, twin = models(which, fld, backend=backend, max_walkers=N_EVAL)
    if shape == (70, 66):
        assert (int(tied.engine.get_option('transform_ny')), int(tied.engine.get_option('transform_nx'))) != shape
    ll, lp = tied.log_likelihood_and_prior_batch(theta)
    ll2, lp2 = twin.log_likelihood_and_prior_batch(full)
    assert np.array_equal(ll, ll2)
    assert list(np.flatnonzero(~np.isfinite(ll))) == ([5, 66] if which == 0 else [66])
    assert np.array_equal(np.isfinite(lp), np.isfinite(lp2))
    prior = tt.scipy_prior_sum(tied, theta)
    fin = np.isfinite(lp)
    assert np.max(np.abs(lp[fin] - prior[fin]) / np.abs(prior[fin])) <= 5e-14
    for i, w in zip(CONTRACT_WALKERS, want):
        print('%s walker %d: device %.9f, contract %.9f' % (backend, i, ll[i], w))
        assert np.isfinite(w) and abs(ll[i] - w) <= 1e-9 * abs(w), (i, ll[i], w)
    assert np.array_equal(tied.log_posterior_batch(theta)[fin], (ll + lp)[fin])
    # the host path's rows, the tie resolved by numpy on the host
    assert np.array_equal(tied.log_likelihood_batch(theta[:8]), twin.log_likelihood_batch(full[:8]))
    tied.close()
    twin.close()


# -- 4. the samplers ------------------------------------------------------------------------------------------------
def _start(model, fld, n_w, seed):
    return tt.qso_theta(model, fld, n_w, seed, spread=0.02)


@pytest.mark.parametrize('de', [False, True], ids=['stretch', 'de'])
@pytest.mark.parametrize('n_w', [22, 32])
def test_device_sampler_equals_the_host_sampler(n_w, de):
    """22 walkers: the whole-iteration route of small ensembles; 32: half-steps."""
    from psfmc_amd.sampler import DEMove, DeviceEnsembleSampler, EnsembleSampler, StretchMove
    fld = pair(0)[0]
    model = tt.build(tt.qso_components, fld, True, max_walkers=n_w)
    p0 = _start(model, fld, n_w, 31)
    kw = dict(moves=[(DEMove(), 0.5), (StretchMove(), 0.5)]) if de else {}
    host = EnsembleSampler(n_w, model.num_params, batch_lnpostfn=model.log_posterior_batch, live_dangerously=True, **kw)
    dev = DeviceEnsembleSampler(n_w, model, block=3, live_dangerously=True, **kw)
    for s in (host, dev):
        s.random_state = np.random.RandomState(32).get_state()
    list(host.sample(p0, iterations=8))
    list(dev.sample(p0, iterations=8))
    assert dev.chain.shape == (n_w, 8, model.num_params) and model.num_params == 14
    assert np.array_equal(dev.chain, host.chain) and np.array_equal(dev.naccepted, host.naccepted)
    assert np.array_equal(dev.lnprobability, host.lnprobability)
    assert dev.naccepted.sum() > 0 and np.all(np.isfinite(dev.lnprobability))
    model.close()


def test_tempered_sampler_equals_the_host_contract():
    from psfmc_amd.sampler import DeviceTemperedSampler, TemperedEnsembleSampler, default_betas
    fld = pair(0)[0]
    n_t, n_w = 3, 28
    model = tt.build(tt.qso_components, fld, True, max_walkers=n_t * n_w)
    betas = default_betas(n_t, 50.0)
    p0 = _start(model, fld, n_t * n_w, 33).reshape(n_t, n_w, -1)
    host = TemperedEnsembleSampler(n_w, model.num_params, betas, model.log_likelihood_and_prior_batch)
    dev = DeviceTemperedSampler(n_w, model, betas=betas, block=3)
    for s in (host, dev):
        s.random_state = np.random.RandomState(34).get_state()
    list(host.sample(p0, iterations=8))
    list(dev.sample(p0, iterations=8))
    assert dev.chain.shape[-1] == model.num_params
    assert np.array_equal(dev.chain, host.chain) and np.array_equal(dev.lnprobability, host.lnprobability)
    assert np.array_equal(dev.lnlikelihood, host.lnlikelihood)
    assert np.array_equal(dev.naccepted_t, host.naccepted_t) and np.array_equal(dev.nswap, host.nswap)
    assert np.all(np.isfinite(dev.lnlikelihood)) and dev.naccepted_t.sum() > 0
    model.close()


def _untied_14(fld):
    """An untied model of the quasar model's component lists and as many free parameters (14)."""
    ny, nx = fld['shape']
    c = np.array((nx / 2.0, ny / 2.0))
    U, N = tt.U, tt.N
    return [tt._config(fld), Sky(adu=N(0.05, 0.05)), PointSource(xy=U(c - 4.0, c + 4.0), mag=U(17.0, 21.0)),
            Sersic(xy=U(c - 6.0, c + 6.0), mag=U(16.0, 22.0), reff=U(2.0, 22.0), reff_b=U(1.0, 22.0), index=U(0.5, 6.0),
                   angle=U(-180.0, 180.0), angle_degrees=True),
            Sersic(xy=(nx / 2 + 0.4, ny / 2 - 0.3), mag=U(16.0, 22.0), reff=U(1.0, 30.0), reff_b=U(0.5, 30.0), index=1.0,
                   angle=100.0, angle_degrees=True)]


def test_field_set_of_a_tied_and_an_untied_field():
    from psfmc_amd import EnsembleSampler, FieldSet, FieldSetSampler
    fa, fb = make_field(64, 64, seed=41), make_field(64, 64, seed=42)
    tied = tt.build(tt.qso_components, fa, True, max_walkers=1)
    plain = MultiComponentModel(_untied_14(fb), max_walkers=1)
    n_w = 28
    for order in ((tied, plain), (plain, tied)):                       # the tied field first, and second
        fs = FieldSet(list(order), max_walkers=2 * n_w)
        p0 = []
        for m, f in zip(fs.models, (fa, fb) if order[0] is tied else (fb, fa)):
            if m._ties:
                p0.append(_start(m, f, n_w, 43))
            else:
                base = np.array([0.05, 19.0, 32.3, 31.6, 30.0, 2.0, 18.5, 9.0, 5.0, 32.5, 31.0, 19.0, 11.0, 6.0])
                p0.append(base + np.random.RandomState(44).normal(size=(n_w, 14)) * 1e-2)
        samp = FieldSetSampler(n_w, fs, block=3)
        for f, sub in enumerate(samp.fields):
            sub.random_state = np.random.RandomState(45 + f).get_state()
        list(samp.sample(p0, iterations=6))
        for f, sub in enumerate(samp.fields):
            host = EnsembleSampler(n_w, fs.num_params, batch_lnpostfn=fs.models[f].log_posterior_batch)
            host.random_state = np.random.RandomState(45 + f).get_state()
            list(host.sample(p0[f], iterations=6))
            assert sub.chain.shape == (n_w, 6, 14)
            assert np.array_equal(sub.chain, host.chain), f
            assert np.array_equal(sub.lnprobability, host.lnprobability), f
            assert host.naccepted.sum() > 0 and np.all(np.isfinite(host.lnprobability))
        fs.close()


def test_joint_model_whose_tie_source_is_per_field():
    """Two exposures; the point source's position is per field, so the hosts' centres follow each exposure's own."""
    from psfmc_amd.sampler import DeviceEnsembleSampler, EnsembleSampler
    fa, fb = make_field(64, 64, seed=51), make_field(70, 66, seed=52)
    joint = JointModel([tt.build(tt.qso_components, f, True, max_walkers=1) for f in (fa, fb)],
                       per_field=['1_PointSource_xy'], max_walkers=2 * 32)
    assert joint.num_params == 16 and '2_Sersic_xy' not in joint.param_names
    n_w = 32
    base = _start(joint.field_models[0], fa, n_w, 53)
    p0 = np.zeros((n_w, joint.num_params))
    p0[:, joint.field_columns(0)] = base
    other = base.copy()
    other[:, tt.columns_of(joint.field_models[1], '1_PointSource_xy')] += (1.0, 3.0)
    p0[:, joint.field_columns(1)] = other
    assert np.array_equal(joint.field_theta(p0, 0), base) and np.array_equal(joint.field_theta(p0, 1), other)
    # the joint log-posterior: the fields' own tied models' likelihoods (their twins' bits, see above) and the prior
    got = joint.log_posterior_batch(p0)
    twins = [tt.build(tt.qso_components, f, False, max_walkers=n_w) for f in (fa, fb)]
    owns = [tt.build(tt.qso_components, f, True) for f in (fa, fb)]
    ll = [t.log_likelihood_and_prior_batch(tt.expand(o, t, tt.QSO_TIES, joint.field_theta(p0, f)))[0]
          for f, (o, t) in enumerate(zip(owns, twins))]
    want = (ll[0] + ll[1]) + joint.log_priors_batch(p0)
    assert np.all(np.isfinite(want)) and np.max(np.abs(got - want) / np.abs(want)) <= 1e-12
    for t in twins:
        t.close()
    host = EnsembleSampler(n_w, joint.num_params, batch_lnpostfn=joint.log_posterior_batch)
    dev = DeviceEnsembleSampler(n_w, joint, block=3)
    for s in (host, dev):
        s.random_state = np.random.RandomState(54).get_state()
    list(host.sample(p0, iterations=6))
    list(dev.sample(p0, iterations=6))
    assert dev.chain.shape == (n_w, 6, 16)
    assert np.array_equal(dev.chain, host.chain) and np.array_equal(dev.lnprobability, host.lnprobability)
    assert host.naccepted.sum() > 0 and np.all(np.isfinite(host.lnprobability))
    # a walker outside the support through a resolved value only
    bad = p0[:1].copy()
    names = sum(([n] * w for n, w in zip(joint.param_names, joint.param_lens)), [])
    bad[0, names.index('2_Sersic_reff_b_ratio')] = 1.15
    assert joint.log_posterior_batch(bad)[0] == -np.inf and joint.log_priors_batch(bad)[0] == -np.inf
    joint.close()


def test_sharded_half_steps_equal_one_context():
    """Two ranks inside one process (tests/shard_driver.py), 28 walkers: every rank's chain is bit-identical to one
    `DeviceEnsembleSampler`'s on one more context."""
    import shard_driver as sd
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = pair(0)[0]
    ranks, n_w, seed = 2, 28, 7
    all_models = [tt.build(tt.qso_components, fld, True, max_walkers=n_w) for _ in range(ranks + 1)]
    single, shards = all_models[-1], all_models[:-1]
    p0 = _start(single, fld, n_w, 61)
    draws = sd.draw(sd.random_state(seed), sd.N_ITER, n_w, single.num_params)
    lnp0 = shards[0].log_posterior_batch(p0)
    samp = DeviceEnsembleSampler(n_w, single)
    samp.random_state = sd.random_state(seed)
    list(samp.sample(p0, iterations=sd.N_ITER))
    res = sd.run_blocks(shards, p0, lnp0, draws)
    for r in range(ranks):
        assert np.array_equal(res['chain'][r], samp.chain), r
        assert np.array_equal(res['lnchain'][r], samp.lnprobability), r
    assert samp.naccepted.sum() > 0 and np.all(np.isfinite(res['gathered']))
    grp = single.device_group([0], max_walkers=n_w)
    assert np.array_equal(grp.logpost_theta(p0), lnp0)
    grp.close()
    for m in all_models:
        m.close()


# -- 5. the Fisher entry and the mode search ----------------------------------------------------------------------------
def _tied_fisher_case():
    fld, ties, theta, full, _ = pair(0)
    twin = tt.build(tt.qso_components, fld, False, backend='hipfft')        # host side only: the contract's raw model
    build = lambda backend: tt.build(tt.qso_components, fld, True, backend=backend, max_walkers=64)
    tied = build('hipfft')
    evaluate = lambda field, t: contract_evaluate(twin, field, tt.expand(tied, twin, ties, t)[0])
    return dict(build=build, field=oracle_field(fld), layout=None, has_psf_index=False, theta=theta[0],
                n_columns=tied.num_params, evaluate=evaluate)


@pytest.mark.parametrize('backend', ['fused', 'hipfft'])
def test_fisher_of_a_tied_model_against_the_definition(backend):
    """`model.fisher` of the tied model against `mode.fisher_from_stencil` on the twin's contract images of the
    expanded stencil vectors, at the bound tests/test_gpu_fisher.py derives for an untied model
    (`mode_helpers.fisher_error_bound`), and on its own images at `fisher_rounding_bound`."""
    import mode_helpers as mh
    import test_gpu_fisher as tgf
    from psfmc_amd import mode
    ref = tgf.reference('tied-qso', _tied_fisher_case)
    model = ref['case']['build'](backend)
    out = model.fisher(ref['case']['theta'])
    assert np.array_equal(out['columns'], ref['columns']) and len(out['columns']) == 14
    err_f, err_g = mh.fisher_errors(out['F'], out['grad'], ref['F'], ref['g'])
    print('tied %s: normalised error F %.3g (bound %.3g), g %.3g (bound %.3g)' % (
        backend, err_f, ref['bounds'][0], err_g, ref['bounds'][1]))
    assert err_f <= ref['bounds'][0] and err_g <= ref['bounds'][1]
    want_ll = ref['imgs']['ll'][0]
    assert abs(out['loglike'] - want_ll) <= 1e-9 * abs(want_ll)
    vecs = mode.stencil(ref['case']['theta'], ref['step'], ref['columns'])[0]
    tgf.held_to_own_images(model, vecs, out, 0.5 / ref['step'][0], 'tied %s' % backend)
    model.close()


def planted_components(fld):
    """Sky + a point source and an exponential host on ONE centre with the axis ratio q fitted: 9 free parameters."""
    ny, nx = fld['shape']
    c = np.array((nx / 2.0, ny / 2.0))
    U, N = tt.U, tt.N
    centre, size = U(c - 6.0, c + 6.0), U(2.0, 20.0)
    return [tt._config(fld), Sky(adu=N(0.05, 0.05)), PointSource(xy=centre, mag=U(16.0, 22.0)),
            Sersic(xy=Tied(centre), mag=U(15.0, 22.0), reff=size, reff_b=Tied(size, ratio=U(0.1, 0.9)), index=1.0,
                   angle=U(-90.0, 270.0), angle_degrees=True)]


def test_find_mode_on_a_planted_quasar_and_host():
    from psfmc_amd import find_mode
    fld = make_field(64, 64, seed=71)
    first = MultiComponentModel(planted_components(fld), max_walkers=1)
    assert first.param_names == ['0_Sky_adu', '1_PointSource_mag', '1_PointSource_xy', '2_Sersic_angle', '2_Sersic_mag',
                                 '2_Sersic_reff', '2_Sersic_reff_b_ratio']
    truth = np.array([0.05, 18.5, 32.3, 31.6, 35.0, 17.5, 8.0, 0.55])
    # the planted image: the contract's convolved model of the untied equivalent at the expanded truth
    ny, nx = fld['shape']
    untied = MultiComponentModel([tt._config(fld), Sky(adu=tt.N(0.05, 0.05)),
                                  PointSource(xy=tt.U((20.0, 20.0), (44.0, 44.0)), mag=tt.U(16.0, 22.0)),
                                  Sersic(xy=tt.U((20.0, 20.0), (44.0, 44.0)), mag=tt.U(15.0, 22.0), reff=tt.U(2.0, 20.0),
                                         reff_b=tt.U(0.2, 20.0), index=1.0, angle=tt.U(-90.0, 270.0), angle_degrees=True)],
                                 max_walkers=1)
    full = np.array([0.05, 18.5, 32.3, 31.6, 35.0, 17.5, 8.0, 0.55 * 8.0 + 0.0, 1.0 * 32.3 + 0.0, 1.0 * 31.6 + 0.0])
    conv = contract_evaluate(untied, oracle_field(fld), full)[1]['convolved_model']
    noise = fld['sci'].astype(np.float64) - 0.05
    data = dict(fld, sci=(conv + noise).astype(np.float32))
    model = MultiComponentModel(planted_components(data), max_walkers=64)
    start = truth * (1.0 + 0.02 * np.where(np.arange(len(truth)) % 2, -1.0, 1.0))
    res = find_mode(model, start=start)
    at_truth = model.log_posterior_batch(truth[None])[0]
    print('find_mode: %r; log-posterior at the truth %.6f' % (res, at_truth))
    assert res.converged and res.ok and len(res.columns) == 8
    assert res.lnpost >= at_truth and res.lnpost == model.log_posterior_batch(res.theta)[0]
    np.linalg.cholesky(res.cov)
    sigma = np.sqrt(np.diag(res.cov))
    assert np.all(np.abs(res.theta - truth) <= 5.0 * sigma), (res.theta - truth) / sigma
    model.close()


# -- 6. the library's refusals ------------------------------------------------------------------------------------------
def test_the_library_refuses_what_the_header_says():
    from psfmc_amd.engine import MAX_TIES, NativeError
    fld = pair(0)[0]
    tied = tt.build(tt.qso_components, fld, True, max_walkers=4)
    eng, p = tied.engine, tied.num_params
    theta = pair(0)[2][:2]
    before = tied.log_posterior_batch(theta)
    ok = ([0], [-1], [1.0], [-1], [0.0])
    with pytest.raises(NativeError, match='n_ties=%d outside' % (MAX_TIES + 1)):
        eng.set_ties(*[v * (MAX_TIES + 1) for v in ok])
    with pytest.raises(NativeError, match='source column -1'):
        eng.set_ties([-1], [-1], [1.0], [-1], [0.0])
    with pytest.raises(NativeError, match='ratio column -2'):
        eng.set_ties([0], [-2], [1.0], [-1], [0.0])
    with pytest.raises(NativeError, match='offset column -3'):
        eng.set_ties([0], [-1], [1.0], [-3], [0.0])
    with pytest.raises(NativeError, match='must be finite'):
        eng.set_ties([0], [-1], [np.inf], [-1], [0.0])
    with pytest.raises(NativeError, match='must be finite'):
        eng.set_ties([0], [-1], [1.0], [-1], [np.nan])
    assert np.array_equal(tied.log_posterior_batch(theta), before)           # a refused call changes nothing
    # the calls that pass a table: a plain context of the same structure, registered by hand
    n_slots = 1 + 3 + 7 * 2 + 1
    col = [-1] * n_slots
    layout = lambda c, n_par=p: eng.set_layout(1, n_par, c, [1.0] * n_slots, [0], [1, 1], 25.0,
                                               np.ones(n_par, dtype=np.int32), np.zeros(n_par), np.ones(n_par), np.zeros(n_par))
    eng.set_ties(*ok)
    with pytest.raises(NativeError, match='refers to tie 1 of 1'):
        layout([-3] + col[1:])
    with pytest.raises(NativeError, match='PSF index, cannot be tied'):
        layout(col[:-1] + [-2])
    eng.set_ties([p], [-1], [1.0], [-1], [0.0])
    with pytest.raises(NativeError, match='source column %d' % p):
        layout([-2] + col[1:])
    eng.set_ties([0], [p], [1.0], [-1], [0.0])
    with pytest.raises(NativeError, match='ratio column %d' % p):
        layout([-2] + col[1:])
    eng.set_ties([0], [-1], [1.0], [p + 3], [0.0])
    with pytest.raises(NativeError, match='offset column %d' % (p + 3)):
        layout([-2] + col[1:])
    # the model's own registration again: the context computes what it computed
    tied._register_layout(eng)
    assert np.array_equal(tied.log_posterior_batch(theta), before)
    tied.close()
    # an aux table and a block's table naming a tie the field does not have
    gen = tt.build(tt.gen_components, pair(1)[0], True, max_walkers=4)
    eng = gen.engine
    n_aux = 2 * 2 + 2
    with pytest.raises(NativeError, match='aux value 4 refers to tie 40 of'):
        eng.set_aux_layout([-1] * 4 + [-42, -1], [0.0] * n_aux, [True, True], [True, True])
    with pytest.raises(NativeError, match='bending value 1 refers to tie 40 of'):
        eng.set_bending_layout([2, 2], [-1, -42] + [-1] * 6, [0.0] * 8)
    gen.close()


# -- 7. neutrality ------------------------------------------------------------------------------------------------------
def test_a_context_that_had_ties_returns_the_bits_of_one_that_never_did():
    fld, ties, theta, full, _ = pair(0)
    tied, twin = models(0, fld, max_walkers=N_EVAL)
    fresh = tt.build(tt.qso_components, fld, False, max_walkers=N_EVAL)
    want = fresh.log_posterior_batch(full)
    first = tied.log_posterior_batch(theta)
    assert np.isfinite(first[0])
    # the twin's layout on the context that held the tied one's (same component lists): its ties cleared
    assert tied.engine.has_ties
    tied.engine.set_ties([], [], [], [], [])
    twin._register_layout(tied.engine)
    assert not tied.engine.has_ties
    assert np.array_equal(tied.engine.logpost_theta(full), want)
    rows, lnprior, skip = tied.engine.debug_theta_rows(full)
    rows2, lnprior2, skip2 = fresh.engine.debug_theta_rows(full)
    assert np.array_equal(rows, rows2) and np.array_equal(lnprior, lnprior2) and np.array_equal(skip, skip2)
    # and tied again
    tied._register_layout(tied.engine)
    assert np.array_equal(tied.log_posterior_batch(theta), first)
    for m in (tied, twin, fresh):
        m.close()
