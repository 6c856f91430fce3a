"""The pixel-averaged mode of the general components (`pixel_mean=True`) on the device, held to the numpy definition
(`Sersic.general_mean_image`) composed with the oracle's point source, convolution and likelihood: raw images per pixel
on every forward-kernel family of both back ends, batch independence and the support, the samplers, mixed models,
posterior sums, field sets, joint fits, f32 storage, context groups, the library's refusals, the untouched models
without the keyword and a planted narrow Moffat.  Field, model and contract helpers are those of
tests/test_gpu_general_components.py and tests/test_gpu_radial_laws.py."""
import numpy as np
import pytest

import psfmc_oracle as orc
import test_general_mean as tm
import test_gpu_fourier_modes as tgf
import test_gpu_general_components as tgg
import test_gpu_radial_laws as trl
import test_gpu_spiral_arms as tgs
from extra_contract import EDGE_MARGIN, law_error
from test_gpu_general_components import RAW_BOUND, contract_evaluate, contract_raw, make_field, oracle_field, raw_error
from test_gpu_radial_laws import build, column, named, vector
from psfmc_amd.ModelComponents import Ferrer, Moffat, Sersic
from psfmc_amd.ModelComponents.Sersic import (INTEG_GRID_FAR, INTEG_GRID_NEAR, INTEG_HALF_BOX, MEAN_EDGE_GRID)

pytestmark = pytest.mark.gpu

MEAN = dict(pixel_mean=True)


def mean_ferrer_state(model):
    """(smallest Sigma_0, smallest |1 - x| over every DECISION SAMPLE) of the model's Ferrer components with
    `pixel_mean=True` at the model's current values, from the definition alone: the centre and the four corners of
    every pixel, the 8 x 8 samples of every pixel the edge crosses, and the box pixels' grids.  (0, inf) without one."""
    sigma0, margin = [], np.inf
    ny, nx = model.config.obs_data.shape
    for comp in model.components:
        if not (isinstance(comp, Ferrer) and comp.pixel_mean):
            continue
        get = lambda k: getattr(comp, k)
        row = comp.derived_row(model.config.mag_zeropoint)
        box = float(np.ravel(comp.boxiness)[0]) if comp.has_boxiness else 0.0
        amps, phases = comp._fourier_values(get) if comp.has_fourier else ((), ())
        modes = list(zip(comp.fourier_modes, amps, phases))
        spiral = comp._spiral_values(get) if comp.has_spiral else None
        pars = comp._radial_values(get)
        x_of = lambda x, y: Sersic._general_point_x('ferrer', row, pars, box, modes, spiral, x, y)[1]
        sigma0.append(Sersic.radial_central('ferrer', row, pars, box, modes, spiral))
        yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
        cyy, cxx = np.mgrid[0:ny + 1, 0:nx + 1].astype(np.float64) - 0.5
        mid, cor = x_of(xx, yy), x_of(cxx, cyy)
        margin = min(margin, float(np.abs(1 - mid).min()), float(np.abs(1 - cor).min()))
        n_in = sum((a < 1.0).astype(int) for a in (mid, cor[:-1, :-1], cor[:-1, 1:], cor[1:, :-1], cor[1:, 1:]))
        todo = [(j, i, MEAN_EDGE_GRID) for j, i in zip(*np.nonzero((n_in > 0) & (n_in < 5)))]
        px, py = int(np.floor(row[0] + 0.5)), int(np.floor(row[1] + 0.5))
        for j in range(max(py - INTEG_HALF_BOX, 0), min(py + INTEG_HALF_BOX + 1, ny)):
            for i in range(max(px - INTEG_HALF_BOX, 0), min(px + INTEG_HALF_BOX + 1, nx)):
                todo += [(j, i, INTEG_GRID_NEAR), (j, i, INTEG_GRID_FAR)]
        for j, i, s in todo:
            o = (np.arange(s) + 0.5) / s - 0.5
            sx, sy = np.meshgrid(i + o, j + o)
            margin = min(margin, float(np.abs(1 - x_of(sx, sy)).min()))
    return (min(sigma0) if sigma0 else 0.0), margin


TWO = trl.TWO


def contract_sets(fld):
    """[(components, build keywords, [{name: value}])]: each law alone, a boxy Ferrer with modes and a spiral beside a
    mean Moffat and a plain Sersic, a mean Moffat beside a pixel-integrated Sersic, a non-mean general Sersic and a
    tilted sky -- ten walkers in five models.  Centres on pixel centres, edges and corners and outside the image; a
    Moffat of fwhm 1.1; Ferrers of r_out 0.31 and 3 times the side."""
    ny, nx = fld['shape']
    cx, cy = nx // 2, ny // 2
    small, large = 0.31 * min(ny, nx), 3.0 * max(ny, nx)
    faint = {'1_PointSource_mag': 23.9}
    return [
        ([(Sersic, dict(angle='free', boxiness='free', **MEAN))], dict(degrees=False), [
            named(2, 'Sersic', angle=0.5, boxiness=0.7, index=4.0, mag=18.0, reff=3.0, reff_b=1.5, xy=(float(cx), float(cy))),
            named(2, 'Sersic', angle=-1.1, boxiness=-0.8, index=1.0, mag=18.3, reff=2.0, reff_b=1.4, xy=(cx + 0.5, cy - 0.5))]),
        ([(Moffat, dict(angle='free', **MEAN))], dict(degrees=False), [
            named(2, 'Moffat', angle=0.5, beta=2.5, fwhm=1.1, fwhm_b=1.0, mag=18.0, xy=(cx + 0.31, cy - 0.27)),
            named(2, 'Moffat', angle=-0.5 * np.pi, beta=6.0, fwhm=9.0, fwhm_b=3.0, mag=18.3, xy=(cx + 0.5, float(cy))),
            named(2, 'Moffat', angle=0.2, beta=1.2, fwhm=20.0, fwhm_b=8.0, mag=18.9, xy=(nx + 5.0, ny + 2.5))]),
        ([(Ferrer, dict(angle='free', **MEAN))], dict(degrees=False), [
            dict(named(2, 'Ferrer', alpha=0.0, angle=0.4, beta=0.0, mag=18.0, r_out=small, r_out_b=0.6 * small,
                       xy=(cx + 0.37, cy - 0.21)), **faint),
            dict(named(2, 'Ferrer', alpha=4.0, angle=1.1, beta=-2.0, mag=15.0, r_out=large, r_out_b=0.5 * large,
                       xy=(-3.6, cy + 0.4)), **faint)]),
        ([(Ferrer, dict(angle='free', boxiness='free', fourier=TWO,
                        spiral=dict(r_in='free', r_out='free', winding='free', inclination=35.0, sky_angle=20.0), **MEAN)),
          (Moffat, dict(angle='free', **MEAN)), (Sersic, dict(angle='free'))], dict(degrees=True), [
            dict(named(2, 'Ferrer', alpha=2.0, angle=30.0, beta=0.0, boxiness=0.8, f2_amp=0.2, f2_phase=30.0, f3_amp=-0.1,
                       mag=18.0, r_out=small, r_out_b=0.35 * small, spiral_r_in=2.0, spiral_r_out=10.0,
                       spiral_wind=150.0, xy=(cx - 1.37, cy + 0.72)),
                 **dict(named(3, 'Moffat', angle=110.0, beta=2.5, fwhm=3.0, fwhm_b=1.5, mag=19.0, xy=(float(cx + 2), float(cy - 1))),
                        **named(4, 'Sersic', angle=-20.0, index=1.0, mag=18.5, reff=8.0, reff_b=3.0, xy=(cx + 3.2, cy - 1.1)))),
            dict(named(2, 'Ferrer', alpha=0.5, angle=-40.0, beta=1.5, boxiness=-0.4, f2_amp=-0.2, f2_phase=100.0, f3_amp=0.1,
                       mag=18.3, r_out=1.23 * small, r_out_b=0.5 * small, spiral_r_in=0.0, spiral_r_out=6.0,
                       spiral_wind=-200.0, xy=(cx + 0.5, float(cy))),
                 **dict(named(3, 'Moffat', angle=0.0, beta=1.2, fwhm=5.0, fwhm_b=5.0, mag=19.3, xy=(-2.5, -1.5)),
                        **named(4, 'Sersic', angle=45.0, index=4.0, mag=18.8, reff=3.0, reff_b=1.5, xy=(cx - 4.3, cy + 2.6))))]),
        ([(Sersic, dict(angle='free', integrate=True)), (Moffat, dict(angle='free', boxiness='free', **MEAN)),
          (Sersic, dict(angle='free', boxiness='free'))], dict(degrees=True, slope=True), [
            dict(named(2, 'Sersic', angle=100.0, index=3.0, mag=18.5, reff=4.0, reff_b=2.0, xy=(cx - 2.5, cy + 0.5)),
                 **dict(named(3, 'Moffat', angle=30.0, beta=2.5, boxiness=0.4, fwhm=2.0, fwhm_b=1.6, mag=18.8,
                              xy=(cx + 0.3, cy - 1.2)),
                        **named(4, 'Sersic', angle=-20.0, boxiness=-0.5, index=1.0, mag=18.6, reff=6.0, reff_b=3.0,
                                xy=(cx + 5.2, cy + 3.1))))]),
    ]


@pytest.mark.parametrize('backend,shape', [('fused', s) for s in tgg.SHAPES] + [('hipfft', (64, 64)), ('hipfft', (70, 66))],
                         ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_device_against_the_definition(backend, shape):
    """Raw image per pixel at RAW_BOUND -- relative to the pixel, relative to Sigma_0 for a model with a Ferrer (no pixel
    left out) -- after the host asserted that no decision sample of a Ferrer is within EDGE_MARGIN of the edge; the
    log-posterior through raw vectors and the log-likelihood through the host path's rows against the contract (1e-9).
    MEASURED worst per shape: DESIGN.md section 20."""
    fld = make_field(*shape, seed=1)
    field = oracle_field(fld)
    worst = 0.0
    for n_set, (comps, kw, cases) in enumerate(contract_sets(fld)):
        model = build(fld, comps, backend=backend, **kw)
        assert any(model.sersic_general_mean)
        thetas = np.array([vector(model, fld, v, adu=0.05 + 0.002 * i) for i, v in enumerate(cases)])
        want_all = []
        for i, t in enumerate(thetas):                                 # the host first: the condition on the inputs
            want_ll, images = contract_evaluate(model, field, t)
            sigma0, margin = mean_ferrer_state(model)
            assert margin >= EDGE_MARGIN, (shape, n_set, i, margin)
            want_all.append((want_ll, images, sigma0))
        imgs = model.sample_images(thetas, ('raw_model',))['raw_model']
        lp = model.log_posterior_batch(thetas)
        ll_rows = model.log_likelihood_batch(thetas)
        prior = model.log_priors_batch(thetas)
        for i, (want_ll, want, sigma0) in enumerate(want_all):
            tag = '%s %dx%d set %d case %d' % ((backend,) + shape + (n_set, i))
            if sigma0:
                err = law_error(imgs[i], want['raw_model'], sigma0, tag)
            else:
                err = raw_error(imgs[i], want['raw_model'], tag)
                print('%s: raw model max relative error %.2e' % (tag, err))
            worst = max(worst, err)
            assert np.isfinite(want_ll) and np.isfinite(prior[i])
            assert abs(ll_rows[i] - want_ll) <= 1e-9 * abs(want_ll), (tag, ll_rows[i], want_ll)
            assert abs(lp[i] - (want_ll + prior[i])) <= 1e-9 * abs(want_ll), (tag, lp[i], want_ll + prior[i])
        model.close()
    print('%s %dx%d: worst raw-model error %.2e' % ((backend,) + shape + (worst,)))
    assert worst <= RAW_BOUND


BOTH = [(Moffat, dict(angle='free', boxiness='free', **MEAN)), (Ferrer, dict(angle='free', boxiness='free', **MEAN))]


def test_batch_independence_and_the_support():
    """A walker's log-posterior bits are the same alone, in a batch of 64 and in permuted order; values outside the
    support are -inf from raw vectors and leave the other walkers' bits unchanged."""
    fld = make_field(64, 64, seed=4)
    model = build(fld, BOTH, max_walkers=64)
    thetas = trl._both_start(fld, model, 64, 5)
    full = model.log_posterior_batch(thetas)
    assert np.all(np.isfinite(full))
    for i in (0, 7, 63):
        assert model.log_posterior_batch(thetas[i:i + 1])[0] == full[i]
    perm = np.random.RandomState(6).permutation(64)
    assert np.array_equal(model.log_posterior_batch(thetas[perm]), full[perm])
    bad = [('2_Moffat_beta', 1.0), ('3_Ferrer_alpha', -0.1), ('3_Ferrer_beta', 2.0), ('2_Moffat_boxiness', -2.0),
           ('3_Ferrer_boxiness', np.nan)]
    where = [3 + 9 * k for k in range(len(bad))]
    mixed = thetas.copy()
    for k, (name, val) in zip(where, bad):
        mixed[k, column(model, name)] = val
    got = model.log_posterior_batch(mixed)
    keep = np.ones(64, dtype=bool)
    keep[where] = False
    assert np.all(got[where] == -np.inf) and np.array_equal(got[keep], full[keep])
    assert np.all(model.log_posterior_batch_host(mixed)[where] == -np.inf)
    # the keyword changes what is computed
    plain = build(fld, trl.BOTH, max_walkers=64)
    assert not np.array_equal(plain.log_posterior_batch(thetas[:4]), full[:4])
    plain.close()
    model.close()


LEAN = [(Ferrer, dict(boxiness='free', beta=0.5, r_out_b=6.0, **MEAN)), (Moffat, dict(xy=(33.6, 31.2), fwhm_b=2.5, **MEAN))]


@pytest.mark.parametrize('n_w', [22, 64])
def test_device_sampler_equals_the_host_sampler(n_w):
    from psfmc_amd.sampler import EnsembleSampler, DeviceEnsembleSampler
    fld = make_field(64, 64, seed=7)
    model = build(fld, LEAN, max_walkers=n_w, ps_free=False)
    assert model.num_params == 11
    p0 = trl._lean_start(fld, model, n_w, 2)
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
    from psfmc_amd.sampler import TemperedEnsembleSampler, DeviceTemperedSampler, default_betas
    fld = make_field(64, 64, seed=8)
    model = build(fld, LEAN, max_walkers=4 * 24, ps_free=False)
    betas = default_betas(4, 50.0)
    p0 = trl._lean_start(fld, model, 4 * 24, 3).reshape(4, 24, -1)
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


def test_accumulated_images_against_the_definition():
    fld = make_field(70, 66, seed=9)
    comps, kw, cases = contract_sets(fld)[3]
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


@pytest.mark.parametrize('order', [(0, 1), (1, 0)], ids=['mean-first', 'mean-last'])
def test_field_set_keeps_the_flag_per_field(order):
    """A 64x64 field with the keyword on both components and a 96x64 field with the same components without it,
    registered in either order, against each field's own context: within 1e-12 of the largest value, bit-identical
    where the own context has the set's transform."""
    from psfmc_amd.models import FieldSet
    flds = [make_field(64, 64, seed=10), make_field(96, 64, seed=11)]
    specs = [BOTH, trl.BOTH]
    flds, specs = [flds[i] for i in order], [specs[i] for i in order]
    fs = FieldSet([build(f, s, max_walkers=1) for f, s in zip(flds, specs)], max_walkers=32)
    own = [build(f, s, max_walkers=16) for f, s in zip(flds, specs)]
    assert sorted(any(m.sersic_general_mean) for m in fs.models) == [False, True]
    thetas = [trl._both_start(f, m, 4, 12, scale=0.05) for f, m in zip(flds, own)]
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


def test_joint_model():
    from psfmc_amd import JointModel
    fa, fb = make_field(64, 64, seed=12), make_field(70, 66, seed=13)
    joint = JointModel([build(fa, BOTH, max_walkers=1, extent=70), build(fb, BOTH, max_walkers=1, extent=70)],
                       per_field=['3_Ferrer_r_out', '1_PointSource_xy', '2_Moffat_xy', '3_Ferrer_xy'], max_walkers=32)
    own_a, own_b = build(fa, BOTH, max_walkers=1, extent=70), build(fb, BOTH, max_walkers=1, extent=70)
    base_a, base_b = trl._both_start(fa, own_a, 3, 14, scale=0.02), trl._both_start(fb, own_b, 3, 14, scale=0.02)
    base_b[:, column(own_b, '3_Ferrer_r_out')] += 3.0
    thetas = np.zeros((3, joint.num_params))
    thetas[:, joint.field_columns(1)] = base_b
    thetas[:, joint.field_columns(0)] = base_a
    got = joint.log_posterior_batch(thetas)
    prior = joint.log_priors_batch(thetas)
    field_a, field_b = oracle_field(fa), oracle_field(fb)
    for i, t in enumerate(thetas):
        ta, tb = joint.field_theta(t, 0)[0], joint.field_theta(t, 1)[0]
        want = (contract_evaluate(own_a, field_a, ta)[0] + contract_evaluate(own_b, field_b, tb)[0]) + prior[i]
        assert np.isfinite(want) and abs(got[i] - want) <= 1e-9 * abs(want), (i, got[i], want)
    assert joint.log_posterior_batch(thetas[1:2])[0] == got[1]
    joint.close()
    own_a.close()
    own_b.close()


def test_f32_storage_and_context_group():
    fld = make_field(64, 64, seed=14)
    field = oracle_field(fld)
    f32 = build(fld, BOTH, storage='f32')
    thetas = trl._both_start(fld, f32, 3, 15, scale=0.02)
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
    grp.close()
    model.close()


def test_the_library_refuses_what_the_header_says_and_removal_gives_the_bits_back():
    from psfmc_amd.engine import NativeError
    fld = make_field(64, 64, seed=15)
    model = build(fld, [(Moffat, MEAN), (Sersic, dict(boxiness=0.3)), (Sersic, {})], max_walkers=4)
    same = build(fld, [(Moffat, {}), (Sersic, dict(boxiness=0.3)), (Sersic, {})], max_walkers=4)
    t = vector(model, fld, dict(named(2, 'Moffat', beta=2.5, fwhm=2.0, fwhm_b=1.5, mag=18.5, xy=(32.3, 30.8)),
                                **dict(named(3, 'Sersic', index=1.5, mag=18.7, reff=5.0, reff_b=3.0, xy=(28.4, 34.1)),
                                       **named(4, 'Sersic', index=2.0, mag=19.0, reff=4.0, reff_b=2.0, xy=(35.6, 33.3)))))[None]
    eng = model.engine
    first = model.log_posterior_batch(t)[0]
    want = same.log_posterior_batch(t)[0]
    assert np.isfinite(first) and np.isfinite(want) and first != want
    with pytest.raises(NativeError, match='general'):
        eng.set_general_mean([1, 0, 1])                                # the third slot is a plain Sersic
    with pytest.raises(NativeError, match='n_sersic'):
        eng.set_general_mean([1, 0])
    assert model.log_posterior_batch(t)[0] == first                    # refused: nothing changed
    eng.set_general_mean([1, 1, 0])                                    # a general Sersic may take the flag
    both = model.log_posterior_batch(t)[0]
    assert np.isfinite(both) and both != first
    eng.set_general_mean([0, 0, 0])                                    # all-zero flags remove them: today's bits
    assert model.log_posterior_batch(t)[0] == want
    eng.set_general_mean([1, 0, 0])
    assert model.log_posterior_batch(t)[0] == first
    model._register_layout(eng)                                        # a new layout drops and re-registers
    assert model.log_posterior_batch(t)[0] == first
    same._register_layout(model.engine)                                # the model without the keyword: the flags are gone
    assert model.log_posterior_batch(t)[0] == want
    model.close()
    same.close()
    plain = build(fld, [(Sersic, {})], max_walkers=4)
    with pytest.raises(NativeError, match='aux layout'):
        plain.engine.set_general_mean([1])
    plain.engine.set_general_mean([0])                                 # nothing registered, nothing to remove
    plain.close()
    integ = build(fld, [(Sersic, dict(integrate=True))], max_walkers=4, slope=True)          # (a tilted sky: an aux layout)
    with pytest.raises(NativeError, match='integrated'):
        integ.engine.set_general_mean([1])
    integ.close()


def _law_reference():
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(64, 64, seed=7)
    model = build(fld, trl.LEAN, max_walkers=32, ps_free=False)
    p0 = trl._lean_start(fld, model, 32, 2)
    lp = model.log_posterior_batch(p0)
    s = DeviceEnsembleSampler(32, model, block=5)
    s.random_state = np.random.RandomState(3).get_state()
    list(s.sample(p0, iterations=20))
    out = lp, s.chain.copy(), s.lnprobability.copy()
    model.close()
    return out


def test_models_without_the_keyword_are_untouched_by_mean_contexts():
    """Plain, boxiness-only, Fourier, spiral and law models: bit-identical log-posteriors and 20-iteration device chains
    before and after contexts with mean components lived and died in the process."""
    refs = lambda: (tgg._plain_reference()[2], tgf._boxiness_reference(), tgs._fourier_reference(),
                    trl._spiral_reference(), _law_reference())
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


def test_a_planted_narrow_moffat_is_recovered():
    """sci = the oracle's convolution of sky + point source + the 32 x 32 sub-pixel mean of a Moffat of fwhm 1.6 / 1.3
    (2.5 mag fainter than the point source beside it: the wings a PSF mismatch leaves) plus the helper's fixed-seed
    noise.  With `pixel_mean=True` the central 95 % of the last 100 of 200 iterations of a 32-walker device chain
    holds the planted fwhm."""
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(64, 64, seed=16)
    noise = fld['sci'].astype(np.float64) - 0.05
    comps = [(Moffat, dict(fwhm_b=1.3, beta=2.5, **MEAN))]
    truth = named(2, 'Moffat', fwhm=1.6, mag=21.5, xy=(33.9, 30.6))
    first = build(fld, comps, max_walkers=1, ps_free=False)
    planted = vector(first, fld, truth)
    raw = contract_raw(first, planted)
    comp = [c for c in first.components if isinstance(c, Moffat)][0]
    args =('moffat', comp.derived_row(fld['mag_zp']), (2.5, 0.0), 0.0, [], None)
    raw += tm.truth_of(*args) - Sersic.general_mean_image(*(args + (raw.shape,)))
    conv = orc.convolve(raw, oracle_field(fld).psf_spec[0])
    first.close()
    model = build(dict(fld, sci=(conv + noise).astype(np.float32)), comps, max_walkers=32, ps_free=False)
    fw = column(model, '2_Moffat_fwhm')
    off = planted.copy()
    off[fw] = 2.2
    lp = model.log_posterior_batch(np.array([planted, off]))
    print('log-posterior at the planted vector %.2f, with fwhm = 2.2: %.2f' % (lp[0], lp[1]))
    assert np.isfinite(lp[1]) and lp[0] > lp[1]
    start = planted.copy()
    start[fw] = 1.7
    scale = np.full(len(start), 1e-2)
    scale[0], scale[fw] = 1e-3, 0.05
    p0 = start + np.random.RandomState(4).normal(size=(32, len(start))) * scale
    s = DeviceEnsembleSampler(32, model, block=50)
    s.random_state = np.random.RandomState(5).get_state()
    list(s.sample(p0, iterations=200))
    lo, med, hi = np.percentile(s.chain[:, -100:, fw], [2.5, 50.0, 97.5])
    print('fwhm of the last 100 iterations: 2.5 %% %.3f, median %.3f, 97.5 %% %.3f' % (lo, med, hi))
    assert lo <= 1.6 <= hi
    model.close()
