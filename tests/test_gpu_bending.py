"""Bending modes of general components on the device, held to the numpy definition (`Sersic.bent_image`,
`Sersic.general_mean_image(..., bending)`) composed with the oracle's point source, convolution and likelihood: raw
images per pixel on both back ends, from raw vectors and from rows with auxiliary rows; neutrality towards contexts and
models without the keyword, removal, batch independence and the support, the samplers with and without a DE move, the
tempered sampler, sharded half-steps, field sets, joint fits, the Fisher entry, f32 storage, the library's refusals and a
planted banana.  Field, model and contract helpers are those of tests/test_gpu_radial_laws.py,
tests/test_gpu_general_components.py and tests/test_gpu_truncation.py."""
import numpy as np
import pytest

import test_gpu_fourier_modes as tgf
import test_gpu_general_components as tgg
import test_gpu_radial_laws as tgr
import test_gpu_spiral_arms as tgs
import test_gpu_truncation as tgt
from extra_contract import EDGE_MARGIN, law_error
from test_gpu_general_components import RAW_BOUND, contract_evaluate, make_field, oracle_field
from test_gpu_radial_laws import U, build, column, named, vector
from test_gpu_truncation import BOTH, DRESS, DRESS_VALUES, IN, OUT, cut, radii
from psfmc_amd.ModelComponents import Ferrer, Moffat, Sersic

pytestmark = pytest.mark.gpu

BD = lambda: U(-3.0, 3.0)                # a bending amplitude
AMPS = {1: (0.2, -0.1), 2: (0.3, -0.25), 3: (-0.1, 0.15), 4: (0.05, -0.05)}     # per mode: walker 0, walker 1


def bent(modes):
    return {m: BD() for m in modes}


def amps(modes, i):
    return {'bend%d' % m: AMPS[m][i] for m in modes}


def ferrer_state(model):
    """(smallest Sigma_0, smallest |1 - x| over the image's pixels) of the model's Ferrer components, bent as they
    are, at the model's current values: `extra_contract.ferrer_state` with the bending in the radius."""
    sigma0, margin = [], np.inf
    for comp in model.components:
        if isinstance(comp, Ferrer):
            get = lambda k: getattr(comp, k)
            row = comp.derived_row(model.config.mag_zeropoint)
            box = float(np.ravel(comp.boxiness)[0]) if comp.has_boxiness else 0.0
            a, ph = comp._fourier_values(get) if comp.has_fourier else ((), ())
            modes = list(zip(comp.fourier_modes, a, ph))
            spiral = comp._spiral_values(get) if comp.has_spiral else None
            pars = comp._radial_values(get)
            rho2, centre = Sersic.radial_rho2(row, box, modes, spiral, model.config.obs_data.shape, comp.bending_list())
            with np.errstate(all='ignore'):
                x = np.where(centre, 0.0, rho2 ** (0.5 * (2.0 - pars[1])))
            sigma0.append(Sersic.radial_central('ferrer', row, pars, box, modes, spiral))
            margin = min(margin, float(np.min(np.abs(1.0 - x))))
    return (min(sigma0) if sigma0 else 0.0), margin


# (bending modes, dress, truncated sides or None, pixel_mean) of the Sersic, the Moffat and the Ferrer of each model:
# every law with every dress, with and without a truncation, the mode sets {2}, {1, 3}, {4} and {1, 2, 3, 4} on every
# law, pixel means of a Sersic law and of a Moffat
PLAN = [(((2,), 0, None, False), ((1, 3), 1, OUT, False), ((4,), 2, None, False)),
        (((1, 2, 3, 4), 1, BOTH, False), ((2,), 2, None, False), ((1, 3), 3, IN, False)),
        (((4,), 2, None, True), ((1, 2, 3, 4), 3, IN, True), ((2,), 0, OUT, False)),
        (((1, 3), 3, None, False), ((4,), 0, None, False), ((1, 2, 3, 4), 1, None, False))]


def contract_sets(fld):
    """[(components, [{name: value}])]: four models of a Sersic, a Moffat and a Ferrer (`PLAN`), two walkers each.
    Amplitudes of magnitude 0.05 ... 0.4 (`AMPS`: walker 1's of the opposite sign), r_a / r_b <= 3; the Sersic's (r_a,
    r_b, n) = (14, 9, 2.5) and (8, 3, 4).  Walker 1: the Sersic's centre outside the image, the Moffat's on a pixel
    centre with its axis along the pixel grid."""
    ny, nx = fld['shape']
    cx, cy = nx // 2, ny // 2
    small = 0.31 * min(ny, nx)
    sets = []
    for plan in PLAN:
        comps, cases = [], [{}, {}]
        for idx, (cls, (modes, d, sides, mean)) in enumerate(zip((Sersic, Moffat, Ferrer), plan)):
            kw = dict(angle='free', bending=bent(modes), **DRESS[d])
            if sides:
                kw['truncation'] = cut(sides)
            if mean:
                kw['pixel_mean'] = True
            comps.append((cls, kw))
            for i in range(2):
                if cls is Sersic:
                    v = dict(angle=-20.0 + 50 * i, index=(2.5, 4.0)[i], mag=18.5, reff=(14.0, 8.0)[i], reff_b=(9.0, 3.0)[i],
                             xy=((cx + 3.2, cy - 1.1), (-3.6, cy + 0.4))[i])
                    ramps = (((0.5, 3.0), (0.0, 12.0))[i], ((6.0, 14.0), (6.0, 40.0))[i])
                elif cls is Moffat:
                    v = dict(angle=(110.0, 90.0)[i], beta=(2.5, 1.2)[i], fwhm=(6.0, 9.0)[i], fwhm_b=(4.0, 3.0)[i], mag=18.8,
                             xy=((cx + 0.25, cy + 0.4), (float(cx - 3), float(cy + 2)))[i])
                    ramps = (((0.5, 3.0), (4.0, 12.0))[i], ((3.5, 9.0), (6.0, 16.0))[i])
                else:
                    v = dict(alpha=(2.0, 0.5)[i], angle=30.0 + 40 * i, beta=(0.0, 1.5)[i], mag=18.0,
                             r_out=(small, 1.3 * small)[i], r_out_b=(0.45 * small, 0.9 * small)[i],
                             xy=((cx - 1.4, cy + 0.7), (cx + 0.37, cy - 0.21))[i])
                    ramps = (((3.0, 7.0), (5.0, 5.5))[i], ((9.0, 15.0), (11.0, 11.5))[i])
                v.update(DRESS_VALUES[d])
                v.update(amps(modes, i))
                if sides:
                    v.update(radii(sides, *ramps))
                cases[i].update(named(2 + idx, cls.__name__, **v))
        sets.append((comps, cases))
    return sets


_CONTRACT = {}


def contract_of(shape):
    """The field of a shape and, per model of `contract_sets`, the parameter vectors with the contract's
    (log-likelihood, images, Sigma_0) -- computed once per shape on the host, shared by the back ends, left unchanged."""
    if shape not in _CONTRACT:
        fld = make_field(*shape, seed=1)
        field = oracle_field(fld)
        out = []
        for n_set, (comps, cases) in enumerate(contract_sets(fld)):
            model = build(fld, comps, backend='hipfft', degrees=True, slope=(n_set % 2 == 1), max_walkers=2)
            thetas = np.array([vector(model, fld, v, adu=0.05 + 0.002 * i) for i, v in enumerate(cases)])
            want = []
            for i, t in enumerate(thetas):                             # the host first: the condition on the inputs
                ll, imgs = contract_evaluate(model, field, t)
                sigma0, margin = ferrer_state(model)
                assert margin >= EDGE_MARGIN, (shape, n_set, i, margin)
                want.append((ll, imgs, sigma0))
            out.append((comps, thetas, want))
        _CONTRACT[shape] = (fld, out)
    return _CONTRACT[shape]


@pytest.mark.parametrize('backend,shape', [('fused', (64, 64)), ('fused', (70, 66)), ('fused', (64, 320)),
                                           ('hipfft', (64, 64)), ('hipfft', (70, 66))],
                         ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_device_against_the_contract(backend, shape):
    """Raw image per pixel by `law_error` at RAW_BOUND (1e-11; the float64 definition is within 8.2e-14 of its
    long-double evaluation on these shapes and amplitudes: two orders of room; MEASURED worst: DESIGN.md section 32);
    the five images to 1e-12 of the image maximum; the log-posterior through raw vectors and the log-likelihood through
    the host path's rows and auxiliary rows against the contract (1e-9).  70 x 66: a second 64-lane chunk in every
    row, an embedded image; 64 x 320: five chunks, the power-table forward form."""
    fld, sets = contract_of(shape)
    worst = 0.0
    for n_set, (comps, thetas, want_all) in enumerate(sets):
        model = build(fld, comps, backend=backend, degrees=True, slope=(n_set % 2 == 1))
        assert model.aux_rows(np.zeros((1, model.num_params))).shape[1] == 2 + 29 * 3
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


# Sky + PS (a fixed position) + an exponential banana with 8 free parameters: adu, the point source's mag, the
# Sersic's bend2, mag, reff, reff_b, x, y
BANANA = [(Sersic, dict(index=1.0, bending={2: U(-1.0, 2.0)}))]
BANANA_TRUTH = dict(mag=17.5, reff=10.0, reff_b=3.0, xy=(32.3, 30.8), bend2=0.25)
STRAIGHT = [(Sersic, dict(index=1.0, bending={2: 0.0}))]


def _banana_start(fld, model, n_w, seed, scale=1e-2):
    base = vector(model, fld, named(2, 'Sersic', **BANANA_TRUTH), ps_mag=19.0)
    return base + np.random.RandomState(seed).normal(size=(n_w, len(base))) * scale


FULL = [(Sersic, dict(angle='free', boxiness='free', bending=bent((1, 3))))]


def _full(fld, model, n_w, seed, scale=0.02, idx=2):
    ny, nx = fld['shape']
    base = vector(model, fld, named(idx, 'Sersic', angle=30.0, boxiness=0.3, index=1.2, mag=17.8, reff=10.0, reff_b=6.5,
                                    xy=(nx / 2 + 0.31, ny / 2 - 0.27), bend1=0.15, bend3=-0.1))
    return base + np.random.RandomState(seed).normal(size=(n_w, len(base))) * scale


def test_zero_amplitudes_equal_the_component_without_the_keyword():
    """A component with zero-amplitude bending against the same without the keyword: log-posteriors EQUAL -- a boxy
    Sersic with modes, a truncated Moffat and a wound Ferrer, each in its own pair of contexts."""
    fld = make_field(64, 64, seed=17)
    pairs = [(Sersic, dict(boxiness='free', fourier=tgt.TWO),
              dict(boxiness=0.3, f2_amp=0.2, f2_phase=30.0, f3_amp=-0.15, index=1.5, mag=18.0, reff=8.0, reff_b=5.0)),
             (Moffat, dict(boxiness='free', truncation={'inner': (2.0, 6.0), 'outer': (8.0, 14.0)}),
              dict(beta=2.5, boxiness=0.3, fwhm=9.0, fwhm_b=6.5, mag=18.5)),
             (Ferrer, dict(boxiness='free', spiral=dict(r_in=2.0, r_out=10.0, winding=150.0)),
              dict(alpha=1.5, beta=0.5, boxiness=-0.4, mag=18.3, r_out=18.3, r_out_b=7.1))]
    for cls, kw, vals in pairs:
        zero = build(fld, [(cls, dict(bending={2: 0.0, 3: 0.0}, **kw))], max_walkers=4)
        plain = build(fld, [(cls, kw)], max_walkers=4)
        assert zero.param_names == plain.param_names and zero.sersic_bending_masks == [0b110]
        t = np.array([vector(plain, fld, named(2, cls.__name__, xy=(32.3 + i, 30.8), **vals)) for i in range(3)])
        got, want = zero.log_posterior_batch(t), plain.log_posterior_batch(t)
        print('%s: zero amplitudes %r, without the keyword %r' % (cls.__name__, got, want))
        assert np.all(np.isfinite(want)) and np.array_equal(got, want), cls.__name__
        zero.close()
        plain.close()


def _chain_reference(comps, start):
    """(log-posteriors, 20-iteration device chain, its log-probabilities) of a 32-walker model of `comps`."""
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(64, 64, seed=7)
    model = build(fld, comps, max_walkers=32, ps_free=False)
    p0 = start(fld, model, 32, 2)
    lp = model.log_posterior_batch(p0)
    s = DeviceEnsembleSampler(32, model, block=5)
    s.random_state = np.random.RandomState(3).get_state()
    list(s.sample(p0, iterations=20))
    out = lp, s.chain.copy(), s.lnprobability.copy()
    assert s.naccepted.sum() > 0
    model.close()
    return out


def _law_reference():
    """... of a Moffat + Ferrer model (a context with laws, none with truncations or bending)."""
    return _chain_reference(tgr.LEAN, tgr._lean_start)


def _truncation_reference():
    """... of a truncated model (a context with truncations, none with bending)."""
    return _chain_reference(tgt.RING, tgt._ring_start)


def test_models_without_bending_are_untouched_by_bending_contexts():
    """Plain, boxiness-only, Fourier, spiral, radial-law and truncated models: bit-identical log-posteriors and
    20-iteration device chains (every one of the six) before and after contexts with bending lived and died in the
    process."""
    refs = lambda: (tgg._plain_reference()[2], tgf._boxiness_reference(), tgs._fourier_reference(),
                    tgr._spiral_reference(), _law_reference(), _truncation_reference())
    before = refs()
    assert all(len(r) == 3 and r[1].shape[1] == 20 for r in before[-3:])       # the chains are there
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


def test_all_zero_masks_remove_the_block():
    fld = make_field(64, 64, seed=17)
    bnt = build(fld, [(Moffat, dict(boxiness='free', bending={2: 0.3, 3: -0.1}))], max_walkers=4)
    plain = build(fld, [(Moffat, dict(boxiness='free'))], max_walkers=4)
    assert bnt.param_names == plain.param_names
    t = vector(plain, fld, named(2, 'Moffat', beta=2.5, boxiness=0.3, fwhm=9.0, fwhm_b=6.5, mag=18.5, xy=(32.3, 30.8)))[None]
    want, first = plain.log_posterior_batch(t)[0], bnt.log_posterior_batch(t)[0]
    assert int(bnt.engine.get_option('aux_stride')) == 2 + 29
    bnt.engine.set_bending_layout([0], [-1] * 4, [0.0] * 4)
    again = bnt.log_posterior_batch(t)[0]
    print('bent %.6f, the slot without its mask %.6f, the plain Moffat %.6f' % (first, again, want))
    assert np.isfinite(first) and first != want and again == want
    bnt.close()
    plain.close()


def test_batch_independence_and_the_support():
    """A walker's log-posterior bits are the same alone, in a batch of 64 and in permuted order; a NaN or inf
    amplitude is -inf from raw vectors on the device and on the host, leaves the other walkers' bits unchanged, and is
    NaN through a row-based call (no writable flags there)."""
    fld = make_field(64, 64, seed=4)
    comps = [(Sersic, dict(angle='free', bending=bent((1, 2, 3, 4)))),
             (Ferrer, dict(angle='free', bending=bent((2,)), truncation=cut(OUT)))]
    model = build(fld, comps, max_walkers=64)
    base = vector(model, fld, dict(
        named(2, 'Sersic', angle=30.0, index=1.5, mag=18.0, reff=9.0, reff_b=6.0, xy=(32.3, 30.8), bend1=0.1, bend2=0.3,
              bend3=-0.1, bend4=0.05),
        **named(3, 'Ferrer', alpha=1.5, angle=70.0, beta=0.5, mag=18.3, r_out=18.3, r_out_b=7.1, xy=(30.31, 33.73),
                bend2=-0.2, trunc_out_lo=8.0, trunc_out_hi=13.0)))
    thetas = base + np.random.RandomState(5).normal(size=(64, len(base))) * 1e-3
    full = model.log_posterior_batch(thetas)
    assert np.all(np.isfinite(full))
    for i in (0, 7, 63):
        assert model.log_posterior_batch(thetas[i:i + 1])[0] == full[i]
    perm = np.random.RandomState(6).permutation(64)
    assert np.array_equal(model.log_posterior_batch(thetas[perm]), full[perm])
    bad = [('2_Sersic_bend1', np.nan), ('2_Sersic_bend4', np.inf), ('2_Sersic_bend2', -np.inf), ('3_Ferrer_bend2', np.nan),
           ('3_Ferrer_bend2', np.inf)]
    where = [1 + 2 * k for k in range(len(bad))]
    mixed = thetas.copy()
    for k, (name, val) in zip(where, bad):
        mixed[k, column(model, name)] = val
    got = model.log_posterior_batch(mixed)
    keep = np.ones(64, dtype=bool)
    keep[where] = False
    for k, what in zip(where, bad):
        assert got[k] == -np.inf, what
    assert np.array_equal(got[keep], full[keep])
    with np.errstate(all='ignore'):
        assert np.all(model.log_posterior_batch_host(mixed)[where] == -np.inf)
        rows = model.engine.loglike(model.derived_rows(mixed[where]), aux=model.aux_rows(mixed[where]))
    for what, r in zip(bad, rows):
        assert np.isnan(r), what
    assert np.isfinite(model.engine.loglike(model.derived_rows(thetas[:1]), aux=model.aux_rows(thetas[:1]))[0])
    model.close()


@pytest.mark.parametrize('de', [False, True], ids=['stretch', 'de'])
@pytest.mark.parametrize('n_w', [22, 64])
def test_device_sampler_equals_the_host_sampler(n_w, de):
    """The device-resident chain equals the host loop's fed the device's own log-posteriors, bit for bit (22 walkers:
    the whole-iteration route of small ensembles; 64: half-steps), with the stretch move and with `DEMove()`."""
    from psfmc_amd.sampler import DEMove, DeviceEnsembleSampler, EnsembleSampler
    fld = make_field(64, 64, seed=7)
    model = build(fld, BANANA, max_walkers=n_w, ps_free=False)
    assert model.num_params == 8
    p0 = _banana_start(fld, model, n_w, 2)
    kw = dict(moves=DEMove()) if de else {}
    host = EnsembleSampler(n_w, model.num_params, batch_lnpostfn=model.log_posterior_batch, **kw)
    dev = DeviceEnsembleSampler(n_w, model, block=7, **kw)
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
    model = build(fld, BANANA, max_walkers=3 * 18, ps_free=False)
    betas = default_betas(3, 50.0)
    p0 = _banana_start(fld, model, 3 * 18, 3).reshape(3, 18, -1)
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


def test_sharded_half_steps_equal_one_context():
    """Two ranks inside one process (tests/shard_driver.py), 20 walkers on an embedded 70 x 66 field: a wrong walker
    offset of the bending constants would evaluate a walker with another walker's amplitudes.  Every rank's chain is
    bit-identical to one `DeviceEnsembleSampler`'s on one more context, and gathered log-posteriors equal the
    contract's to 1e-9 |ll|."""
    import shard_driver as sd
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(70, 66, seed=18)
    field = oracle_field(fld)
    ranks, n_w, seed = 2, 20, 7
    models = [build(fld, BANANA, max_walkers=n_w, ps_free=False) for _ in range(ranks + 1)]
    single, models = models[-1], models[:-1]
    p0 = _banana_start(fld, single, n_w, seed, scale=0.05)
    draws = sd.draw(sd.random_state(seed), sd.N_ITER, n_w, single.num_params)
    lnp0 = models[0].log_posterior_batch(p0)
    samp = DeviceEnsembleSampler(n_w, single)
    samp.random_state = sd.random_state(seed)
    list(samp.sample(p0, iterations=sd.N_ITER))
    res = sd.run_blocks(models, p0, lnp0, draws)
    for r in range(ranks):
        assert np.array_equal(res['chain'][r], samp.chain), r
        assert np.array_equal(res['lnchain'][r], samp.lnprobability), r
    q, acc = sd.replay(p0, res['chain'][0], draws[0], draws[2])
    assert acc.sum() > 0 and np.all(np.isfinite(res['gathered']))
    for h in range(2):
        for j in (0, 9):                                               # a walker of either rank's block
            want = contract_evaluate(single, field, q[0, h, j])[0] + single.log_priors_batch(q[0, h, j][None])[0]
            assert abs(res['gathered'][0, h, j] - want) <= 1e-9 * abs(want), (h, j)
    for m in models + [single]:
        m.close()


def test_field_set_of_a_bent_a_truncated_and_a_plain_field():
    """62 x 66 bent, 70 x 64 truncated but not bent, 64 x 64 PLAIN -- a Sersic with no keyword: no aux layout and no
    general flag, in a context whose walkers carry 2 + 29 auxiliary entries -- with as many free parameters each (the
    index of the first two is fixed, one amplitude and one radius are free).  Every field equals its own model BIT FOR
    BIT: the own model in a set of the same three shapes, hence the same transform, whose other two fields are plain
    (for the plain field a context that never saw an aux layout).  Against the own one-field context: within 1e-12,
    and equal where that context happens to have the set's transform.  A field alone in a call equals itself in the
    full call."""
    from psfmc_amd.models import FieldSet
    shapes = [(62, 66), (70, 64), (64, 64)]
    flds = [make_field(ny, nx, seed=10 + i) for i, (ny, nx) in enumerate(shapes)]
    plain = [(Sersic, dict(angle='free'))]
    specs = [[(Sersic, dict(angle='free', index=1.5, bending={1: BD(), 3: -0.1}))],
             [(Sersic, dict(angle='free', index=1.5, truncation={'inner': (tgt.TR(), 9.0), 'outer': (14.0, 30.0)}))],
             plain]
    extra = [dict(bend1=0.15), dict(trunc_in_lo=2.0), dict(index=1.5)]
    make_set = lambda which: FieldSet([build(f, s, max_walkers=1) for f, s in zip(flds, which)], max_walkers=16)
    fs = make_set(specs)
    own = [build(f, s, max_walkers=8) for f, s in zip(flds, specs)]
    assert [any(m.sersic_bending_masks) for m in own] == [True, False, False]
    assert [any(m.sersic_truncation_flags) for m in own] == [False, True, False]
    assert [m.has_aux for m in own] == [True, True, False] and len({m.num_params for m in own}) == 1
    assert int(fs.context.get_option('aux_stride')) == 2 + 29
    thetas = []
    for f, m, more in zip(flds, own, extra):
        ny, nx = f['shape']
        thetas.append(np.array([vector(m, f, named(2, 'Sersic', angle=30.0 + 10 * i, mag=18.0, reff=8.0, reff_b=4.0,
                                                   xy=(nx / 2 + 0.31 + i, ny / 2 - 0.27), **more))
                                for i in range(4)]))
    got = fs.log_posterior_batch(thetas)
    raws = [fs.models[f].sample_images(thetas[f][:2], ('raw_model',))['raw_model'] for f in range(3)]
    transform = fs.context.get_option('transform_ny'), fs.context.get_option('transform_nx')
    for f in range(3):
        alone = [None, None, None]
        alone[f] = thetas[f]
        assert np.array_equal(fs.log_posterior_batch(alone)[f], got[f]), f
        mine = own[f].log_posterior_batch(thetas[f])
        assert np.all(np.isfinite(got[f])) and np.abs(got[f] - mine).max() <= 1e-12 * np.abs(mine).max(), f
        if (own[f].engine.get_option('transform_ny'), own[f].engine.get_option('transform_nx')) == transform:
            assert np.array_equal(got[f], mine), f
    fs.close()
    for m in own:
        m.close()
    # bit for bit, every field: its own model at the set's transform, beside plain fields
    for f in range(3):
        ref = make_set([specs[k] if k == f else plain for k in range(3)])
        assert (ref.context.get_option('transform_ny'), ref.context.get_option('transform_nx')) == transform
        if f == 2:
            assert int(ref.context.get_option('aux_stride')) == 0          # a context that never saw an aux layout
        alone = [None, None, None]
        alone[f] = thetas[f]
        assert np.array_equal(ref.log_posterior_batch(alone)[f], got[f]), f
        assert np.array_equal(ref.models[f].sample_images(thetas[f][:2], ('raw_model',))['raw_model'], raws[f]), f
        ref.close()


def test_joint_model_keeps_bend2_per_field():
    from psfmc_amd import JointModel
    fa, fb = make_field(64, 64, seed=12), make_field(70, 66, seed=13)
    spec = [(Sersic, dict(angle='free', bending=bent((2, 3))))]
    make = lambda f: build(f, spec, max_walkers=1, extent=70)
    joint = JointModel([make(fa), make(fb)], per_field=['2_Sersic_bend2', '1_PointSource_xy', '2_Sersic_xy'], max_walkers=16)
    names = joint.param_names
    assert names.count('2_Sersic_bend3') == 1 and '2_Sersic_bend2_f0' in names and '2_Sersic_bend2_f1' in names
    own_a, own_b = make(fa), make(fb)

    def start(f, m, b2):
        ny, nx = f['shape']
        base = vector(m, f, named(2, 'Sersic', angle=30.0, index=1.2, mag=17.8, reff=10.0, reff_b=4.0,
                                  xy=(nx / 2 + 0.31, ny / 2 - 0.27), bend2=b2, bend3=-0.1))
        return base + np.random.RandomState(14).normal(size=(3, len(base))) * 0.01
    base_a, base_b = start(fa, own_a, 0.25), start(fb, own_b, -0.2)
    thetas = np.zeros((3, joint.num_params))
    thetas[:, joint.field_columns(1)] = base_b
    thetas[:, joint.field_columns(0)] = base_a
    got = joint.log_posterior_batch(thetas)
    prior = joint.log_priors_batch(thetas)
    field_a, field_b = oracle_field(fa), oracle_field(fb)
    for i, t in enumerate(thetas):
        ta, tb = joint.field_theta(t, 0)[0], joint.field_theta(t, 1)[0]
        assert ta[column(own_a, '2_Sersic_bend3')] == tb[column(own_b, '2_Sersic_bend3')]
        assert abs(ta[column(own_a, '2_Sersic_bend2')] - tb[column(own_b, '2_Sersic_bend2')] - 0.45) < 0.1
        want = (contract_evaluate(own_a, field_a, ta)[0] + contract_evaluate(own_b, field_b, tb)[0]) + prior[i]
        assert np.isfinite(want) and abs(got[i] - want) <= 1e-9 * abs(want), (i, got[i], want)
    assert joint.log_posterior_batch(thetas[1:2])[0] == got[1]
    bad = thetas[:1].copy()
    bad[0, joint.field_columns(1)[column(own_b, '2_Sersic_bend2')]] = np.nan
    assert joint.log_posterior_batch(bad)[0] == -np.inf
    joint.close()
    own_a.close()
    own_b.close()


@pytest.mark.parametrize('backend', ['fused', 'hipfft'])
def test_fisher_of_a_bent_model_on_its_own_images(backend):
    """`model.fisher` within `mode_helpers.fisher_rounding_bound` of the long-double definition on the model's own
    images of the stencil's vectors."""
    from psfmc_amd import mode
    from test_gpu_fisher import held_to_own_images
    fld = make_field(64, 64, seed=19)
    model = build(fld, FULL, backend=backend, max_walkers=64, ps_free=False)
    theta = _full(fld, model, 1, 20, scale=0.0)[0]
    assert model.aux_rows(theta[None]).shape[1] == 2 + 29
    out = model.fisher(theta)
    columns = mode.default_columns(model)
    step = mode.default_steps(model, theta, columns)
    assert column(model, '2_Sersic_bend1') in columns and column(model, '2_Sersic_bend3') in columns
    vecs = mode.stencil(theta, step, columns)[0]
    want_f, _ = held_to_own_images(model, vecs, out, 0.5 / step[0], 'bent %s' % backend)
    assert np.linalg.eigvalsh(want_f).min() > 0
    model.close()


def test_f32_storage_and_context_group():
    """storage='f32' within its documented 2e-6; a ContextGroup on one device equals the plain context."""
    fld = make_field(64, 64, seed=14)
    field = oracle_field(fld)
    f32 = build(fld, FULL, storage='f32')
    thetas = _full(fld, f32, 3, 15)
    ll = f32.log_likelihood_batch(thetas)
    lp32 = f32.log_posterior_batch(thetas)
    prior = f32.log_priors_batch(thetas)
    for i, t in enumerate(thetas):
        want_ll, _ = contract_evaluate(f32, field, t)
        assert abs(ll[i] - want_ll) <= 2e-6 * abs(want_ll) and abs(lp32[i] - want_ll - prior[i]) <= 2e-6 * abs(want_ll)
    f32.close()
    model = build(fld, FULL)
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
    zeros = [0.0] * 12
    with pytest.raises(NativeError, match='bending mask 0x10 names a mode outside 1 ... 4'):
        eng.set_bending_layout([16, 0, 0], [-1] * 12, zeros)
    with pytest.raises(NativeError, match='names a mode outside'):
        eng.set_bending_layout([-1, 0, 0], [-1] * 12, zeros)
    with pytest.raises(NativeError, match='has bending modes but is not flagged general'):
        eng.set_bending_layout([1, 0, 2], [-1] * 12, zeros)                    # the third slot is a plain Sersic
    with pytest.raises(NativeError, match='n_sersic=2, the context has 3'):
        eng.set_bending_layout([1, 0], [-1] * 8, zeros[:8])
    with pytest.raises(NativeError, match='column'):
        eng.set_bending_layout([1, 0, 0], [model.num_params] + [-1] * 11, zeros)
    assert model.log_posterior_batch(t)[0] == before                          # nothing changed
    eng.set_bending_layout([0b0110, 0b1000, 0], [-1] * 12, [0.0, 0.3, -0.1, 0.0, 0.0, 0.0, 0.0, 0.05, 0.0, 0.0, 0.0, 0.0])
    bent_lp = model.log_posterior_batch(t)[0]
    assert np.isfinite(bent_lp) and bent_lp != before and int(eng.get_option('aux_stride')) == 2 + 29 * 3
    eng.set_general_mean([False, False, False])                                # keeps the masks
    assert model.log_posterior_batch(t)[0] == bent_lp
    eng.set_truncation_layout([0, 0, 0], [-1] * 12, [0.0, 1.0] * 6)            # an earlier block's layout drops the block
    assert model.log_posterior_batch(t)[0] == before
    eng.set_bending_layout([0b0110, 0b1000, 0], [-1] * 12, [0.0, 0.3, -0.1, 0.0, 0.0, 0.0, 0.0, 0.05, 0.0, 0.0, 0.0, 0.0])
    assert model.log_posterior_batch(t)[0] == bent_lp
    eng.set_bending_layout([0, 0, 0], [-1] * 12, zeros)                        # all-zero masks remove it
    assert model.log_posterior_batch(t)[0] == before
    model.close()
    plain = build(fld, [(Sersic, {})], max_walkers=4)
    with pytest.raises(NativeError, match='has no aux layout'):
        plain.engine.set_bending_layout([1], [-1] * 4, zeros[:4])
    plain.close()
    integ = build(fld, [(Sersic, dict(integrate=True))], max_walkers=4, slope=True)          # (a tilted sky: an aux layout)
    with pytest.raises(NativeError, match='pixel-integrated: bending and integrate exclude each other'):
        integ.engine.set_bending_layout([2], [-1] * 4, zeros[:4])
    integ.close()


def test_a_planted_banana_is_recovered():
    """sci = the contract's convolved image of an exponential banana (reff 10 / 3, a_2 = 0.25) plus the helper's
    fixed-seed noise.  A 64-walker, 200-iteration device chain started in a 1e-2 ball about the truth: the truth of
    bend2 lies inside the 2.5 ... 97.5 % interval of the last 100 iterations.  The same data fitted with a_2 fixed at 0
    (one free parameter fewer) has a maximum log-posterior lower by more than the number of free parameters."""
    from psfmc_amd.sampler import DeviceEnsembleSampler
    fld = make_field(64, 64, seed=16)
    noise = fld['sci'].astype(np.float64) - 0.05
    first = build(fld, BANANA, max_walkers=1, ps_free=False)
    planted = vector(first, fld, named(2, 'Sersic', **BANANA_TRUTH))
    conv = contract_evaluate(first, oracle_field(fld), planted)[1]['convolved_model']
    first.close()
    data = dict(fld, sci=(conv + noise).astype(np.float32))
    best = []
    for spec, truth in ((BANANA, BANANA_TRUTH), (STRAIGHT, {k: v for k, v in BANANA_TRUTH.items() if k != 'bend2'})):
        model = build(data, spec, max_walkers=64, ps_free=False)
        base = vector(model, data, named(2, 'Sersic', **truth))
        p0 = base + np.random.RandomState(4).normal(size=(64, len(base))) * 1e-2
        s = DeviceEnsembleSampler(64, model, block=50)
        s.random_state = np.random.RandomState(5).get_state()
        list(s.sample(p0, iterations=200))
        best.append(np.max(s.lnprobability))
        if spec is BANANA:
            col = column(model, '2_Sersic_bend2')
            lo, med, hi = np.percentile(s.chain[:, -100:, col], [2.5, 50.0, 97.5])
            print('bend2 of the last 100 iterations: 2.5 %% %.4f, median %.4f, 97.5 %% %.4f' % (lo, med, hi))
            assert model.num_params == 8 and lo <= 0.25 <= hi
        model.close()
    print('maximum log-posterior: bent %.2f, a_2 = 0 %.2f' % tuple(best))
    assert best[0] - best[1] > 8
