"""The Fisher matrix and gradient on the device (psfmc_fisher_rows), the mode search built on them (`find_mode`) and
`model_galaxy_mcmc(start='mode')`, against the numpy definition (`psfmc_amd.mode.fisher_from_stencil`) fed with the
ORACLE's images -- never the device's own.

The bound of the entry against the definition is derived, not picked (`mode_helpers.fisher_error_bound`): the
per-pixel tolerance tests/test_gpu_parity.py test_images_match_fp64_oracle holds the device's images to -- 1e-12 of
an image's largest value -- propagated to first order through a_k, b_k, w and r on the oracle's images, times the
project's factor 4 (helpers.RASTER_ORACLE_FACTOR).  The figures it gives for the cases below are in DESIGN.md
section 30.

That bound is as large as the variance half of the Gram matrix on every case but `noisy-psf`, so the entry is also
held, on the device's OWN sample images, to the definition in long double within the roundings that separate the two
(`mode_helpers.fisher_reference_longdouble`, `mode_helpers.fisher_rounding_bound`; tests/test_fisher_reference.py
shows on the CPU what that bound catches).  tests/test_gpu_fisher_paths.py and tests/test_gpu_fisher_fields.py do the
same on every tile count of the Gram kernel and for the fields of a set."""
import numpy as np
import pytest

import helpers
import mode_helpers as mh
import psfmc_oracle as orc
from psfmc_amd import engine, mode

pytestmark = pytest.mark.gpu

PARITY_IMAGE_TOL = 1e-12         # tests/test_gpu_parity.py test_images_match_fp64_oracle, of the image's largest value
BACKENDS = ['fused', 'hipfft']


# ---------------------------------------------------------------------------
# 1. the Gram kernel alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n_pix', [1, 3, 4, 64, 65, 255, 257, 4099])
@pytest.mark.parametrize('k', [1, 3, 15, 16, 17, 31, 32, 33, 47, 48, 63])
def test_gram_kernel_is_exact_on_small_integers(k, n_pix):
    """Small-integer vectors: every product and every sum is exact in fp64 (|sum| <= 4099 * 2 * 81 < 2^53), so F and g
    equal numpy's integer result exactly, whatever the order of the sums; every row and column of a tile holds a
    different vector, so a result written to the wrong row of the f64 fragment map is a wrong integer.  K = 1, 3 sit
    below one tile (K + 1 <= 16 with the gradient's column), 16 and 17 put that column or a row in a second tile, 33
    needs three tile rows and their off-diagonal tiles; 15 fills one tile with the gradient in its last column, and
    15 | 16, 31 | 32, 47 | 48 sit either side of each tile-row step, 63 is the largest K (four tile rows, ten tiles:
    k_fisher_gram<4, FisherVectors> and the finish kernel's triangle walk at T = 4); n_pix = 1, 3 are less than one
    MFMA, 4 exactly one, 64 exactly one wave, 65 a second wave that holds one pixel, 255 one short of four waves'
    slabs (one workgroup), 257 a second workgroup that holds one pixel, 4099 sixty-five slabs with a tail of 3 in the
    last and a second round of the finish kernel's four-way split.  A fifth of the pixels are zeroed (bad
    pixels)."""
    rng = np.random.RandomState(1000 * k + n_pix)
    a = rng.randint(-9, 10, size=(k, n_pix)).astype(np.float64)
    b = rng.randint(-9, 10, size=(k, n_pix)).astype(np.float64)
    c = rng.randint(-9, 10, size=n_pix).astype(np.float64)
    d = rng.randint(-9, 10, size=n_pix).astype(np.float64)
    bad = rng.rand(n_pix) < 0.2
    for v in (a, b, c, d):
        v[..., bad] = 0.0
    ai, bi, ci, di = (v.astype(np.int64) for v in (a, b, c, d))
    want_f = np.dot(ai, ai.T) + np.dot(bi, bi.T)
    want_g = np.dot(ai, ci) + np.dot(bi, di)
    got_f, got_g = engine.debug_fisher_gram(a, b, c, d)
    assert np.array_equal(got_f, got_f.T)
    assert np.array_equal(got_f, want_f.astype(np.float64)), np.argwhere(got_f != want_f)[:4]
    assert np.array_equal(got_g, want_g.astype(np.float64))


def test_gram_hook_refuses_bad_arguments():
    one = np.zeros((1, 4))
    with pytest.raises(engine.NativeError):
        engine.debug_fisher_gram(np.zeros((64, 4)), np.zeros((64, 4)), np.zeros(4), np.zeros(4))
    with pytest.raises(ValueError):
        engine.debug_fisher_gram(one, one, np.zeros(3), np.zeros(4))


# ---------------------------------------------------------------------------
# 2. the entry against the definition on the oracle's images
# ---------------------------------------------------------------------------
def _synth_model(fld, backend, max_walkers=64):
    """test_gpu_fullsize.make_model's point source + Sersic model on a given synth field."""
    from psfmc_amd import MultiComponentModel
    from psfmc_amd.ModelComponents import Configuration, PointSource, Sersic
    from psfmc_amd.distributions import Uniform, WeibullMinimum
    side = fld['sci'].shape[0]
    c = np.array((side / 2 + 0.5,) * 2)
    comps = [Configuration(fld['sci'], fld['ivm'], fld['psf'], fld['psf_ivm'], mag_zeropoint=fld['mag_zp']),
             PointSource(xy=Uniform(loc=c - 8, scale=16 * np.ones(2)), mag=Uniform(loc=18.0, scale=2.0)),
             Sersic(xy=Uniform(loc=c - 8, scale=16 * np.ones(2)), mag=Uniform(loc=19.0, scale=5.0),
                    reff=Uniform(loc=2.0, scale=side / 16.0), reff_b=Uniform(loc=2.0, scale=side / 16.0),
                    index=WeibullMinimum(c=1.5, scale=4), angle=Uniform(loc=0, scale=180), angle_degrees=True)]
    return MultiComponentModel(comps, backend=backend, max_walkers=max_walkers)


NOISY_PSF_WEIGHT = 1e-3          # the `noisy-psf` case: the synth field's PSF weight map times this
MIN_VARIANCE_SHARE = 0.5         # ... so that 1/2 sum w^2 dv_k^2 is at least this share of F_kk for some column


def _synth_case(psf_weight=1.0):
    fld, field = mh.synth_field_64(psf_weight)
    return dict(build=lambda backend: _synth_model(fld, backend), field=field,
                layout=mh.SYNTH_LAYOUT, has_psf_index=False, theta=fld['truth'], n_columns=10)


def _edge_case(shape, comps, n_psf=1, spoil=False, seed=4100, psf_side=21, max_walkers=64):
    import test_gpu_random as tgr
    case = tgr.edge_case(seed + shape[0] * 7 + shape[1], shape, (psf_side, psf_side), comps, n_walkers=3, n_psf=n_psf)
    if spoil:                    # a mask, weights <= 0 and NaN pixels, whatever the random field drew
        case['mask'] = np.zeros(shape, dtype=np.uint8)
        case['mask'][10:17, 40:52] = 1
        case['ivm'] = case['ivm'].copy()
        case['ivm'][5, 7], case['ivm'][33, 30], case['ivm'][34, 30] = 0.0, -1.0, np.nan
        case['sci'] = case['sci'].copy()
        case['sci'][12, 45], case['sci'][40, 21] = np.nan, np.nan      # one under the mask, one on its own
    field = orc.make_field(case['sci'], case['ivm'], case['psfs'], case['pivms'], mask=case['mask'], mag_zp=case['zp'])
    return dict(build=lambda backend, max_walkers=max_walkers: tgr.build(case, backend, max_walkers=max_walkers),
                field=field, layout=case['layout'], has_psf_index=case['has_psf_index'], theta=case['theta'][0],
                n_columns=len(case['theta'][0]) - int(case['has_psf_index']))


def _ps(nx, ny):
    return dict(type='ps', xy=(nx * 0.45 + 0.3, ny * 0.55 - 0.2), mag=18.5, method='lanczos3')


def _sersic(nx, ny, k=0):
    return dict(type='sersic', xy=(nx * (0.5 + 0.12 * k) + 0.4, ny * (0.45 - 0.1 * k) + 0.1), mag=18.0 + k, reff=5.0 + k,
                reff_b=3.0 + 0.5 * k, index=1.5 + k, angle=35.0 + 50 * k, angle_degrees=True)


def _general_case():
    """Sky + PS + a boxy Moffat with an inner truncation: aux rows of every block up to the truncations."""
    import test_gpu_general_components as tgg
    import test_gpu_radial_laws as tgl
    from psfmc_amd.ModelComponents import Moffat
    fld = tgg.make_field(64, 64, seed=1)
    field = tgg.oracle_field(fld)
    comps = [(Moffat, dict(angle='free', boxiness='free', truncation={'inner': (tgl.U(-5.0, 90.0), tgl.U(-5.0, 90.0))}))]
    values = tgl.named(2, 'Moffat', angle=110.0, beta=2.5, boxiness=0.6, fwhm=6.0, fwhm_b=4.0, mag=18.8,
                       xy=(32.25, 32.4), trunc_in_lo=0.5, trunc_in_hi=3.0)
    build = lambda backend: tgl.build(fld, comps, backend=backend, max_walkers=64, degrees=True)
    host = build('hipfft')                   # the contract's raw model comes from a model's host components
    theta = tgl.vector(host, fld, values)
    return dict(build=build, field=field, layout=None, has_psf_index=False, theta=theta, n_columns=len(theta),
                evaluate=lambda fld_, t: tgg.contract_evaluate(host, fld_, t), host=host)


CASES = {
    'synth64': _synth_case,
    'noisy-psf': lambda: _synth_case(NOISY_PSF_WEIGHT),
    'embedded70x64': lambda: _edge_case((70, 64), [_ps(64, 70), _sersic(64, 70)]),
    'edge-mask-nan': lambda: _edge_case((64, 64), [dict(type='sky', adu=0.004), _ps(64, 64), _sersic(64, 64)],
                                        spoil=True),
    'psf-index': lambda: _edge_case((64, 64), [dict(type='sky', adu=0.004), _ps(64, 64), _sersic(64, 64),
                                               _sersic(64, 64, 1)], n_psf=2),
    'boxy-moffat-truncated': _general_case,
}
_REFS = {}


def reference(name, make=None):
    """The case (CASES[name], or make()), the steps and columns `model.fisher` takes by default, and the definition on
    the oracle's images of the same 2K+1 vectors with its derived bounds: computed once per case, shared by the back
    ends."""
    if name in _REFS:
        return _REFS[name]
    case = (make or CASES[name])()
    model = case['build']('hipfft')              # host side only: columns and steps come from the priors
    columns = mode.default_columns(model)
    assert len(columns) == case['n_columns']
    step = mode.default_steps(model, case['theta'], columns)
    model.close()
    want_f, want_g, imgs = mh.oracle_fisher(case['field'], case['layout'], case['theta'], step, columns,
                                            case['has_psf_index'], case.get('evaluate'))
    fin = np.isfinite(imgs['ivm'][0])
    eps_conv = PARITY_IMAGE_TOL * np.abs(imgs['conv'][0]).max()
    eps_ivm = PARITY_IMAGE_TOL * np.abs(imgs['ivm'][0][fin]).max()
    bound_f, bound_g = mh.fisher_error_bound(imgs, case['field'], 0.5 / step[0], eps_conv, eps_ivm)
    print('%s: K = %d, derived bounds F %.3g, g %.3g' % (name, len(columns), bound_f, bound_g))
    assert np.all(np.isfinite(want_f)) and np.linalg.eigvalsh(want_f).min() > 0
    share = mh.variance_share(imgs['conv'], imgs['ivm'], ~case['field'].bad_px, 0.5 / step[0])
    print('%s: largest share of the variance half in F_kk %.3g' % (name, share.max()))
    if name == 'noisy-psf':
        assert share.max() >= MIN_VARIANCE_SHARE
    _REFS[name] = dict(case=case, columns=columns, step=step, F=want_f, g=want_g, imgs=imgs, bounds=(bound_f, bound_g),
                       share=share)
    return _REFS[name]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', sorted(CASES))
def test_entry_matches_the_definition_on_oracle_images(name, backend):
    ref = reference(name)
    case = ref['case']
    model = case['build'](backend)
    if name == 'embedded70x64' and backend == 'fused':
        assert (int(model.engine.get_option('transform_ny')), int(model.engine.get_option('transform_nx'))) != (70, 64)
    if name == 'psf-index':
        assert len(ref['columns']) == model.num_params - 1           # the discrete column is left out
    if name == 'boxy-moffat-truncated':
        assert model.aux_rows(case['theta']).shape[1] == 2 + 25
    out = model.fisher(case['theta'])
    assert np.array_equal(out['columns'], ref['columns']) and np.array_equal(out['step'], ref['step'][0])
    assert out['F'].shape == (len(ref['columns']),) * 2 and np.array_equal(out['F'], out['F'].T)
    err_f, err_g = mh.fisher_errors(out['F'], out['grad'], ref['F'], ref['g'])
    print('%s %s: normalised error F %.3g (bound %.3g), g %.3g (bound %.3g)' % (
        name, backend, err_f, ref['bounds'][0], err_g, ref['bounds'][1]))
    assert err_f <= ref['bounds'][0] and err_g <= ref['bounds'][1]
    want_ll = ref['imgs']['ll'][0]
    assert abs(out['loglike'] - want_ll) <= 1e-9 * abs(want_ll)
    # 4. the device's own sample images: the entry against the long-double definition of the SAME images, within
    # the roundings that separate the two (mode_helpers.fisher_rounding_bound)
    vecs = mode.stencil(case['theta'], ref['step'], ref['columns'])[0]
    held_to_own_images(model, vecs, out, 0.5 / ref['step'][0], '%s %s' % (name, backend))
    model.close()


def held_to_own_images(model, vecs, out, inv2h, tag):
    """Assert that `out` (F, grad of ONE stencil from the entry) lies within `fisher_rounding_bound` of
    `fisher_reference_longdouble` on the model's own `sample_images` of the stencil's vectors; the science image and
    the counted pixels are the model's.  -> the reference (F, g) as float64."""
    dev = model.sample_images(vecs, ('convolved_model', 'composite_ivm'))
    sci, good = np.asarray(model.config.obs_data, dtype=np.float64), ~np.asarray(model.config.bad_px, dtype=bool)
    args = (dev['convolved_model'], dev['composite_ivm'], sci, good, inv2h)
    want_f, want_g = mh.fisher_reference_longdouble(*args)
    bound_f, bound_g = mh.fisher_rounding_bound(*args)
    assert np.all(np.isfinite(want_f.astype(np.float64))) and np.all(np.isfinite(want_g.astype(np.float64)))
    err_f, err_g = mh.fisher_errors(out['F'], out['grad'], want_f, want_g)
    print('%s, own images, K = %d: rounding-level error F %.3g (bound %.3g), g %.3g (bound %.3g)' % (
        tag, len(want_g), err_f, bound_f, err_g, bound_g))
    assert err_f <= bound_f and err_g <= bound_g, (tag, err_f, bound_f, err_g, bound_g)
    return want_f.astype(np.float64), want_g.astype(np.float64)


# ---------------------------------------------------------------------------
# 3. batch independence
# ---------------------------------------------------------------------------
def _straddle_side(n_st):
    """The smallest built side at which the middle one of three stencils of n_st walkers straddles a pass boundary:
    the pass size is read from the library (a context on blank pixels)."""
    for side in [s for s in engine.FUSED_SIDES if s >= 256]:
        blank = np.ones((side, side))
        ctx = engine.Context(blank, blank, np.zeros((side, side), dtype=bool), np.ones((1, 21, 21)),
                             np.ones((1, 21, 21)), n_ps=1, n_sersic=1, max_walkers=97)
        size = ctx.pass_size(1)
        ctx.close()
        if any(n_st < b < 2 * n_st for b in range(size, 3 * n_st, size)):
            return side, size
    raise AssertionError('no built side splits %d walkers inside the middle stencil' % (3 * n_st))


def _three_stencils(model, thetas):
    assert model.engine.pass_size(1) == int(model.engine.get_option('chunk_walkers'))
    both = model.fisher(thetas)
    alone = model.fisher(thetas[1])
    again = model.fisher(thetas)
    for key in ('F', 'grad', 'loglike'):
        assert np.array_equal(both[key][1], alone[key]), key
        assert np.array_equal(both[key], again[key]), key
    assert not np.array_equal(both['F'][0], both['F'][1])
    assert np.array_equal(both['loglike'], model.log_likelihood_batch(thetas))


def test_a_stencil_does_not_depend_on_the_batch_fused():
    import synth_field
    import test_gpu_fullsize as tfs
    side, size = _straddle_side(21)
    print('side %d: passes of %d walkers' % (side, size))
    model, fld = tfs.make_model(side, 1, 'fused', max_walkers=64)
    assert model.engine.pass_size(1) == size and 3 * 21 <= 64
    assert any(21 < b < 42 for b in range(size, 63, size))           # the middle stencil straddles a pass boundary
    thetas = np.vstack([fld['truth'], synth_field.draw_walkers(side, 1, 2, seed=3, near_truth=fld['truth'])])
    _three_stencils(model, thetas)
    model.close()


def test_a_stencil_does_not_depend_on_the_batch_hipfft():
    import synth_field
    import test_gpu_fullsize as tfs
    model, fld = tfs.make_model(64, 1, 'hipfft', max_walkers=64)
    model.engine.set_option('chunk_walkers', 30)                     # 21 < 30 < 42
    thetas = np.vstack([fld['truth'], synth_field.draw_walkers(64, 1, 2, seed=3, near_truth=fld['truth'])])
    _three_stencils(model, thetas)
    model.close()


# ---------------------------------------------------------------------------
# 4. model.fisher(): refusals, and what a context that never calls it looks like
# ---------------------------------------------------------------------------
OPTION_KEYS = ('chunk_walkers', 'max_walkers', 'streams', 'stagger', 'cols3', 'column_engine', 'raster_group',
               'row_group', 'rows3', 'pow_tabs', 'partials_per_walker', 'storage_f32', 'aux_stride', 'cols_grid',
               'transform_ny', 'transform_nx', 'linear_accumulation', 'speculate', 'exclusive')


def test_fisher_refusals_and_untouched_contexts():
    import test_gpu_fullsize as tfs
    from test_gpu_general_components import make_field, make_model
    f32 = make_model(make_field(64, 64), storage='f32')
    with pytest.raises(ValueError, match='f64'):
        f32.fisher(np.zeros(f32.num_params))
    rows = np.zeros((1, 3, f32.engine.row_len))
    with pytest.raises(engine.NativeError, match='fp64'):
        f32.engine.fisher_rows(rows, np.ones((1, 1)), aux=np.zeros((3, 3)))
    f32.close()
    used, fld = tfs.make_model(64, 1, 'fused', max_walkers=64)
    fresh, _ = tfs.make_model(64, 1, 'fused', max_walkers=64)
    before = {k: used.engine.get_option(k) for k in OPTION_KEYS}
    ll = fresh.log_posterior_batch(fld['truth'])
    used.fisher(fld['truth'])
    assert {k: used.engine.get_option(k) for k in OPTION_KEYS} == before
    assert {k: fresh.engine.get_option(k) for k in OPTION_KEYS} == before
    assert np.array_equal(used.log_posterior_batch(fld['truth']), ll)
    # the limits of the entry
    with pytest.raises(ValueError):
        used.engine.fisher_rows(np.zeros((5, 21, used.engine.row_len)), np.ones((5, 10)))     # 105 walkers > 97
    with pytest.raises(ValueError):
        used.fisher(fld['truth'], columns=[])
    with pytest.raises(ValueError):
        used.fisher(fld['truth'], step=0.0)
    some = used.fisher(fld['truth'], columns=[0, 3], step=[1e-4, 1e-3])
    assert some['F'].shape == (2, 2) and np.all(np.isfinite(some['F']))
    used.close()
    fresh.close()


# ---------------------------------------------------------------------------
# 5. find_mode, 6. model_galaxy_mcmc(start='mode')
# ---------------------------------------------------------------------------
def test_find_mode_from_prior_draws():
    import test_gpu_fullsize as tfs
    from psfmc_amd import find_mode
    model, fld = tfs.make_model(64, 1, 'fused', max_walkers=64)
    # The CPU oracle search's mode value.  The likelihood's maximum (mode_helpers.cpu_mode_search) lies OUTSIDE this
    # model's priors -- reff = 6.20 where the prior ends at 6 -- so the value a posterior search can be held to is
    # that of the same search on the oracle's likelihood plus the model's host priors, started at the truth: it
    # stops on the edge reff = 6.
    field, columns = mh.synth_field_64()[1], np.arange(model.num_params)
    inside = lambda th: np.isfinite(model.log_priors_batch(th))

    def oracle_posterior(th):
        lp = model.log_priors_batch(th)
        return np.where(np.isfinite(lp), mh.oracle_loglike(field, mh.SYNTH_LAYOUT, th) + lp, -np.inf)

    def oracle_curvature(thetas):
        step = mode.default_steps(model, thetas, columns)
        first, second = mode.prior_derivatives(model.log_priors_batch, thetas, step, columns)
        pairs = [mh.oracle_fisher(field, mh.SYNTH_LAYOUT, t, s, columns)[:2] for t, s in zip(thetas, step)]
        return (np.array([p[0] for p in pairs]) - np.array([np.diag(s) for s in second]),
                np.array([p[1] for p in pairs]) + first)

    cpu = mode.lm_search(oracle_curvature, oracle_posterior, fld['truth'], columns, feasible=inside)[0]
    assert cpu.converged and cpu.lnpost > oracle_posterior(fld['truth'][None, :])[0]
    res = find_mode(model, rng=np.random.RandomState(11))
    print('find_mode: %r, laplace lnZ %.3f; CPU oracle search %.9f' % (res, res.laplace_log_evidence, cpu.lnpost))
    assert res.converged and res.ok
    assert res.lnpost >= cpu.lnpost - 1e-9 * abs(cpu.lnpost)
    np.linalg.cholesky(res.cov)
    assert np.array_equal(res.cov, res.cov.T) or np.allclose(res.cov, res.cov.T, rtol=1e-10, atol=0)
    assert np.isfinite(res.laplace_log_evidence)
    assert res.lnpost == model.log_posterior_batch(res.theta)[0]
    model.close()


def test_model_galaxy_mcmc_starts_from_the_mode(tmp_path):
    import test_gpu_fullsize as tfs
    from psfmc_amd import model_galaxy_mcmc, load_database
    k = 10

    def run(tag, **kw):
        model, _ = tfs.make_model(64, 1, 'fused', max_walkers=64)
        np.random.seed(17)                                # prior draws use numpy's global generator
        out = str(tmp_path / tag)
        model_galaxy_mcmc(model, output_name=out, chains=22, burn=0, iterations=20, random_state=5, quiet=True,
                          **kw)
        model.close()
        return out + '_db.fits'

    db = load_database(run('mode', start='mode'))
    assert db.meta['MCSTART'] == 'mode' and np.isfinite(db.meta['MCMODELP'])
    first = np.asarray(db['lnprobability'])[np.asarray(db['sample']) == np.min(db['sample'])]
    assert len(first) == 22 and np.all(np.isfinite(first))
    print('first iteration: %.2f ... %.2f below the mode' % (np.min(db.meta['MCMODELP'] - first),
                                                             np.max(db.meta['MCMODELP'] - first)))
    assert np.all(db.meta['MCMODELP'] - first <= 3 * k)
    plain, prior = run('plain'), run('prior', start='prior')
    with open(plain, 'rb') as a, open(prior, 'rb') as b:
        assert a.read() == b.read()
    assert 'MCSTART' not in load_database(prior).meta and 'MCMODELP' not in load_database(prior).meta
