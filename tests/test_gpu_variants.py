"""The kernels a caller selects at run time, held to the fp64 oracle like the defaults: every column engine of option
cols3 at every row-group size it meets, the two-stage inverse row kernels behind PSFMC_ROWS3=0, complex64 storage
(storage='f32') at every shape it accepts, and the refusals of the options that select them.

Every case asserts what the library reports it runs (column_engine: 0 k_cols, 1 k_cols3, 2 k_cols3g, 3 k_cols3f;
rows3; row_group; storage_f32; the transform shape) against literal values, so a silent fall-back to another kernel
fails here."""
import numpy as np
import pytest

import helpers
import psfmc_oracle as orc
from test_gpu_headline import ORACLE_TOL, REF_TOL
from test_gpu_random import (build, check_images, check_posterior_sums, check_walkers, image_pair, oracle_walker,
                             random_case, several_passes)

pytestmark = pytest.mark.gpu

K_COLS, K_COLS3, K_COLS3G, K_COLS3F = 0, 1, 2, 3
# Two fp64 column engines are two orderings of the same transform: each transformed value differs by O(log2 N) ulps
# of the column's norm (about 10 x 1.1e-16 here), so chi^2 -- a sum of S non-negative terms plus the log-weights, of
# the magnitude of |lnL| for these fields -- moves by a few 1e-15 relative.  1e-11 is the bound the suite already
# holds the fused back end to against hipFFT (independent fp64 arithmetic), far below any wrong value.
ENGINE_TOL = 1e-11


def field_of(case):
    return orc.make_field(case['sci'], case['ivm'], case['psfs'], case['pivms'], mask=case['mask'], mag_zp=case['zp'])


def assert_report(eng, tag, column_engine=None, rows3=None, row_group=None, storage_f32=None, transform=None):
    if column_engine is not None:
        assert eng.get_option('column_engine') == column_engine, (tag, eng.get_option('column_engine'))
    if rows3 is not None:
        assert eng.get_option('rows3') == rows3, (tag, eng.get_option('rows3'))
    if row_group is not None:
        assert eng.get_option('row_group') == row_group, (tag, eng.get_option('row_group'))
    if storage_f32 is not None:
        assert eng.get_option('storage_f32') == storage_f32, tag
    if transform is not None:
        assert (eng.get_option('transform_ny'), eng.get_option('transform_nx')) == transform, tag


def check_against_oracle(model, case, field, tag, sums=True):
    """The oracle checks of one variant: a distinct-walker batch in passes of at most two (uneven tail), the images of
    two walkers from one call, and (sums) the posterior-image sums under both accumulation routes -- the linear sums
    convolved through the from-image column path, and every sample through the whole pipeline."""
    theta = case['theta']
    n_w = len(theta)
    want_ll = np.array([oracle_walker(field, case, t)[0] for t in theta])
    chunk = model.engine.get_option('chunk_walkers')
    assert several_passes(model, n_w) <= 2
    got = model.log_posterior_batch(theta)
    check_walkers(got, want_ll, model.log_priors_batch(theta), case['outside'], tag)
    model.engine.set_option('chunk_walkers', chunk)
    pair = image_pair(want_ll)
    assert pair, tag
    refs = [oracle_walker(field, case, theta[i], images=True)[1] for i in pair]
    check_images(model.sample_images(theta[pair]), refs, tag)
    if sums:
        for linear in (1, 0):
            model.engine.set_option('linear_accumulation', linear)
            check_posterior_sums(model, theta[pair], refs, (tag, 'linear_accumulation', linear))
        model.engine.set_option('linear_accumulation', 1)
    return got


# (shape (ny = column length, nx), cols3, column_engine, row_group): nx 64 gives row groups of 8 (the unguarded
# power-of-two row kernels of 8 rows per wave), nx 96 / 100 groups of 4
COLUMN_CASES = [
    # cols3 = 0: the two-stage k_cols at 512 / 1024 ...
    ((512, 64), 0, K_COLS, 8), ((512, 96), 0, K_COLS, 4), ((1024, 64), 0, K_COLS, 8), ((1024, 100), 0, K_COLS, 4),
    # ... and at sides whose default is k_cols3g: 384 (load pipeline), 500 (eight per-lane offsets), 640, 900
    ((384, 96), 0, K_COLS, 4), ((500, 100), 0, K_COLS, 4), ((640, 64), 0, K_COLS, 8), ((900, 96), 0, K_COLS, 4),
    # cols3 = 3: round 3's k_cols3 (fp64 storage)
    ((512, 64), 3, K_COLS3, 8), ((512, 96), 3, K_COLS3, 4), ((1024, 64), 3, K_COLS3, 8), ((1024, 100), 3, K_COLS3, 4),
    # cols3 = 2: k_cols3g at the four 8 m x 64 sides (L = 64: its layout serves every row group)
    ((512, 64), 2, K_COLS3G, 8), ((1024, 100), 2, K_COLS3G, 4), ((1536, 96), 2, K_COLS3G, 4), ((2048, 64), 2, K_COLS3G, 8),
    # 520 = 10 x 52 (k_cols3g's L = 52 lanes): a multiple of 4 but not of 8, so rows in groups of 8 fall back to k_cols
    # (default and 2; cols3g_layout_ok)
    ((520, 64), 1, K_COLS, 8), ((520, 64), 2, K_COLS, 8),
    # cols3 = 4: the defaults
    ((512, 96), 4, K_COLS3F, 4), ((1024, 64), 4, K_COLS3F, 8), ((1536, 96), 4, K_COLS3F, 4),
]


def test_column_cases_cover_the_issue():
    assert {c[1] for c in COLUMN_CASES} == {0, 1, 2, 3, 4}
    for cols3, sides in ((0, (512, 1024)), (3, (512, 1024))):
        for side in sides:
            assert {c[3] for c in COLUMN_CASES if c[1] == cols3 and c[0][0] == side} == {4, 8}, (cols3, side)
    assert {c[0][0] for c in COLUMN_CASES if c[1] == 2 and c[2] == K_COLS3G} == {512, 1024, 1536, 2048}


@pytest.mark.parametrize('shape,cols3,code,group', COLUMN_CASES,
                         ids=lambda v: '%dx%d' % v if isinstance(v, tuple) else str(v))
def test_column_engine_matches_oracle(shape, cols3, code, group):
    """One column engine on one shape against the oracle (check_against_oracle); at cols3 = 4 also bit for bit the
    default engine's values."""
    case = random_case(11000 + 3 * shape[0] + shape[1] + 7 * cols3, shape, n_walkers=5)
    model = build(case, 'fused', max_walkers=8)
    eng = model.engine
    default = model.log_posterior_batch(case['theta'])
    eng.set_option('cols3', cols3)
    assert eng.get_option('cols3') == cols3
    assert_report(eng, (shape, cols3), column_engine=code, row_group=group, rows3=0, storage_f32=0, transform=shape)
    got = check_against_oracle(model, case, field_of(case), (shape, cols3))
    if cols3 in (1, 4):
        assert np.array_equal(got, default), shape
    model.close()


def test_column_engine_of_an_embedded_transform():
    """An image of an unbuilt side (530 = 2 x 5 x 53; PSF 32 x 16) embedded in a transform whose default columns run
    on k_cols3g (576, choose_embedding): k_cols there (cols3 = 0) against the oracle, with the wrapped rasteriser and
    the embedding margin.  (The draw has a raw-model peak below 100 counts: fields with peaks of 1e5 put even hipFFT
    several 1e-9 from the oracle -- the variance channel's rounding grows with the squared peak, test_gpu_random.)"""
    from psfmc_amd import engine
    case = random_case(11778, (530, 96), n_walkers=5)
    assert case['psfs'][0].shape == (32, 16)
    model = build(case, 'auto', max_walkers=8)
    eng = model.engine
    assert model._backend == 'fused'
    assert_report(eng, 530, transform=(576, 96))
    ty = 576
    assert engine.column_engine(ty)[0] == 'k_cols3g'
    assert_report(eng, ty, column_engine=K_COLS3G, row_group=4)
    eng.set_option('cols3', 0)
    assert_report(eng, ty, column_engine=K_COLS, row_group=4)
    check_against_oracle(model, case, field_of(case), ('embedded', ty))
    model.close()


@pytest.mark.parametrize('name', ['synth512x2', 'synth1024x4'])
def test_switching_column_engines_after_creation(tmp_path, name):
    """The kernel spectra are transformed once, at context creation, by the default engine; every engine selected
    later multiplies by them.  The fixture vectors under each engine against the reference (REF_TOL) and the fp64
    oracle evaluated next to it (ORACLE_TOL); every engine within ENGINE_TOL of the default; switching back gives
    the default's bits."""
    case, _ = helpers.load_light_case(name)
    n = len(case['params'])
    model = helpers.build_model(name, case, tmp_path, backend='fused', max_walkers=n)
    eng = model.engine
    side = case['sci'].shape[0]
    group = {512: 4, 1024: 2}[side]                  # the unguarded row kernels' rows per wave at nx = 512 / 1024
    want = np.where(np.isfinite(case['lnprob']), case['loglike_f64'] + case['lnprior'], -np.inf)
    assert_report(eng, name, column_engine=K_COLS3F, row_group=group, rows3=0)
    base = model.log_posterior_batch(case['params'])
    fin = np.isfinite(base)
    assert fin.sum() >= 2 and np.array_equal(fin, np.isfinite(want))
    for cols3, code in ((0, K_COLS), (3, K_COLS3), (2, K_COLS3G), (4, K_COLS3F), (1, K_COLS3F)):
        eng.set_option('cols3', cols3)
        assert_report(eng, (name, cols3), column_engine=code, row_group=group)
        got = model.log_posterior_batch(case['params'])
        assert helpers.rel_err(got, case['lnprob']) <= REF_TOL, cols3
        assert helpers.rel_err(got, want) <= ORACLE_TOL, cols3
        assert np.all(np.abs(got[fin] - base[fin]) <= ENGINE_TOL * np.abs(base[fin])), cols3
        if cols3 in (1, 4):
            assert np.array_equal(got, base), cols3
    model.close()


def test_cols3_refusals_keep_the_context():
    """set_option('cols3') refuses at that call -- not at the next evaluation -- values outside {0, ..., 4} and 0 where
    the transform's columns have no two-stage kernel (above 1024, an embedded transform too); the context keeps the
    engine it had and evaluates as before."""
    from psfmc_amd.engine import NativeError
    case = random_case(12001, (512, 96), n_walkers=3)
    model = build(case, 'fused', max_walkers=4)
    eng = model.engine
    assert eng.get_option('cols3') == 1
    eng.set_option('cols3', 3)
    before = model.log_posterior_batch(case['theta'])
    for bad in (-1, 5, 2.5, 0.5, 1e10, float('nan'), float('inf')):
        with pytest.raises(NativeError):
            eng.set_option('cols3', bad)
        assert eng.get_option('cols3') == 3 and eng.get_option('column_engine') == K_COLS3, bad
    assert np.array_equal(model.log_posterior_batch(case['theta']), before)
    model.close()
    # above 1024 (k_cols3f at 1536): refused at once, and the next default evaluation matches the oracle
    case = random_case(12002, (1536, 1536), n_walkers=3)
    model = build(case, 'fused', max_walkers=4)
    eng = model.engine
    with pytest.raises(NativeError):
        eng.set_option('cols3', 0)
    assert eng.get_option('cols3') == 1
    assert_report(eng, 1536, column_engine=K_COLS3F, rows3=3, row_group=1)
    field = field_of(case)
    want_ll = np.array([oracle_walker(field, case, t)[0] for t in case['theta']])
    check_walkers(model.log_posterior_batch(case['theta']), want_ll, model.log_priors_batch(case['theta']),
                  case['outside'], 1536)
    for cols3, code in ((2, K_COLS3G), (3, K_COLS3G), (4, K_COLS3F)):      # (3 acts as 2 away from 512 / 1024)
        eng.set_option('cols3', cols3)
        assert eng.get_option('column_engine') == code, cols3
    model.close()
    # an image embedded in a transform above 1024
    case = random_case(12003, (1100, 64), n_walkers=3)
    model = build(case, 'auto', max_walkers=4)
    eng = model.engine
    assert eng.get_option('transform_ny') > 1024
    with pytest.raises(NativeError):
        eng.set_option('cols3', 0)
    assert eng.get_option('cols3') == 1 and np.isfinite(model.log_posterior_batch(case['theta'][:1])).all()
    model.close()


# ---- two-stage inverse rows where the default is the three-stage kernel ----
ROWS3_SIDES = [676, 720, 728, 780, 784, 840, 900]


@pytest.mark.parametrize('nx', ROWS3_SIDES)
def test_two_stage_inverse_rows_match_oracle(monkeypatch, nx):
    """PSFMC_ROWS3=0 (read at context creation) puts these sides' inverse rows back on the two-stage k_rows_inv (the
    default before round 4): a distinct-walker batch and two walkers' images against the oracle."""
    shape = (64, nx)
    case = random_case(13000 + nx, shape, n_walkers=5)
    model = build(case, 'fused', max_walkers=8)
    assert_report(model.engine, nx, rows3=2, row_group=4)          # the default: the three-stage inverse kernel
    model.close()
    monkeypatch.setenv('PSFMC_ROWS3', '0')
    model = build(case, 'fused', max_walkers=8)
    assert_report(model.engine, nx, rows3=0, row_group=4, column_engine=K_COLS)
    check_against_oracle(model, case, field_of(case), ('rows3=0', nx), sums=False)
    model.close()


def test_rows3_environment_where_it_does_not_apply(monkeypatch):
    """PSFMC_ROWS3=0 above 1024 keeps the three-stage rows (no two-stage row kernel exists there); PSFMC_ROWS3=1 in
    a build without PSFMC_ROWS3_EXTRA changes nothing at a power-of-two side nor at a rows3 side."""
    case = random_case(13500, (64, 1152), n_walkers=3)
    monkeypatch.setenv('PSFMC_ROWS3', '0')
    model = build(case, 'fused', max_walkers=4)
    assert_report(model.engine, 1152, rows3=3, row_group=1)
    field = field_of(case)
    want_ll = np.array([oracle_walker(field, case, t)[0] for t in case['theta']])
    check_walkers(model.log_posterior_batch(case['theta']), want_ll, model.log_priors_batch(case['theta']),
                  case['outside'], 1152)
    model.close()
    for shape, rows3, group in (((96, 256), 0, 4), ((64, 676), 2, 4)):
        case = random_case(13600 + shape[1], shape, n_walkers=3)
        monkeypatch.delenv('PSFMC_ROWS3')
        model = build(case, 'fused', max_walkers=4)
        monkeypatch.setenv('PSFMC_ROWS3', '1')
        forced = build(case, 'fused', max_walkers=4)
        for m in (model, forced):
            assert_report(m.engine, shape, rows3=rows3, row_group=group,
                          column_engine=model.engine.get_option('column_engine'))
        assert np.array_equal(forced.log_posterior_batch(case['theta']), model.log_posterior_batch(case['theta']))
        model.close()
        forced.close()


# ---- complex64 storage ----
U32 = 2.0 ** -24        # unit roundoff of a float32 component (round to nearest)
POW2 = [64, 128, 256, 512, 1024, 2048]


def f32_bounds(model, imgs, good):
    """|lnL(storage_f32) - lnL(fp64)| per walker, from that walker's fp64 images.

    The fused path stores the row half-spectra twice per channel as complex64: after the forward rows (X, the rows'
    transform of the raw model and of its square) and after the columns (Y, the same of the convolved model and of
    the model variance).  Rounding each re / im part to nearest perturbs every stored element by |dX| <= u |X|,
    u = 2^-24.  The rest of the pipeline is linear in the stored values.  From X: the column transforms, the
    product with the kernel spectrum (operator norm kappa = max |K|, read from the device spectra) and the inverse
    transforms; from Y: the inverse rows.  A real inverse transform from a half spectrum has operator norm sqrt(2)
    relative to the full one, so with Parseval
        ||dm||_2 <= sqrt(2) u (kappa_m ||raw||_2 + ||m||_2) <= 2 sqrt(2) u kappa_m ||raw||_2,
        ||dv||_2 <= 2 sqrt(2) u kappa_v ||raw^2||_2
    (m the convolved model, v the model variance; ||m||_2 <= kappa_m ||raw||_2).  The log-likelihood
    lnL = -1/2 sum_good (r^2 w - log(w / 2 pi)), r = sci - m, w = 1 / (obs_var + v), moves to first order by
        d lnL = sum_good r w dm + 1/2 sum_good (w - r^2 w^2) dv,
    so by Cauchy-Schwarz |d lnL| <= ||r w||_2 ||dm||_2 + 1/2 ||w - r^2 w^2||_2 ||dv||_2 (good pixels).  The returned
    bound takes 4 u for 2 sqrt(2) u (second-order terms, the fp64 rounding of both evaluations)."""
    psf_spec, var_spec = model.engine.spectra()
    kappa_m, kappa_v = np.abs(psf_spec).max(), np.abs(var_spec).max()
    out = []
    for raw, r, w in zip(imgs['raw_model'], imgs['residual'], imgs['composite_ivm']):
        dm = 4 * U32 * kappa_m * np.linalg.norm(raw)
        dv = 4 * U32 * kappa_v * np.linalg.norm(raw * raw)
        rg, wg = r[good], w[good]
        out.append(np.linalg.norm(rg * wg) * dm + 0.5 * np.linalg.norm(wg - rg * rg * wg * wg) * dv)
    return np.array(out)


def good_pixels(sci, ivm, mask=None):
    good = np.isfinite(sci) & np.isfinite(ivm) & (ivm > 0)
    return good if mask is None else good & ~np.asarray(mask).astype(bool)


def fp64_images(model, theta):
    kinds = ('raw_model', 'residual', 'composite_ivm')
    parts = [model.sample_images(theta[i:i + 4], kinds) for i in range(0, len(theta), 4)]
    return {k: np.concatenate([p[k] for p in parts]) for k in kinds}


def check_f32(model, theta, got64, got32, good, tag):
    """got32 against got64 of the same context: the same non-finite pattern, a difference somewhere (the complex64
    path ran), every finite walker within its f32_bounds."""
    fin = np.isfinite(got64)
    assert np.array_equal(np.isfinite(got32), fin) and np.array_equal(got32[~fin], got64[~fin]), tag
    assert fin.any() and np.abs(got32[fin] - got64[fin]).max() > 0, tag
    bound = f32_bounds(model, fp64_images(model, theta[fin]), good)
    err = np.abs(got32[fin] - got64[fin])
    assert np.all(err <= bound + ENGINE_TOL * np.abs(got64[fin])), (tag, err, bound)
    return bound


def test_f32_storage_accepts_exactly_the_power_of_two_shapes_up_to_1024():
    """Every power-of-two pair 64 ... 2048: set_option('storage_f32', 1) either raises NativeError at that call (the
    context stays on fp64 storage and evaluates as before) or evaluation afterwards succeeds and agrees with fp64 on
    the same context at the derived bound.  Accepted: both sides <= 1024 (every power-of-two ny is a whole number of
    the unguarded row kernels' workgroups).  Refused too: 1536, embedded transforms, the hipFFT back end."""
    from psfmc_amd.engine import NativeError
    accepted = []
    for ny in POW2:
        for nx in POW2:
            case = random_case(14000 + ny + 3 * nx, (ny, nx), n_walkers=3)
            model = build(case, 'fused', max_walkers=4)
            eng = model.engine
            theta = case['theta']
            got64 = model.log_posterior_batch(theta)
            try:
                eng.set_option('storage_f32', 1)
            except NativeError:
                assert eng.get_option('storage_f32') == 0, (ny, nx)
                assert np.array_equal(model.log_posterior_batch(theta), got64), (ny, nx)
            else:
                accepted.append((ny, nx))
                assert_report(eng, (ny, nx), storage_f32=1, rows3=0)
                got32 = model.log_posterior_batch(theta)
                check_f32(model, theta, got64, got32, good_pixels(case['sci'], case['ivm'], case['mask']), (ny, nx))
            model.close()
    assert accepted == [(ny, nx) for ny in POW2 for nx in POW2 if max(ny, nx) <= 1024]
    for shape, backend in (((1536, 64), 'fused'), ((64, 1536), 'fused'), ((170, 170), 'auto'), ((256, 256), 'hipfft'),
                           ((498, 128), 'auto')):
        case = random_case(14500 + shape[0] + shape[1], shape, n_walkers=3)
        model = build(case, backend, max_walkers=4)
        with pytest.raises(NativeError):
            model.engine.set_option('storage_f32', 1)
        assert model.engine.get_option('storage_f32') == 0 and np.isfinite(
            model.log_posterior_batch(case['theta'][:1])).all(), shape
        model.close()


def test_f32_storage_refuses_a_set_of_fields_at_the_launch():
    """A set of two 64 x 64 fields: set_option('storage_f32', 1) is accepted (both sides are power-of-two shapes), and
    the next evaluation is refused at its inverse-row launch -- complex64 storage has no kernel that sums chi^2 per
    field.  With the option off again the set returns the bits it returned first."""
    from psfmc_amd import FieldSet
    from psfmc_amd.engine import NativeError
    from test_gpu_random import edge_case, edge_components
    cases = [edge_case(16000 + f, (64, 64), (9, 9), edge_components(64, 64), n_walkers=3) for f in range(2)]
    fs = FieldSet([build(c, 'fused', max_walkers=1) for c in cases], max_walkers=8)
    ctx = fs.context
    assert ctx.n_fields == 2
    assert_report(ctx, 'set', storage_f32=0, rows3=0, transform=(64, 64))
    thetas = [c['theta'] for c in cases]
    assert all(len(t) == 3 for t in thetas)
    first = fs.log_posterior_batch(thetas)
    assert all(np.isfinite(f).any() for f in first)
    ctx.set_option('storage_f32', 1)
    assert_report(ctx, 'set', storage_f32=1)
    with pytest.raises(NativeError, match='single-precision storage serves contexts of one field') as err:
        fs.log_posterior_batch(thetas)
    assert err.value.code == -1                                   # PSFMC_EINVAL
    ctx.set_option('storage_f32', 0)
    assert_report(ctx, 'set', storage_f32=0)
    again = fs.log_posterior_batch(thetas)
    assert all(np.array_equal(a, f) for a, f in zip(again, first))
    fs.close()


def f32_invariance(model, theta, got32, tag):
    """Bitwise: the batch permuted, and in passes of at most two."""
    perm = np.random.RandomState(len(theta)).permutation(len(theta))
    assert np.array_equal(model.log_posterior_batch(theta[perm]), got32[perm]), tag
    chunk = model.engine.get_option('chunk_walkers')
    several_passes(model, len(theta))
    assert np.array_equal(model.log_posterior_batch(theta), got32), tag
    model.engine.set_option('chunk_walkers', chunk)


def convolved_close(model, theta, ref, tag):
    got = model.sample_images(theta, ('convolved_model',))['convolved_model']
    assert np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max(), tag


@pytest.mark.parametrize('name', ['synth512x2', 'synth1024x4'])
def test_f32_storage_at_512_and_1024(tmp_path, name):
    """storage='f32' at the sizes bench.py times it (k_cols3<512 | 1024, cf>; at 1024 rows of 2 per wave): the
    fixture vectors against the reference (5e-6, test_single_precision_storage_option's bound) and the oracle at the
    derived bound; the convolved model within 2e-6 of its maximum; bitwise invariance; storage_f32 off restores the
    fp64 bits."""
    from psfmc_amd import MultiComponentModel
    case, _ = helpers.load_light_case(name)
    theta = case['params']
    n = len(theta)
    full = helpers.build_model(name, case, tmp_path, backend='fused', max_walkers=n)
    (tmp_path / 'f32').mkdir()
    half = MultiComponentModel(helpers.write_case_files(name, case, tmp_path / 'f32'), backend='fused',
                               max_walkers=n, storage='f32')
    group = {512: 4, 1024: 2}[case['sci'].shape[0]]
    assert_report(half.engine, name, storage_f32=1, column_engine=K_COLS3, row_group=group, rows3=0)
    got64 = full.log_posterior_batch(theta)
    got32 = half.log_posterior_batch(theta)
    assert helpers.rel_err(got32, case['lnprob']) <= 5e-6
    good = good_pixels(case['sci'], case['ivm'])
    bound = check_f32(full, theta, got64, got32, good, name)
    want = np.where(np.isfinite(case['lnprob']), case['loglike_f64'] + case['lnprior'], -np.inf)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got32), fin)
    assert np.all(np.abs(got32[fin] - want[fin]) <= bound + ORACLE_TOL * np.abs(want[fin])), name
    pick = np.flatnonzero(fin)[:2]
    convolved_close(half, theta[pick], full.sample_images(theta[pick], ('convolved_model',))['convolved_model'], name)
    f32_invariance(half, theta, got32, name)
    half.engine.set_option('storage_f32', 0)
    assert_report(half.engine, name, storage_f32=0, column_engine=K_COLS3F)
    assert np.array_equal(half.log_posterior_batch(theta), got64)
    full.close()
    half.close()


# (shape, cols3, column_engine, row_group) of complex64 storage away from the squares: k_cols3<512, cf> on rows in
# groups of 8, k_cols<1024, cf> and k_cols<512, cf> (cols3 = 0), and 1024-pixel rows (two per wave) over k_cols<128, cf>
F32_RECT = [((512, 64), 1, K_COLS3, 8), ((1024, 128), 0, K_COLS, 8), ((512, 256), 0, K_COLS, 4),
            ((128, 1024), 1, K_COLS, 2)]


@pytest.mark.parametrize('shape,cols3,code,group', F32_RECT, ids=lambda v: '%dx%d' % v if isinstance(v, tuple) else str(v))
def test_f32_storage_rectangular(shape, cols3, code, group):
    """A distinct-walker batch under storage_f32 against the oracle at the derived bound, the convolved model within
    2e-6 of its maximum, bitwise invariance, and fp64 bits back when it is turned off."""
    case = random_case(15000 + shape[0] + 3 * shape[1], shape, n_walkers=5)
    theta = case['theta']
    model = build(case, 'fused', max_walkers=8)
    eng = model.engine
    eng.set_option('cols3', cols3)
    got64 = model.log_posterior_batch(theta)
    pick = image_pair(got64)
    conv64 = model.sample_images(theta[pick], ('convolved_model',))['convolved_model']
    eng.set_option('storage_f32', 1)
    assert_report(eng, shape, storage_f32=1, column_engine=code, row_group=group, rows3=0)
    got32 = model.log_posterior_batch(theta)
    eng.set_option('storage_f32', 0)
    good = good_pixels(case['sci'], case['ivm'], case['mask'])
    bound = check_f32(model, theta, got64, got32, good, shape)
    field = field_of(case)
    want_ll = np.array([oracle_walker(field, case, t)[0] for t in theta])
    want = want_ll + model.log_priors_batch(theta)
    fin = np.isfinite(got64)
    assert np.array_equal(np.isfinite(want), fin), shape
    assert np.all(np.abs(got32[fin] - want[fin]) <= bound + 2e-10 * np.abs(want_ll[fin])), shape
    eng.set_option('storage_f32', 1)
    convolved_close(model, theta[pick], conv64, shape)
    f32_invariance(model, theta, got32, shape)
    eng.set_option('storage_f32', 0)
    assert_report(eng, shape, storage_f32=0)
    assert np.array_equal(model.log_posterior_batch(theta), got64), shape
    model.close()
