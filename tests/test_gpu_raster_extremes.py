"""Every form of the Sersic rasteriser at the extremes a Uniform prior allows (helpers.RASTER_FORMS: one 64-row
image per form -- log2 + exp2, power tables with G = 1 / 2 / 4, one row per wave, their WRAP variants, the hipFFT
back end's literal formula -- and helpers.extreme_specs: indices 0.1 ... 15, radii 0.05 ... 3000, axis ratios 0.01
and 1, angles whose cosines are 6e-17, centres on, beside and far off the pixels, magnitudes 8 ... 60, the two ends of
the power tables' exponent range), each extreme in one of three Sersic slots with ordinary or dark neighbours.

Held to: the fp64 oracle's log-likelihood (fuzz_shapes.fuzz_bound), a long-double evaluation of the raw model per
pixel (bound max(1e-11, 4 x the oracle's own error against it), helpers.extreme_references), the posterior sums
(k_raster_sums), and -- device against device, bit for bit -- independence of the table source, of the walkers a
walker is batched with, of their order and of the pass size.  tests/test_raster_extremes_reference.py holds the
references and the conditions that keep these checks from passing emptily, without a GPU."""
import numpy as np
import pytest

import helpers
from helpers import RASTER_FORMS

pytestmark = pytest.mark.gpu

FORM_IDS = [f[0] for f in RASTER_FORMS]
BELOW_FLOOR_MAX = 1e-279


def open_model(form, case, max_walkers, backend=None):
    """The model of one RASTER_FORMS row, with the PROOF of which rasteriser it runs: what the context reports
    through get_option against the row's expectations."""
    import test_gpu_random as tgr
    from psfmc_amd import engine
    tag, shape, psf_shape, form_backend, kind, wrap, want = form
    backend = backend or form_backend
    model = tgr.build(case, backend, max_walkers=max_walkers)
    assert model._backend == backend, (tag, model._backend)
    eng = model.engine
    group = eng.get_option('raster_group')
    if backend != 'fused':
        assert np.isnan(group), (tag, group)            # the literal OCML formula: no tables, no groups
        print('RASTER-FORM %s backend=%s raster_group=nan' % (tag, backend))
        return model
    tny, tnx = int(eng.get_option('transform_ny')), int(eng.get_option('transform_nx'))
    report = dict(pow_tabs=int(eng.get_option('pow_tabs')), rows3_fwd=int(eng.get_option('rows3')) & 1,
                  raster_group=int(group))
    print('RASTER-FORM %s backend=fused transform=%dx%d %r' % (tag, tny, tnx, report))
    assert tny == shape[0], (tag, tny)
    if wrap:
        assert not engine.fused_supports(*shape) and tnx in engine.FUSED_SIDES
        assert tnx >= engine.embedding_side(shape[1], psf_shape[1]), (tag, tnx)
        assert (tnx <= 256) == (kind == 'logexp') and (tnx > 1024) == (kind == 'rows3'), (tag, tnx)
    else:
        assert tnx == shape[1], (tag, tnx)
    assert report == want, (tag, report, want)
    return model


def test_form_table_covers_every_rasteriser():
    helpers.check_raster_form_coverage()


@pytest.mark.parametrize('form', RASTER_FORMS, ids=FORM_IDS)
def test_extremes_match_references(form):
    """Every walker of the shape's list: log-likelihood against the fp64 oracle, raw model per pixel against the
    long-double evaluation, finiteness patterns, the posterior sums of an ordinary and an extreme walker, and
    finiteness on the other back end."""
    from test_gpu_random import check_posterior_sums
    tag, shape = form[0], form[1]
    refs = helpers.extreme_references(tag)
    theta, info = refs['theta'], refs['info']
    model = open_model(form, refs['case'], max_walkers=len(theta))
    got = model.log_likelihood_batch(theta)
    raw = model.sample_images(theta, ('raw_model',))['raw_model']
    assert raw.shape == (len(theta),) + tuple(shape)
    failures = []
    for i, inf in enumerate(info):
        who = '%s/%s/slot%d' % (inf['name'], inf['kind'], inf['slot'])
        exact, want = refs['exact'][i], refs['ll'][i]
        # the conditions the CPU companion checks, on this shape's own references
        assert np.isfinite(want) == ('on_pixel' not in inf['flags']), (tag, who, want)
        assert refs['n_rel'][i] >= 500 or (inf['kind'] == 'solo' and inf['name'] in helpers.FEW_PIXELS), (tag, who)
        rel, n_rel, low = helpers.pixel_errors(raw[i], exact)
        ll_err = abs(got[i] - want) if np.isfinite(want) and np.isfinite(got[i]) else float('nan')
        print('RASTER-EXTREME %-12s %-22s e_orc %.2e e_dev %.2e bound %.2e px %6d low %.1e | ll %.10g err %.2e bound %.2e'
              % (tag, who, refs['e_orc'][i], rel, refs['bound'][i], n_rel, low, got[i], ll_err, refs['ll_bound'][i]))
        if not np.array_equal(np.isfinite(raw[i]), np.isfinite(exact)):
            failures.append((who, 'finiteness pattern', int((~np.isfinite(raw[i])).sum())))
            continue
        if 'on_pixel' in inf['flags']:
            ys, xs = np.nonzero(np.isnan(raw[i]))
            if len(ys) != 1 or (xs[0], ys[0]) != (int(shape[1] * 0.5), shape[0] // 2):
                failures.append((who, 'NaN pixels', list(zip(xs, ys))))
        if not np.isfinite(want):
            if got[i] != -np.inf:
                failures.append((who, 'log-likelihood not -inf', got[i]))
        elif not (np.isfinite(got[i]) and ll_err <= refs['ll_bound'][i]):
            failures.append((who, 'log-likelihood', got[i], want, ll_err, refs['ll_bound'][i]))
        if not rel <= refs['bound'][i]:
            failures.append((who, 'raw model per pixel', rel, refs['bound'][i]))
        if not low <= BELOW_FLOOR_MAX:
            failures.append((who, 'pixels below the floor', low))
    assert not failures, (tag, failures)
    # posterior sums: k_raster_sums (log2 + exp2 in segments at every size) of the ordinary walker and one extreme
    # one, a different extreme on every shape
    names = [f[0] for f in RASTER_FORMS]
    cand = [i for i, inf in enumerate(info) if inf['kind'] == 'mixed' and inf['name'] != 'base' and
            np.isfinite(refs['ll'][i]) and 'near_pixel' not in inf['flags']]
    pair = [0, cand[(7 * names.index(tag) + 3) % len(cand)]]
    assert info[0]['name'] == 'base' and info[0]['kind'] == 'mixed'
    print('RASTER-SUMS %s base + %s' % (tag, info[pair[1]]['name']))
    check_posterior_sums(model, theta[pair], [refs['images'][i] for i in pair], (tag, info[pair[1]]['name']))
    model.close()
    # the other back end: finite exactly where this one is
    other_backend = 'hipfft' if form[3] == 'fused' else 'fused'
    from psfmc_amd import engine
    if other_backend == 'hipfft' or engine.fused_supports(shape[0], shape[1], form[2]):
        import test_gpu_random as tgr
        other = tgr.build(refs['case'], other_backend, max_walkers=len(theta))
        theirs = other.log_likelihood_batch(theta)
        other.close()
        assert np.array_equal(np.isfinite(theirs), np.isfinite(got)), \
            (tag, [info[i]['name'] for i in np.flatnonzero(np.isfinite(theirs) != np.isfinite(got))])


@pytest.mark.parametrize('form', RASTER_FORMS, ids=FORM_IDS)
def test_extremes_do_not_depend_on_the_batch(form):
    """Device against device, bit for bit.  TABLE SOURCE: the extreme list as small batches (the row waves form the
    table entries: pow_tabs_built == 0) and padded with ordinary walkers past the 8192 (row wave, component) pairs
    from which k_pow_tables builds them (pow_tabs_built == 1).  NO LEAKAGE: the ordinary walkers of a mixed batch
    return what they return without the extreme ones (a NaN, an inf or a saturated table entry must not cross lanes
    or records), under a permutation, and in passes of at most two walkers."""
    from test_gpu_random import several_passes
    tag, shape, backend = form[0], form[1], form[3]
    theta, info = helpers.extreme_walkers(*shape)
    n_ext = len(theta)
    case = helpers.extreme_case(shape, form[2])
    model = open_model(form, case, max_walkers=256)
    eng = model.engine
    tables = backend == 'fused' and eng.get_option('pow_tabs') == 1
    ordinary = helpers.ordinary_walkers(shape[0], shape[1], 8, seed=1)
    alone = model.log_likelihood_batch(ordinary)
    assert np.isfinite(alone).all() and len(np.unique(alone)) == len(alone)
    # the extreme walkers by themselves, in batches small enough for the row waves to form their own tables
    last = n_ext
    if tables:
        last = 8192 // (3 * int(eng.get_option('partials_per_walker')))     # walkers of the last such batch
        assert 8 < last < 256, last
    ext = []
    for lo in range(0, n_ext, min(last, n_ext)):
        ext.append(model.log_likelihood_batch(theta[lo:lo + min(last, n_ext)]))
        if tables:
            assert eng.get_option('pow_tabs_built') == 0, (tag, lo)
    ext = np.concatenate(ext)
    on_pixel = np.array(['on_pixel' in inf['flags'] for inf in info])
    assert np.all(ext[on_pixel] == -np.inf) and np.isfinite(ext[~on_pixel]).all(), \
        (tag, [info[i]['name'] for i in np.flatnonzero(np.isfinite(ext) == on_pixel)])
    if tables:
        pad = helpers.ordinary_walkers(shape[0], shape[1], max(last + 1 - n_ext, 0) + 8, seed=2)
        big = np.vstack([theta, pad])
        assert last < len(big) <= 256
        got = model.log_likelihood_batch(big)
        assert eng.get_option('pow_tabs_built') == 1, tag
        assert np.array_equal(got[:n_ext], ext), (tag, 'table source',
                                                  [info[i]['name'] for i in np.flatnonzero(got[:n_ext] != ext)])
        assert np.isfinite(got[n_ext:]).all()
    # the mixed batch: ordinary walkers before and after the extreme ones (a small batch again where it fits)
    mixed = np.vstack([ordinary[:4], theta, ordinary[4:]])
    want = np.concatenate([alone[:4], ext, alone[4:]])
    got = model.log_likelihood_batch(mixed)
    assert np.array_equal(got, want), (tag, 'mixed batch', np.flatnonzero(got != want))
    perm = np.random.RandomState(len(tag) + shape[1]).permutation(len(mixed))
    assert np.array_equal(model.log_likelihood_batch(mixed[perm]), want[perm]), (tag, 'permutation')
    # extreme and ordinary walkers interleaved one by one, in passes of at most two: an extreme record shares its
    # pass with an ordinary one
    inter = np.vstack([np.vstack([theta[i], ordinary[i % 8]]) for i in range(n_ext)])
    want_inter = np.ravel(np.column_stack([ext, alone[np.arange(n_ext) % 8]]))
    default = int(eng.get_option('chunk_walkers')) if backend == 'fused' else None
    assert np.array_equal(model.log_likelihood_batch(inter), want_inter), (tag, 'interleaved')
    if backend == 'fused':
        assert several_passes(model, len(inter)) <= 2
        got = model.log_likelihood_batch(inter)
        eng.set_option('chunk_walkers', default)
        assert np.array_equal(got, want_inter), (tag, 'passes of two', np.flatnonzero(got != want_inter))
    model.close()


SCALE_FORMS = [f for f in RASTER_FORMS if f[0] in ('logexp-256', 'g4-288')]


@pytest.mark.parametrize('form', SCALE_FORMS, ids=[f[0] for f in SCALE_FORMS])
def test_scale_of_the_variance_channel_with_sources_off_the_image(form):
    """prep_head scales raw^2 (the imaginary part of the one complex transform) by a power of two from a PEAK
    ESTIMATE per component -- a Sersic's brightness half a pixel from its centre, a point source's |flux| --
    whether or not that point is on the image.  A bright component centred off the image makes the estimate exceed
    every pixel by orders of magnitude, and each order costs the variance channel a digit.  Three such walkers, each
    beside an ordinary faint Sersic (raw peak of order 1): the weight map and the log-likelihood against the
    long-double evaluation, no farther from it than 4 x the fp64 oracle itself + 1e-11 of the map's scale
    (test_general_sides_match_oracle's rule) and + the 5e-12 of the log-likelihood's terms that fuzz_bound allows."""
    import psfmc_oracle as orc
    import test_gpu_random as tgr
    tag, shape = form[0], form[1]
    failures = []
    for name, method, theta in helpers.scale_walkers(*shape):
        case = helpers.extreme_case(shape, form[2], ps_method=method)
        field = helpers.extreme_field(case)
        layout = case['layout']
        comps, psf = helpers.comps_from_theta(layout, theta)
        ll_orc, imgs = orc.evaluate(field, comps, psf, raw_dtype=np.float64)
        assert np.isfinite(ll_orc), (tag, name)
        raw, ref = imgs['raw_model'], imgs['composite_ivm']
        # the scale case is one: the faint Sersic's peak is of order 1 and the estimate exceeds the image's peak
        model = open_model(form, case, max_walkers=4)
        both = np.vstack([theta, theta])
        got = model.log_likelihood_batch(both)
        dev = model.sample_images(both, ('composite_ivm', 'raw_model'))
        model.close()
        assert got[0] == got[1]
        exact_ivm, ll_exact, cond = helpers.longdouble_loglike(field, raw, psf)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(dev['composite_ivm'][0]), fin), (tag, name)
        scale = max(np.abs(ref[fin]).max(), 1e-300)
        e_orc = float(np.abs(ref[fin].astype(np.longdouble) - exact_ivm[fin]).max())
        e_gpu = float(np.abs(dev['composite_ivm'][0][fin].astype(np.longdouble) - exact_ivm[fin]).max())
        l_orc, l_gpu = abs(float(ll_orc - ll_exact)), abs(float(got[0] - ll_exact))
        print('RASTER-SCALE %-10s %-16s raw peak %.3g | ivm e_orc %.2e e_gpu %.2e (of scale) | ll %.10g e_orc %.2e '
              'e_gpu %.2e terms %.3g' % (tag, name, np.abs(raw).max(), e_orc / scale, e_gpu / scale, got[0], l_orc,
                                         l_gpu, cond))
        if not e_gpu <= 4.0 * e_orc + 1e-11 * scale:
            failures.append((name, 'composite_ivm', e_gpu / scale, e_orc / scale))
        if not l_gpu <= 4.0 * l_orc + 5e-12 * cond:
            failures.append((name, 'log-likelihood', l_gpu, l_orc, 5e-12 * cond))
    assert not failures, (tag, failures)
