"""The general components at the extremes a Uniform prior allows (tests/general_extremes.py: boxiness -1.9 ... 10,
Fourier amplitudes summing to 0.99, spiral ramps a hundredth of a pixel wide, windings of 1e6 degrees, Moffat beta
1.0001 ... 500, Ferrer beta 1.999 ... -50, truncation ramps 1e-3 px wide and beyond the image, bending amplitudes of 3
at q = 0.01, centres on, beside and far off the pixels, magnitudes 8 and 60), each extreme in one of two general slots
with ordinary or dark neighbours, on the seven instantiations a context's general launches take (GenLevel of
psfmc_hip.hip, `GEN_PLAIN ... GEN_BND`) and the three of the pixel-mean kernels.

A family runs at the lowest level whose kernels have its block, every family again at GEN_BND -- its model beside a
dark component that carries a bending mode, so that the family's blocks are wave-uniform branches of the deepest
kernel -- and the Fourier and spiral families at GEN_FOU_SPI.  Held to: a long-double evaluation of the raw model per
pixel (bound max(1e-11, 4 x the fp64 definition's own error against it)), its finiteness pattern, the contract's
log-likelihood (`fuzz_shapes.fuzz_bound`), finiteness on the hipFFT back end, and -- device against device, bit for
bit -- independence of the walkers a walker is batched with, of their order and of the pass size.  The pixel-mean
kernels are held to the fp64 definition `Sersic.general_mean_image` at the bound of tests/test_gpu_general_mean.py: no
definition of the pixel mean finer than fp64 exists.  tests/test_general_extremes_reference.py holds the references
and the conditions that keep these checks from passing emptily, without a GPU."""
import numpy as np
import pytest

import general_extremes as ge
from general_extremes import EMBEDDED, FAMILIES, LEVELS, SHAPE

pytestmark = pytest.mark.gpu

BELOW_FLOOR_MAX = 1e-279
# (level, the families run there): its own families, the Fourier and spiral ones together, everything at the deepest
LEVEL_RUNS = [(lv, tuple(f for f, (_, _, own) in FAMILIES.items() if own == lv)) for lv in LEVELS[:3]] + \
             [('fou+spi', ('fou', 'spi'))] + \
             [(lv, tuple(f for f, (_, _, own) in FAMILIES.items() if own == lv)) for lv in LEVELS[4:6]] + \
             [('bnd', tuple(FAMILIES))]
LEVEL_CASES = [(lv, fam, SHAPE) for lv, fams in LEVEL_RUNS for fam in fams] + [('bnd', fam, EMBEDDED) for fam in FAMILIES]
# the pixel-mean kernels' three instantiations: contexts up to GEN_RAD, GEN_TRU, GEN_BND
MEAN_RUNS = [('rad', ('box', 'spi', 'mof', 'fer')), ('tru', ('tru', 'spi')), ('bnd', tuple(FAMILIES))]
MEAN_CASES = [(lv, fam) for lv, fams in MEAN_RUNS for fam in fams]
AUX_PER_SERSIC = {'plain': 1, 'fou': 13, 'spi': 19, 'fou+spi': 19, 'rad': 21, 'tru': 25, 'bnd': 29}
case_id = lambda v: '%dx%d' % v if isinstance(v, tuple) else str(v)


def open_model(family, level, fld, max_walkers, backend='fused', mean=False):
    """The family's model in a context of `level`, with the proof of the level: the model's block tags and the
    doubles per walker of the context's auxiliary vectors."""
    model = ge.build_model(fld, family, level, mean=mean, backend=backend, max_walkers=max_walkers)
    assert model._backend == backend and ge.level_of(model) == level, (family, level, ge.level_of(model))
    n_sersic = len(model.sersic_general_flags)
    assert n_sersic == 2 + int(level != FAMILIES[family][2])
    assert model.aux_rows(np.zeros((1, model.num_params))).shape[1] == 2 + AUX_PER_SERSIC[level] * n_sersic
    return model


@pytest.mark.parametrize('level,family,shape', LEVEL_CASES, ids=case_id)
def test_extremes_match_references(level, family, shape):
    """Every walker of the family's list: raw model per pixel against the long-double evaluation, finiteness patterns,
    pixels below the floor, the log-likelihood against the contract, and finiteness on the other back end.  MEASURED
    worst per family and level: DESIGN.md section 34."""
    refs = ge.extreme_references(family, shape=shape)
    theta, info = refs['theta'], refs['info']
    model = open_model(family, level, refs['fld'], max_walkers=len(theta))
    got = model.log_likelihood_batch(theta)
    assert int(model.engine.get_option('aux_stride')) == 2 + AUX_PER_SERSIC[level] * len(model.sersic_general_flags)
    raw = model.sample_images(theta, ('raw_model',))['raw_model']
    model.close()
    assert raw.shape == (len(theta),) + tuple(shape)
    failures, worst = [], (0.0, None)
    for i, inf in enumerate(info):
        who = '%s/%s/slot%d' % (inf['name'], inf['kind'], inf['slot'])
        exact, want = refs['exact'][i], refs['ll'][i]
        # the conditions the CPU companion checks, on this shape's own references
        assert np.isfinite(want) == ('on_pixel' not in inf['flags']), (family, who, want)
        assert (refs['n_rel'][i] >= 500 or 'below_floor' in inf['flags'] or
                (inf['kind'] == 'solo' and inf['name'] in ge.FEW_PIXELS)), (family, who)
        rel, n_rel, low = ge.general_pixel_errors(raw[i], exact, refs['sigma0'][i], refs['edge'][i])
        ll_err = abs(got[i] - want) if np.isfinite(want) and np.isfinite(got[i]) else float('nan')
        print('GENERAL-EXTREME %-7s %-4s %dx%d %-30s e_def %.2e e_dev %.2e bound %.2e px %5d low %.1e | ll %.10g err %.2e '
              'bound %.2e' % ((level, family) + tuple(shape) + (who, refs['e_def'][i], rel, refs['bound'][i], n_rel, low,
                                                                 got[i], ll_err, refs['ll_bound'][i])))
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
        if rel > worst[0]:
            worst = (rel, who)
    print('GENERAL-EXTREME-WORST %-7s %-4s %dx%d e_dev %.2e (%s) e_def %.2e'
          % ((level, family) + tuple(shape) + worst + (refs['e_def'].max(),)))
    assert not failures, (level, family, failures)
    # the other back end: finite exactly where this one is
    other = open_model(family, level, refs['fld'], max_walkers=len(theta), backend='hipfft')
    theirs = other.log_likelihood_batch(theta)
    other.close()
    assert np.array_equal(np.isfinite(theirs), np.isfinite(got)), \
        (level, family, [info[i]['name'] for i in np.flatnonzero(np.isfinite(theirs) != np.isfinite(got))])


_MEAN_REFS = {}


def mean_references(family):
    """The fp64 definition of the reduced list's walkers rendered as pixel means (`Sersic.general_mean_image` through
    `add_to_array`), once per process: (fld, field, theta, info, [(log-likelihood, images, Sigma_0)])."""
    if family not in _MEAN_REFS:
        import extra_contract as xc
        import test_gpu_general_components as tgg
        import test_gpu_general_mean as tgm
        fld = tgg.make_field(*SHAPE, seed=31)
        field = tgg.oracle_field(fld)
        model = ge.build_model(fld, family, mean=True, backend='hipfft', max_walkers=1)
        theta, info = ge.extreme_walkers(model, family, names=ge.MEAN_CASES)
        want = []
        for t in theta:
            ll, imgs = tgg.contract_evaluate(model, field, t)
            sigma0, margin = tgm.mean_ferrer_state(model)
            assert margin >= xc.EDGE_MARGIN and np.isfinite(ll), (family, margin, ll)
            want.append((ll, imgs, sigma0))
        _MEAN_REFS[family] = (fld, field, theta, info, want)
    return _MEAN_REFS[family]


@pytest.mark.parametrize('level,family', MEAN_CASES, ids=case_id)
def test_pixel_mean_kernels_at_the_extremes(level, family):
    """The reduced list (`general_extremes.MEAN_CASES`: the spiral ramps, truncation tails, bending, one case of each
    law) with `pixel_mean=True` on both slots, on the three instantiations of k_general_mean_rows / _core.  Held to THE
    FP64 DEFINITION `Sersic.general_mean_image` -- there is none finer -- at the bound of tests/test_gpu_general_mean.py:
    RAW_BOUND per pixel (relative to the pixel above 1e-12 of the peak, to Sigma_0 with a Ferrer), finite everywhere,
    and the log-likelihood at `fuzz_bound`."""
    import extra_contract as xc
    import fuzz_shapes
    import test_gpu_general_components as tgg
    fld, field, theta, info, want_all = mean_references(family)
    assert len(theta) >= 2
    own = FAMILIES[family][2]
    run_level = own if level == 'rad' else level
    assert LEVELS.index(own) <= LEVELS.index(level)
    model = open_model(family, run_level, fld, max_walkers=len(theta), mean=True)
    assert model.sersic_general_mean[:2] == [True, True]
    got = model.log_likelihood_batch(theta)
    raw = model.sample_images(theta, ('raw_model',))['raw_model']
    model.close()
    failures = []
    for i, (inf, (want_ll, want, sigma0)) in enumerate(zip(info, want_all)):
        who = '%s/%s/slot%d' % (inf['name'], inf['kind'], inf['slot'])
        if not np.all(np.isfinite(raw[i])):
            failures.append((who, 'not finite', int((~np.isfinite(raw[i])).sum())))
            continue
        tag = 'GENERAL-EXTREME-MEAN %-4s %-4s %s' % (level, family, who)
        err = xc.law_error(raw[i], want['raw_model'], sigma0, tag) if sigma0 else tgg.raw_error(raw[i], want['raw_model'], tag)
        bound = fuzz_shapes.fuzz_bound(field, want, want_ll)
        print('%s: log-likelihood %.10g err %.2e bound %.2e' % (tag, got[i], abs(got[i] - want_ll), bound))
        if not err <= tgg.RAW_BOUND:
            failures.append((who, 'raw model per pixel', err))
        if not abs(got[i] - want_ll) <= bound:
            failures.append((who, 'log-likelihood', got[i], want_ll, bound))
    assert not failures, (level, family, failures)


@pytest.mark.parametrize('family', list(FAMILIES))
def test_extremes_do_not_depend_on_the_batch(family):
    """Device against device, bit for bit, at the deepest level: the ordinary walkers of a mixed batch return what they
    return without the extreme ones (a NaN or an inf in one record must not reach another), under a permutation, and
    in passes of at most two walkers, an extreme record sharing its pass with an ordinary one."""
    from test_gpu_random import several_passes
    import test_gpu_general_components as tgg
    fld = tgg.make_field(*SHAPE, seed=31)
    model = open_model(family, 'bnd', fld, max_walkers=256)
    theta, info = ge.extreme_walkers(model, family)
    n_ext = len(theta)
    ordinary = ge.ordinary_walkers(model, family, 8, seed=1)
    alone = model.log_likelihood_batch(ordinary)
    assert np.isfinite(alone).all() and len(np.unique(alone)) == len(alone)
    ext = model.log_likelihood_batch(theta)
    on_pixel = np.array(['on_pixel' in inf['flags'] for inf in info])
    assert np.all(ext[on_pixel] == -np.inf) and np.isfinite(ext[~on_pixel]).all(), \
        (family, [info[i]['name'] for i in np.flatnonzero(np.isfinite(ext) == on_pixel)])
    mixed = np.vstack([ordinary[:4], theta, ordinary[4:]])
    want = np.concatenate([alone[:4], ext, alone[4:]])
    got = model.log_likelihood_batch(mixed)
    assert np.array_equal(got, want), (family, 'mixed batch', np.flatnonzero(got != want))
    perm = np.random.RandomState(len(family) + n_ext).permutation(len(mixed))
    assert np.array_equal(model.log_likelihood_batch(mixed[perm]), want[perm]), (family, 'permutation')
    inter = np.vstack([np.vstack([theta[i], ordinary[i % 8]]) for i in range(n_ext)])
    want_inter = np.ravel(np.column_stack([ext, alone[np.arange(n_ext) % 8]]))
    default = int(model.engine.get_option('chunk_walkers'))
    assert np.array_equal(model.log_likelihood_batch(inter), want_inter), (family, 'interleaved')
    assert several_passes(model, len(inter)) <= 2
    got = model.log_likelihood_batch(inter)
    model.engine.set_option('chunk_walkers', default)
    assert np.array_equal(got, want_inter), (family, 'passes of two', np.flatnonzero(got != want_inter))
    model.close()
