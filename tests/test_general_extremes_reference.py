"""The references of tests/test_gpu_general_extremes.py, and the conditions that keep its checks from passing emptily,
without a GPU: the long-double evaluation of a general component (tests/general_extremes.py) against the fp64 numpy
definition at ordinary values and against mpmath at 50 digits on single pixels of the extreme list, the extreme list
itself, the per-pixel bound's rule, how many pixels every case puts into the relative check, and the cap on the cases
whose bound the definition's own error loosens."""
import os
import re

import numpy as np
import pytest

import general_extremes as ge
import helpers
from psfmc_amd.ModelComponents import Sersic

needs_longdouble = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63,
                                      reason='numpy longdouble is not the 80-bit x87 type on this platform')
FAMILIES = list(ge.FAMILIES)


def test_the_list_covers_the_families_and_the_device_test_runs_all_of_it():
    specs = ge.general_extreme_specs(*ge.SHAPE)
    names = [s[0] for s in specs]
    assert len(names) == len(set(names)) and len(names) >= 70
    assert {s[1] for s in specs} == set(ge.FAMILIES)
    for want in ('c-1.9', 'c-1.5', 'c0', 'c3', 'c10', 'c3-q0.01', 'fou-one-0.99', 'fou-six-0.99', 'fou-m6-0.9', 'fou-phase0',
                 'fou-phase90', 'fou-phase1e6', 'fou-amp0', 'fou-amp1e-300', 'spi-ramp100', 'spi-ramp172', 'spi-ramp181',
                 'spi-ramp182', 'spi-ramp2000', 'spi-rin0', 'spi-rout1e4', 'spi-wind1e4', 'spi-wind1e6', 'spi-alpha0',
                 'spi-alpha1e-3', 'spi-alpha5', 'spi-incl89.9', 'spi-on-pixel-alpha0', 'spi-on-pixel-alpha1',
                 'mof-beta1.0001', 'mof-beta1.5', 'mof-beta50', 'mof-beta500', 'mof-fwhm0.05', 'mof-fwhm3000', 'mof-q0.01',
                 'fer-alpha0', 'fer-alpha0.01', 'fer-alpha20', 'fer-beta1.999', 'fer-beta-50', 'fer-rout0.3', 'fer-rout3000',
                 'tru-in-1e-3', 'tru-out-1e-3', 'tru-lo0', 'tru-hi1e6', 'tru-out-first-pixel', 'tru-in-beyond',
                 'tru-overlap', 'bnd-a4+3-q0.01', 'bnd-a4-3-q0.01', 'bnd-ridge', 'bnd-a1-3', 'bnd-amp0', 'bnd-amp1e-300',
                 'bnd-a2-3-c3', 'ser-on-pixel', 'ser-near-pixel', 'ser-left5', 'mof-on-pixel', 'mof-near-pixel', 'mof-left5',
                 'fer-on-pixel', 'fer-near-pixel', 'fer-left5', 'ser-mag8', 'ser-mag60', 'mof-mag8', 'mof-mag60', 'fer-mag8',
                 'fer-mag60'):
        assert want in names, want
    by_name = {s[0]: s for s in specs}
    # the ramp of the issue: r_in = 9, r_out = 9.1, the exponent at r = 0 above fast_exp2's 1024
    over = by_name['spi-ramp181'][2]
    assert (over['spiral_r_in'], over['spiral_r_out']) == (9.0, 9.1)
    ratio = lambda o: (o['spiral_r_in'] + o['spiral_r_out']) / (o['spiral_r_out'] - o['spiral_r_in'])
    assert [round(ratio(by_name['spi-ramp%d' % r][2])) for r in (100, 172, 181, 182, 2000)] == [100, 172, 181, 182, 2000]
    assert 4.0 * np.log2(np.e) * ratio(over) > 1024 > 4.0 * np.log2(np.e) * ratio(by_name['spi-ramp172'][2])
    assert set(ge.MEAN_CASES) <= set(names) and set(ge.FEW_PIXELS) <= set(names) and set(ge.LOOSENED) <= set(names)
    # the device test: no case left out or excused, every level and the three mean instantiations
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_gpu_general_extremes.py')
    with open(path) as f:
        text = f.read()
    assert not re.search(r'skip|xfail|importorskip', text)
    import test_gpu_general_extremes as dev
    assert [lv for lv, _ in dev.LEVEL_RUNS] == list(ge.LEVELS)
    runs = dict(dev.LEVEL_RUNS)
    for fam, (_, _, own) in ge.FAMILIES.items():
        assert fam in runs[own] and fam in runs['bnd'], fam           # its own level, and the deepest one
    assert set(runs['fou+spi']) == {'fou', 'spi'}
    assert [lv for lv, _ in dev.MEAN_RUNS] == ['rad', 'tru', 'bnd']
    mean = dict(dev.MEAN_RUNS)
    assert {'box', 'spi', 'mof', 'fer'} <= set(mean['rad']) and 'tru' in mean['tru'] and set(mean['bnd']) == set(ge.FAMILIES)


def test_every_family_reaches_its_level_and_the_lifted_ones():
    """The models: two slots of the family's class with every keyword value free, and the dark third component that
    lifts a context to a deeper level; the level is read from the model's own block tags."""
    import test_gpu_general_components as tgg
    fld = tgg.make_field(*ge.SHAPE, seed=31)
    for fam, (cls, keys, own) in ge.FAMILIES.items():
        model = ge.build_model(fld, fam, backend='hipfft', max_walkers=1)
        assert ge.level_of(model) == own and len(model.sersic_general_flags) == 2 and all(model.sersic_general_flags), fam
        for level in ge.LEVELS[ge.LEVELS.index(own) + 1:]:
            if level not in ge.LIFTS or (isinstance(ge.LIFTS[level], dict) and fam not in ge.LIFTS[level]):
                continue
            lifted = ge.build_model(fld, fam, level, backend='hipfft', max_walkers=1)
            assert ge.level_of(lifted) == level and lifted.param_names == model.param_names, (fam, level)
            assert len(lifted.sersic_general_flags) == 3
        mean = ge.build_model(fld, fam, mean=True, backend='hipfft', max_walkers=1)
        assert mean.sersic_general_mean == [True, True] and mean.param_names == model.param_names
        theta, info = ge.extreme_walkers(model, fam)
        n = len(ge.specs_of(fam))
        assert theta.shape == (2 * n, model.num_params) and {i['slot'] for i in info} == {0, 1}
        assert {(i['name'], i['kind']) for i in info} == {(s[0], k) for s in ge.specs_of(fam) for k in ('mixed', 'solo')}
        assert np.all(np.isfinite(model.log_priors_batch(theta))), fam             # inside every prior
        assert np.all(np.isfinite(model.log_priors_batch(ge.ordinary_walkers(model, fam, 8, seed=1))))


def test_the_bending_ridge_runs_through_pixel_centres():
    """bnd-ridge: v' = v + a_1 (r_a / r_b) u is EXACTLY 0 at the centres of the diagonal pixels, in the rows the device
    is handed (`derived_rows`: an angle of -90 degrees gives m01 = m10 = 0 exactly) and with the ratio as
    k_general_split forms it -- every factor a power of two, so no order of operations or fused multiply-add can make
    it 1e-17 instead: the `av > 0` select of general_pixel takes its other side on those pixels."""
    import test_gpu_general_components as tgg
    fld = tgg.make_field(*ge.SHAPE, seed=31)
    model = ge.build_model(fld, 'bnd', backend='hipfft', max_walkers=1)
    theta, info = ge.extreme_walkers(model, 'bnd', names=('bnd-ridge',))
    assert len(theta) == 2
    for t, inf in zip(theta, info):
        row = model.derived_rows(t[None])[0]
        at = 1 + 4 * len(model._ps) + 9 * inf['slot']              # (the sky's level, the point sources, the Sersic rows)
        x0, y0, m00, m01, m10, m11 = row[at:at + 6]
        assert (x0, y0, m00, m01, m10, m11) == (32.5, 32.5, 0.125, 0.0, 0.0, 0.25), (inf, row[at:at + 6])
        ratio = (1.0 / np.hypot(m00, m01)) / (1.0 / np.hypot(m10, m11))
        assert ratio == 2.0
        model.param_values = t
        comp = [c for c in model.components if isinstance(c, Sersic)][inf['slot']]
        assert dict(comp.bending_list())[1] == -1.0 and tuple(comp.derived_row(model.config.mag_zeropoint)[:6]) == tuple(row[at:at + 6])
        on_ridge = 0
        for py in range(ge.SHAPE[0]):
            for px in range(ge.SHAPE[1]):
                dx, dy = px - x0, py - y0
                u, v = m00 * dx + m01 * dy, m10 * dx + m11 * dy
                bent = v + (-1.0 * ratio) * u
                assert (bent == 0.0) == (px == py), (px, py, bent)
                on_ridge += int(bent == 0.0 and u != 0.0)
        assert on_ridge == ge.SHAPE[0]


@needs_longdouble
def test_longdouble_evaluation_agrees_with_the_definition_at_ordinary_values():
    """A typo in the long-double text would inflate e_def and with it the device's bound.  At the ordinary values of
    `test_gpu_bending.contract_sets` -- every law, dress, truncation and mode set of tests/test_gpu_bending.py, two
    walkers each -- the fp64 definition (`Sersic.bent_image`) agrees with it at the rounding level of fp64: where
    the component is above 1e-6 of its peak asserted at 5e-14 (a few 1e-14), over every pixel above 1e-30 of the peak
    at 5e-13 (the exponent's error, kappa rho^(1/n) ulps, as for the plain profile).  The measured figures are printed;
    they are between 1e-14 and 2e-14 and between 5e-14 and 9e-14, their digits those of the platform's libm."""
    import test_gpu_bending as tgb
    import test_gpu_general_components as tgg
    fld = tgg.make_field(64, 64, seed=1)
    worst_bright, worst_all, n_comp = 0.0, 0.0, 0
    for n_set, (comps, cases) in enumerate(tgb.contract_sets(fld)):
        model = tgb.build(fld, comps, backend='hipfft', degrees=True, slope=(n_set % 2 == 1), max_walkers=2)
        for i, v in enumerate(cases):
            model.param_values = tgb.vector(model, fld, v, adu=0.05 + 0.002 * i)
            for comp in model.components:
                if not isinstance(comp, Sersic) or comp.pixel_mean:
                    continue
                args = ge.component_args(comp, model.config.mag_zeropoint)
                exact, _ = ge.longdouble_general(*args, shape=(64, 64))
                with np.errstate(all='ignore'):
                    got = Sersic.bent_image(*args, shape=(64, 64))
                assert np.array_equal(np.isfinite(got), np.isfinite(exact))
                fin = np.isfinite(exact)
                peak = float(np.abs(exact[fin]).max())
                scale = np.abs(exact)
                if comp.radial_law == 'ferrer':             # relative to Sigma_0 next to the cut-off, as law_error
                    scale = np.maximum(scale, np.longdouble(float(ge.walker_scalars(*args[:6])[1])))
                with np.errstate(all='ignore'):
                    rel = np.abs(got.astype(np.longdouble) - exact) / scale
                bright, some = fin & (np.abs(exact) > 1e-6 * peak), fin & (np.abs(exact) > 1e-30 * peak)
                assert bright.sum() >= 50, (n_set, i, type(comp).__name__)
                worst_bright = max(worst_bright, float(rel[bright].max()))
                worst_all = max(worst_all, float(rel[some].max()))
                n_comp += 1
    print('GENERAL-LONGDOUBLE %d components: definition against long double %.2e (bright), %.2e (above 1e-30 of the peak)'
          % (n_comp, worst_bright, worst_all))
    assert n_comp >= 20
    assert worst_bright <= 5e-14 and worst_all <= 5e-13, (worst_bright, worst_all)


# single pixels of the extreme list, one deep in each ramp's tail: (case, (x, y))
MPMATH_PIXELS = [('c-1.9', (40, 30)), ('c10', (10, 50)), ('fou-one-0.99', (30, 20)), ('fou-phase1e6', (50, 45)),
                 ('spi-ramp181', (24, 27)),        # inside r_in: the spiral ramp's lower tail, T = e^(-1400)
                 ('spi-ramp2000', (60, 5)), ('spi-wind1e4', (35, 40)), ('spi-alpha5', (30, 30)),
                 ('mof-beta500', (50, 40)), ('fer-beta1.999', (24, 27)),      # (inside the cut-off)
                 ('fer-alpha20', (25, 30)),
                 ('tru-in-1e-3', (28, 18)),        # 0.05 px inside an inner ramp 1e-3 px wide at 10: its tail, e^(-424)
                 ('tru-in-beyond', (30, 30)),      # the inner ramp's tail at 200 px: e^(-19)
                 ('tru-hi1e6', (60, 60)),          # the outer ramp's upper part, hi = 1e6
                 ('tru-overlap', (22, 27)),        # both tails at once
                 ('bnd-a4+3-q0.01', (23, 27)), ('bnd-a2-3-c3', (10, 10))]


@needs_longdouble
def test_longdouble_evaluation_agrees_with_mpmath_on_single_pixels():
    """The long-double image against the same formulas at 50 digits (the fp64 per-walker scalars as they are), on
    pixels of the extreme list's SOLO walkers.  Long double carries 64 bits: 5e-20 per operation, times the condition
    of the pixel -- the exponent kappa rho^(1/n), the winding in radians -- asserted at 1e-15, four orders inside the
    device's 1e-11; in a truncation ramp's tail the condition is the size of the ramp's two terms, and the bound follows
    it (below).  No pixel is exactly 0 or below long double's range: every one is compared."""
    pytest.importorskip('mpmath')
    import test_gpu_general_components as tgg
    fld = tgg.make_field(*ge.SHAPE, seed=31)
    tails = 0
    by_name = {s[0]: s for s in ge.general_extreme_specs(*ge.SHAPE)}
    for name, (x, y) in MPMATH_PIXELS:
        fam = by_name[name][1]
        model = ge.build_model(fld, fam, backend='hipfft', max_walkers=1)
        theta, info = ge.extreme_walkers(model, fam, names=(name,))
        solo = [i for i, inf in enumerate(info) if inf['kind'] == 'solo'][0]
        model.param_values = theta[solo]
        comp = [c for c in model.components if isinstance(c, Sersic)][info[solo]['slot']]
        args = ge.component_args(comp, model.config.mag_zeropoint)
        exact, _ = ge.longdouble_general(*args, shape=ge.SHAPE)
        want = ge.mpmath_general(*args, x=x, y=y)
        import mpmath as mp
        got = exact[y, x]
        # (every pixel is compared: none is exactly 0 or below long double's range, where nothing would be)
        assert want != 0 and abs(want) > mp.mpf(10) ** -4900 and got != 0, (name, want, got)
        with mp.workdps(50):
            mant, expo = np.frexp(got)                      # (exact, whatever the exponent: a tail is 1e-600)
            hi = float(mant)
            have = mp.ldexp(mp.mpf(hi) + mp.mpf(float(mant - np.longdouble(hi))), int(expo))
            err = float(abs(have - want) / abs(want))
        print('GENERAL-MPMATH %-16s (%2d, %2d) value %.3e err %.2e' % (name, x, y, float(got), err))
        # a ramp's exponent 2 (k1 rho + k0) is the difference of two terms of size 2 |k0| = 4 (lo + hi) / (hi - lo): the
        # rounding of the product, of the sum and a few ulps of rho, 4 x 2^-64 of that size, are its ABSOLUTE error and
        # so the factor's relative one -- 1.7e-14 for the ramp 1e-3 px wide at radius 10, below 1e-15 for every other
        bound = 1e-15
        if args[6] is not None:
            sides = [(args[6][k], args[6][k + 1]) for k in (0, 2) if args[6][k] is not None]
            bound = max([bound] + [4.0 * 2.0 ** -64 * 4.0 * (lo + hi) / (hi - lo) for lo, hi in sides])
        print('GENERAL-MPMATH %-16s bound %.2e' % (name, bound))
        assert err <= bound, (name, err, bound)
        tails += int(abs(float(got)) < 1e-6 * float(np.nanmax(np.abs(exact))))
    assert len(MPMATH_PIXELS) >= 12 and tails >= 4


@needs_longdouble
@pytest.mark.parametrize('family', FAMILIES)
def test_conditions_of_the_extreme_cases(family):
    """What the device test relies on, per family (at the family's own level; a lifted context adds a dark component
    that is exactly zero): printed per case and asserted."""
    refs = ge.extreme_references(family)
    info = refs['info']
    few, loose = set(), set()
    for i, inf in enumerate(info):
        who = (family, inf['name'], inf['kind'])
        exact, deff = refs['exact'][i], refs['images'][i]['raw_model']
        print('GENERAL-EXTREME-REF %-4s %-20s %-5s slot%d e_def %.2e bound %.2e px %4d edge %d%s'
              % (family, inf['name'], inf['kind'], inf['slot'], refs['e_def'][i], refs['bound'][i], refs['n_rel'][i],
                 int(refs['edge'][i].sum()), ' LOOSENED' if refs['e_def'][i] > ge.E_DEF_CAP else ''))
        # the reference is finite wherever the definition is, and NaN exactly at the on-pixel centre of a Sersic law
        nan = ~np.isfinite(exact)
        assert np.array_equal(nan, ~np.isfinite(deff)), who
        assert nan.sum() == int('on_pixel' in inf['flags']), who
        if nan.any():
            assert nan[ge.SHAPE[0] // 2, int(ge.SHAPE[1] * 0.5)], who
        assert np.isfinite(refs['ll'][i]) == ('on_pixel' not in inf['flags']), who
        if 'ramp' in inf['flags']:
            assert np.all(np.isfinite(exact)) and np.all(np.isfinite(deff)) and np.isfinite(refs['ll'][i]), who
        # the bound's rule
        assert refs['bound'][i] == max(ge.RAW_BOUND, helpers.RASTER_ORACLE_FACTOR * refs['e_def'][i]), who
        assert (ge.RAW_BOUND, helpers.RASTER_ORACLE_FACTOR) == (1e-11, 4.0)
        if refs['e_def'][i] > ge.E_DEF_CAP:
            loose.add(inf['name'])
        # the pixels in the check: every one of a mixed walker, at least 500 of a solo one but for the named cases; the
        # pixels left out next to a Ferrer's cut-off are a handful
        assert refs['edge'][i].sum() <= 8 and (refs['sigma0'][i] > 0) == (family == 'fer'), who
        if inf['kind'] == 'mixed':
            assert refs['n_rel'][i] >= exact.size - 1 - refs['edge'][i].sum(), who
        elif 'below_floor' in inf['flags']:
            assert refs['n_rel'][i] == 0 and float(np.abs(exact).max()) <= helpers.RASTER_FLOOR, who
        elif refs['n_rel'][i] < 500:
            assert inf['name'] in ge.FEW_PIXELS, who
            few.add(inf['name'])
        if np.isfinite(refs['ll'][i]):
            rel = refs['ll_bound'][i] / abs(refs['ll'][i])
            assert (rel == pytest.approx(1e-5)) if 'near_pixel' in inf['flags'] else (2e-10 <= rel * (1 + 1e-12) and rel < 1e-6), \
                (who, rel)
    names = {s[0] for s in ge.specs_of(family)}
    assert few == set(ge.FEW_PIXELS) & names, few                    # (the lists hold no stale entry)
    assert loose == set(ge.LOOSENED) & names, loose
    print('GENERAL-EXTREME-REF %-4s worst e_def %.2e, few pixels %s, loosened %s'
          % (family, refs['e_def'].max(), sorted(few), sorted(loose)))


def test_the_loosened_tenth():
    """At most one extreme in ten may have a definition farther than 1e-9 from the long-double image."""
    assert len(ge.LOOSENED) <= len(ge.general_extreme_specs(*ge.SHAPE)) // 10
    assert all(isinstance(v, str) and v for v in list(ge.LOOSENED.values()) + list(ge.FEW_PIXELS.values()))
