"""The references of tests/test_gpu_raster_extremes.py, and the conditions that keep its checks from passing emptily,
without a GPU: the long-double Sersic against the fp64 oracle, the per-pixel bound's rule, how many pixels every case
puts into the relative check, which oracle likelihoods are finite, and the table of rasteriser forms."""
import os
import re

import numpy as np
import pytest

import helpers
import psfmc_oracle as orc

needs_longdouble = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63,
                                      reason='numpy longdouble is not the 80-bit x87 type on this platform')
# the quick shapes (0.4 ... 0.7 s of references each); the device test asserts the same conditions on every shape's own
# references before it looks at the device's output
CPU_FORMS = ['logexp-64', 'g4-288', 'wrap-logexp']


def test_form_table_covers_every_rasteriser():
    helpers.check_raster_form_coverage()


def test_device_test_runs_every_case_on_every_shape():
    """No case of the device test is left out or excused: it is parametrised over the whole table and carries no
    marks but `gpu`."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_gpu_raster_extremes.py')
    with open(path) as f:
        text = f.read()
    assert not re.search(r'skip|xfail|importorskip', text)
    assert text.count("@pytest.mark.parametrize('form', RASTER_FORMS, ids=FORM_IDS)") == 2
    names = [s[0] for s in helpers.extreme_specs(64, 288)]
    assert len(names) == len(set(names)) and 30 <= len(names) <= 40
    for want in ('n0.1', 'n0.3', 'n8', 'n15', 'reff-tiny', 'reff-huge', 'round', 'q0.01', 'q0.01-n0.1', 'q0.01-n15',
                 'ang0', 'ang90', 'ang180', 'ang270', 'ang-90', 'ang1e6', 'corner', 'near-pixel', 'on-pixel',
                 'off-corner-n6', 'left5', 'mag8', 'mag35', 'mag60', 'tab-low', 'tab-high'):
        assert want in names, want
    # every extreme sits in each of the three slots on some walker of the list: first, middle, last
    theta, info = helpers.extreme_walkers(64, 288)
    assert theta.shape == (2 * len(names), 25)
    assert {inf['slot'] for inf in info} == {0, 1, 2}
    assert {(inf['name'], inf['kind']) for inf in info} == {(n, k) for n in names for k in ('mixed', 'solo')}


@needs_longdouble
def test_longdouble_sersic_agrees_with_the_oracle_at_ordinary_parameters():
    """A typo in the long-double text would inflate e_orc and with it the device's bound: at ordinary parameters the
    two agree to a few ulps where the profile is bright, and the error further out is the exponent's (kappa rho^(1/n)
    ulps, 1e-13 class at exp(-500))."""
    shape = (64, 288)
    for s in helpers.extreme_slots(*shape):
        args = (tuple(s[5:7]), s[2], s[3], s[4], s[1], s[0], True, helpers.EXTREME_ZP)
        exact = helpers.longdouble_sersic(shape, *args)
        got = orc.add_sersic(np.zeros(shape), *args, coords=orc.array_coords(shape))
        rel = np.abs(got.astype(np.longdouble) - exact) / np.abs(exact)
        bright = exact > 1e-6 * exact.max()
        assert bright.sum() > 500
        assert float(rel[bright].max()) <= 2e-14, float(rel[bright].max())
        assert float(rel.max()) <= 5e-13, float(rel.max())
    # the walkers' images: sky + point source + three ordinary slots, 1e-15 class
    refs = helpers.extreme_references('g4-288')
    assert refs['info'][0]['name'] == 'base' and refs['e_orc'][0] <= 1e-14


@needs_longdouble
@pytest.mark.parametrize('tag', CPU_FORMS)
def test_conditions_of_the_extreme_cases(tag):
    refs = helpers.extreme_references(tag)
    info = refs['info']
    short = set()
    for i, inf in enumerate(info):
        who = (tag, inf['name'], inf['kind'])
        exact = refs['exact'][i]
        # the bound's rule, and a cap on what the oracle's own error may turn it into (the worst case is q = 0.01
        # with n = 0.1: 3e-12 ... 2e-11 on these fields, 6e-11 with the line along other pixels)
        assert refs['bound'][i] == max(1e-11, 4.0 * refs['e_orc'][i]) and refs['e_orc'][i] <= 1e-10, who
        # the oracle's likelihood is finite for every walker but the on-pixel centre, whose raw model is NaN at
        # that pixel and only there
        assert np.isfinite(refs['ll'][i]) == ('on_pixel' not in inf['flags']), who
        nan = ~np.isfinite(exact)
        assert nan.sum() == int('on_pixel' in inf['flags']), who
        assert np.array_equal(nan, ~np.isfinite(refs['images'][i]['raw_model'])), who
        if nan.any():
            assert nan[refs['shape'][0] // 2, int(refs['shape'][1] * 0.5)], who
        # at least 500 pixels in the relative check, the named exceptions apart (solo walkers only)
        if refs['n_rel'][i] < 500:
            assert inf['kind'] == 'solo' and inf['name'] in helpers.FEW_PIXELS, who
            short.add(inf['name'])
        if 'below_floor' in inf['flags'] and inf['kind'] == 'solo':
            assert refs['n_rel'][i] == 0 and float(np.abs(exact).max()) <= helpers.RASTER_FLOOR, who
        if inf['kind'] == 'mixed':
            assert refs['n_rel'][i] >= exact.size - 1, who
    assert short == set(helpers.FEW_PIXELS), short          # (the list holds no stale entry)
    # the log-likelihood bound: fuzz_bound, the near-pixel case's 1e-5 apart
    for i, inf in enumerate(info):
        if np.isfinite(refs['ll'][i]):
            rel = refs['ll_bound'][i] / abs(refs['ll'][i])
            assert (rel == pytest.approx(1e-5)) if 'near_pixel' in inf['flags'] else (2e-10 <= rel * (1 + 1e-12) and rel < 1e-7), \
                (tag, inf['name'], rel)


@needs_longdouble
def test_scale_walkers_are_scale_cases():
    """The faint Sersic's raw peak is of order 1 and the component off the image adds a peak estimate (prep_head's:
    the brightness half a pixel from a Sersic's centre along the minor axis, a point source's flux) orders of
    magnitude above it; the fp64 oracle's own weight map and likelihood sit where the device's bound needs them."""
    f = [f for f in helpers.RASTER_FORMS if f[0] == 'g4-288'][0]
    for name, method, theta in helpers.scale_walkers(*f[1]):
        case = helpers.extreme_case(f[1], f[2], ps_method=method)
        field = helpers.extreme_field(case)
        comps, psf = helpers.comps_from_theta(case['layout'], theta)
        ll, imgs = orc.evaluate(field, comps, psf, raw_dtype=np.float64)
        assert np.isfinite(ll), name
        est = 0.0
        for c in comps:
            if c['type'] == 'ps':
                est = max(est, orc.mag_to_flux(c['mag'], field.mag_zp))
            elif c['type'] == 'sersic':
                kappa = orc.sersic_kappa(c['index'])
                sb = orc.sersic_sb_eff(orc.mag_to_flux(c['mag'], field.mag_zp), c['index'], c['reff'], c['reff_b'], kappa)
                est = max(est, sb * np.exp(-kappa * np.expm1(np.log(0.25 / c['reff_b'] ** 2) * 0.5 / c['index'])))
        raw = imgs['raw_model']
        assert 0.5 < raw.max() < 2.0, (name, raw.max())
        assert est > 1e3 * raw.max(), (name, est)
        ivm, ll_exact, cond = helpers.longdouble_loglike(field, raw, psf)
        fin = np.isfinite(imgs['composite_ivm'])
        scale = np.abs(imgs['composite_ivm'][fin]).max()
        e_orc = float(np.abs(imgs['composite_ivm'][fin] - ivm[fin]).max())
        if name != 'ps-off-bilinear':
            # (the bilinear weights of a source 10 px outside are -1e6 counts on two edge pixels: the oracle's own
            # weight map is 1e-7 from the long-double one there)
            assert e_orc <= 1e-14 * scale and abs(float(ll - ll_exact)) <= 5e-12 * cond, (name, e_orc / scale)
