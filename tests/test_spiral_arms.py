"""Spiral arms on Sersic components by coordinate rotation (`Sersic(..., spiral={...})`) on the host: the numpy
definition (`Sersic.spiral_image`) and the keyword's way from a model file to the packed layout, the auxiliary, Fourier
and spiral layouts.  No GPU needed; the device is held to the same definition in tests/test_gpu_spiral_arms.py."""
import numpy as np
import pytest

import test_general_components as tg
import test_fourier_modes as tf
from psfmc_amd import MultiComponentModel
from psfmc_amd.ModelComponents import Sersic
from psfmc_amd.distributions import Normal, Uniform
from psfmc_amd.models import JointModel

SHAPE = (256, 256)
CENTRE = (127.3, 128.6)
MODES = [(2, 0.15, 0.5), (4, 0.1, -0.8)]
# the spiral sets of the flux check (r_in, r_out, winding, alpha, inclination, sky_angle): |winding| up to 8 rad,
# inclination up to 60 degrees, alpha in {0, 0.5, 1}
SPIRAL_SETS = [(4.0, 20.0, 2.0, 0.0, 0.0, 0.0),
               (0.0, 15.0, -8.0, 0.0, np.deg2rad(30.0), 0.7),
               (6.0, 30.0, 5.0, 0.5, np.deg2rad(45.0), -0.4),
               (2.0, 25.0, -3.0, 1.0, np.deg2rad(20.0), 1.2),
               (5.0, 18.0, 8.0, 0.0, np.deg2rad(60.0), 0.3)]
# MEASURED (n = 1, r_e = 12, r_b = 8, 256^2, centre (127.3, 128.6), angle 0.4): |image sum / (unrotated c = 0 sum) - 1|
# per set, (spiral alone, spiral with boxiness 0.7 and the two modes above) -- the pixel-centre sampling error of
# DESIGN.md sections 15 and 17, which grows with the foreshortening; asserted at twice the worse of a row
#   set 0  2.02e-7  2.95e-4
#   set 1  2.60e-4  1.47e-4
#   set 2  9.44e-4  5.32e-4
#   set 3  1.18e-4  2.13e-4
#   set 4  1.77e-3  1.55e-3
FLUX_WORST = [2.95e-4, 2.60e-4, 9.44e-4, 2.13e-4, 1.77e-3]
# MEASURED worst relative difference beyond 8 pixels between the saturated ramp and the plain component turned by the
# winding (winding 0.9, -2.3, 5.0; c = 0 and 0.7): 3.21e-14; asserted at ten times it
SATURATED_WORST = 3.21e-14


def row(x0=CENTRE[0], y0=CENTRE[1], reff=12.0, reff_b=8.0, index=1.0, angle=0.4):
    return Sersic(xy=(x0, y0), mag=18.0, reff=reff, reff_b=reff_b, index=index, angle=angle).derived_row(25.0)


# -- the definition ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', [0.0, 0.7, -1.0])
def test_zero_winding_is_the_general_and_the_fourier_image(c):
    spiral = (2.0, 9.0, 0.0, 0.5, 0.0, 0.0)
    for modes, want in (([], Sersic.general_image(row(), c, SHAPE)), (MODES, Sersic.fourier_image(row(), c, MODES, SHAPE))):
        got = Sersic.spiral_image(row(), c, modes, spiral, SHAPE)
        err = np.max(np.abs(got - want)) / want.max()
        print('c = %g, %d mode(s): zero-winding difference %.3e of the peak' % (c, len(modes), err))
        assert np.all(np.isfinite(want)) and err <= 1e-15


def test_saturated_ramp_is_the_component_turned_by_plus_the_winding():
    """alpha = 0, r_in = 0, r_out = 1, no inclination: beyond the ramp the image is the plain component at
    angle + winding -- not angle - winding: the sign, and the order of the rotation and the ellipse matrix."""
    yy, xx = np.mgrid[0:SHAPE[0], 0:SHAPE[1]].astype(np.float64)
    far = np.hypot(xx - CENTRE[0], yy - CENTRE[1]) > 8
    worst = 0.0
    for winding in (0.9, -2.3, 5.0):
        for c in (0.0, 0.7):
            got = Sersic.spiral_image(row(), c, [], (0.0, 1.0, winding, 0.0, 0.0, 0.0), SHAPE)
            plus = Sersic.general_image(row(angle=0.4 + winding), c, SHAPE)
            minus = Sersic.general_image(row(angle=0.4 - winding), c, SHAPE)
            err = np.max(np.abs(got - plus)[far] / plus[far])
            worst = max(worst, err)
            assert np.max(np.abs(got - minus)[far] / minus[far]) > 1.0, (winding, c)
    print('saturated ramp: worst relative difference beyond 8 pixels %.3e' % worst)
    assert 10 * SATURATED_WORST <= 1e-11 and worst <= 10 * SATURATED_WORST


@pytest.mark.parametrize('k', range(len(SPIRAL_SETS)))
def test_total_flux_does_not_depend_on_the_spiral(k):
    base = np.sum(Sersic.general_image(row(), 0.0, SHAPE))
    alone = abs(np.sum(Sersic.spiral_image(row(), 0.0, [], SPIRAL_SETS[k], SHAPE)) / base - 1)
    full = abs(np.sum(Sersic.spiral_image(row(), 0.7, MODES, SPIRAL_SETS[k], SHAPE)) / base - 1)
    print('set %d: flux closure %.3e alone, %.3e with boxiness 0.7 and two modes' % (k, alone, full))
    assert max(alone, full) <= 2 * FLUX_WORST[k]


def _position_angle(im, lo, hi):
    """Position angle (mod pi) of the second moments of `im` in the annulus lo <= r < hi around CENTRE."""
    yy, xx = np.mgrid[0:im.shape[0], 0:im.shape[1]].astype(np.float64)
    dx, dy = xx - CENTRE[0], yy - CENTRE[1]
    m = (np.hypot(dx, dy) >= lo) & (np.hypot(dx, dy) < hi)
    f, dx, dy = im[m], dx[m], dy[m]
    return 0.5 * np.arctan2(2 * np.sum(f * dx * dy), np.sum(f * dx * dx) - np.sum(f * dy * dy))


@pytest.mark.parametrize('winding', [0.8, 1.3, 2.0])
def test_a_positive_winding_turns_the_outer_isophotes_by_plus_the_winding(winding):
    """A bar (r_b / r_e = 0.3), alpha = 0: the position angle of the second moments beyond r_out exceeds the one
    inside r_in by the winding (mod pi).  MEASURED error 0.023, 0.021, 0.019 rad (the ramp is 0.018 at r_in, not 0):
    twice that is below 0.05 rad, which is the bound."""
    im = Sersic.spiral_image(row(reff=20.0, reff_b=6.0), 0.0, [], (10.0, 25.0, winding, 0.0, 0.0, 0.0), SHAPE)
    d = _position_angle(im, 32, 60) - _position_angle(im, 2, 8) - winding
    d = (d + 0.5 * np.pi) % np.pi - 0.5 * np.pi
    print('winding %.1f: position angle difference off by %.4f rad' % (winding, d))
    assert abs(d) <= 0.05


def test_on_pixel_centre_is_nan_and_r_zero_follows_alpha():
    for alpha in (0.0, 0.7):
        im = Sersic.spiral_image(row(100.0, 90.0), 0.0, [], (2.0, 9.0, 3.0, alpha, 0.3, 0.2), SHAPE)
        assert np.isnan(im[90, 100]) and np.isfinite(np.delete(im.ravel(), 90 * 256 + 100)).all()


# -- the component ---------------------------------------------------------------------------------------------------

def component(**kw):
    args = dict(xy=Uniform(loc=(20, 20), scale=(20, 20)), mag=18.0, reff=8.0, reff_b=5.0, index=1.0, angle=20.0,
                angle_degrees=True)
    args.update(kw)
    return Sersic(**args)


def test_packing_order_names_degrees_and_header_flags():
    s = component(boxiness=Uniform(loc=-1, scale=2),
                  spiral={'r_in': 2.0, 'r_out': Uniform(loc=5, scale=20), 'winding': Normal(loc=0, scale=200),
                          'sky_angle': Uniform(loc=-90, scale=180)})
    s.update_stochastic_names(2)
    assert s.free_names() == ['boxiness', 'spiral_r_out', 'spiral_sky', 'spiral_wind', 'xy']
    assert s.stochastic_names() == ['2_Sersic_boxiness', '2_Sersic_spiral_r_out', '2_Sersic_spiral_sky',
                                    '2_Sersic_spiral_wind', '2_Sersic_xy']
    assert s.stochastic_names('fitsname')[1:4] == ['2SER_SRO', '2SER_SPA', '2SER_SWD']
    assert s.has_spiral and s.is_general and s.header_flags(2) == {'2SERBOX': True, '2SERSPI': True}
    assert (s.spiral_r_in, s.spiral_alpha, s.spiral_incl) == (2.0, 0.0, 0.0)
    # the three angles are in degrees with angle_degrees
    vals = s._spiral_values(s.values_batch(np.array([[0.1, 12.0, 90.0, 180.0, 25.0, 25.0]])), 1)
    assert np.allclose(vals, [[2.0, 12.0, np.pi, 0.0, 0.0, 0.5 * np.pi]], rtol=1e-15)
    full = component(spiral={'r_in': Uniform(0, 5), 'r_out': Uniform(5, 20), 'winding': Uniform(-3, 6),
                             'alpha': Uniform(0, 2), 'inclination': Uniform(0, 60), 'sky_angle': Uniform(-90, 180)})
    full.update_stochastic_names(1)
    assert full.stochastic_names('fitsname')[:6] == ['1SER_SAL', '1SER_SIN', '1SER_SRI', '1SER_SRO', '1SER_SPA',
                                                     '1SER_SWD']
    plain = component()
    assert not plain.has_spiral and not plain.is_general and plain.header_flags(2) == {}
    assert 'spiral_wind' not in plain.values_batch(np.zeros((1, 2)))


def test_the_value_errors():
    ok = {'r_in': 1.0, 'r_out': 5.0, 'winding': 1.0}
    with pytest.raises(ValueError, match='pitch'):
        component(spiral=dict(ok, pitch=0.3))
    for key in ok:
        with pytest.raises(ValueError, match=key):
            component(spiral={k: v for k, v in ok.items() if k != key})
    with pytest.raises(ValueError, match='integrate'):
        component(integrate=True, spiral=ok)


def test_each_support_violation_is_minus_infinity():
    """Columns alpha, incl, r_in, r_out, sky, wind, x, y; radians."""
    wide = lambda: Uniform(loc=-100, scale=200)
    s = component(angle_degrees=False, angle=0.3,
                  spiral={'r_in': wide(), 'r_out': wide(), 'winding': wide(), 'alpha': wide(), 'inclination': wide(),
                          'sky_angle': wide()})
    good = [0.5, 0.4, 2.0, 9.0, 0.3, 4.0, 25.0, 25.0]
    bad = []
    for col, val in ((2, -0.1), (3, 2.0), (3, 1.5), (0, -0.01), (1, 0.5 * np.pi), (1, -1.6)):
        bad.append(list(good))
        bad[-1][col] = val
    for col in range(6):
        for val in (np.nan, np.inf):
            bad.append(list(good))
            bad[-1][col] = val
    block = np.array([good, [0.0, 0.0, 0.0, 1e-3, 0.0, 0.0, 25.0, 25.0]] + bad)
    lp = s.log_priors_batch(block)
    assert np.all(np.isfinite(lp[:2])) and np.all(lp[2:] == -np.inf)
    for vec, want in zip(block, lp):
        s.set_stochastic_values(vec)
        got = s.log_priors()                 # (eight priors summed in another order: equal to rounding)
        assert abs(got - want) <= 1e-13 * abs(want) if np.isfinite(want) else (got == -np.inf)
    # in degrees the inclination is held to 90
    d = component(spiral={'r_in': 1.0, 'r_out': 5.0, 'winding': 100.0, 'inclination': Uniform(loc=-100, scale=200)})
    lp = d.log_priors_batch(np.array([[89.0, 25.0, 25.0], [90.0, 25.0, 25.0], [-95.0, 25.0, 25.0]]))
    assert np.isfinite(lp[0]) and np.all(lp[1:] == -np.inf)


def test_add_to_array_uses_the_definition_in_degrees_and_beside_the_other_keywords():
    s = component(xy=(30.3, 28.6), spiral={'r_in': 2.0, 'r_out': 9.0, 'winding': 150.0, 'alpha': 0.5,
                                           'inclination': 40.0, 'sky_angle': -25.0})
    arr = np.zeros((64, 64))
    s.add_to_array(arr, 25.0)
    spiral = (2.0, 9.0, np.deg2rad(150.0), 0.5, np.deg2rad(40.0), np.deg2rad(-25.0))
    assert np.array_equal(arr, Sersic.spiral_image(s.derived_row(25.0), 0.0, [], spiral, (64, 64)))
    s = component(xy=(30.3, 28.6), boxiness=0.7, angle_degrees=False, angle=0.3, fourier={2: (0.2, 0.5)},
                  spiral={'r_in': 2.0, 'r_out': 9.0, 'winding': -3.0})
    arr = np.zeros((64, 64))
    s.add_to_array(arr, 25.0)
    want = Sersic.spiral_image(s.derived_row(25.0), 0.7, [(2, 0.2, 0.5)], (2.0, 9.0, -3.0, 0.0, 0.0, 0.0), (64, 64))
    assert np.array_equal(arr, want)


# -- from the model file to the layouts ------------------------------------------------------------------------

class RecordingLayout(tf.RecordingLayout):
    def set_spiral_layout(self, flags, col, const):
        self.calls.append(('spiral', (list(flags), list(col), list(const))))


SPIRAL_TEXT = (", spiral={'r_in': 2.0, 'r_out': Uniform(loc=5, scale=20), 'winding': Normal(loc=0, scale=200), "
               "'inclination': Uniform(loc=0, scale=70)}")


def test_model_file_round_trip_and_the_calls(tmp_path):
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN)
    plain = MultiComponentModel(path)
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN, sersic_text=SPIRAL_TEXT)
    model = MultiComponentModel(path)
    new = [n for n in model.param_names if n not in plain.param_names]
    assert new == ['2_Sersic_spiral_incl', '2_Sersic_spiral_r_out', '2_Sersic_spiral_wind']
    assert [n for n in model.param_names if n not in new] == plain.param_names
    assert model.param_names[model.param_names.index('2_Sersic_reff_b') + 1] == '2_Sersic_spiral_incl'
    assert model.param_names[model.param_names.index('2_Sersic_spiral_wind') + 1] == '2_Sersic_xy'
    abbrs = dict(zip(model.param_names, model.param_fits_abbrs))
    assert abbrs['2_Sersic_spiral_incl'] == '2SER_SIN' and abbrs['2_Sersic_spiral_wind'] == '2SER_SWD'
    assert all(len(a) <= 8 for a in abbrs.values())
    assert model.sersic_general_flags == [True] and model.sersic_spiral_flags == [True] and model.has_aux
    assert model.sersic_fourier_masks == [0] and model.header_flags() == {'2SERSPI': True}
    rec = RecordingLayout()
    model._register_layout(rec)
    # (no modes: no Fourier call; the library gives a field with a spiral the empty Fourier block)
    assert [c[0] for c in rec.calls] == ['layout', 'aux', 'spiral']
    assert rec.calls[1][1] == ([-1, -1, -1], [0.0, 0.0, 0.0], [False], [True])
    inc, rout, wind = (tg.column_of(model, n) for n in new)
    flags, col, const = rec.calls[2][1]
    assert flags == [True]
    assert col == [-1, rout, wind, -1, inc, -1] and const == [2.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert not {inc, rout, wind} & set(rec.calls[0][1][2])
    # aux rows: slope x 2 and boxiness, the twelve (empty) Fourier entries, then the six
    theta = np.arange(2.0 * model.num_params).reshape(2, -1)
    aux = model.aux_rows(theta)
    assert aux.shape == (2, 21) and not aux[:, :15].any()
    assert np.array_equal(aux[:, [16, 17, 19]], theta[:, [rout, wind, inc]]) and np.all(aux[:, 15] == 2.0)
    assert not aux[:, [18, 20]].any()
    # beside modes: layout, aux, fourier, spiral -- in this order
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN, sersic_text=tf.FOURIER_TEXT + SPIRAL_TEXT)
    both = MultiComponentModel(path)
    rec = RecordingLayout()
    both._register_layout(rec)
    assert [c[0] for c in rec.calls] == ['layout', 'aux', 'fourier', 'spiral']
    assert both.header_flags() == {'2SERFOU': '1,3', '2SERSPI': True}
    aux = both.aux_rows(np.arange(2.0 * both.num_params).reshape(2, -1))
    assert aux.shape == (2, 21) and np.all(aux[:, 7] == 0.1) and np.all(aux[:, 15] == 2.0)


def test_a_model_without_the_keyword_makes_the_calls_it_made(tmp_path):
    """`tg.RecordingLayout` and `tf.RecordingLayout` have no `set_spiral_layout`: a call would raise."""
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN)
    model = MultiComponentModel(path)
    rec = tg.RecordingLayout()
    model._register_layout(rec)
    assert [c[0] for c in rec.calls] == ['layout'] and model.sersic_spiral_flags == [False]
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_TILTED, sersic_text=', boxiness=Uniform(loc=-1, scale=2)')
    model = MultiComponentModel(path)
    rec = tg.RecordingLayout()
    model._register_layout(rec)
    assert [c[0] for c in rec.calls] == ['layout', 'aux']
    assert rec.calls[1][1] == ([1, 2, 7], [0.0, 0.0, 0.0], [True], [True])
    assert model.aux_rows(np.zeros((3, model.num_params))).shape == (3, 3)
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN, sersic_text=tf.FOURIER_TEXT)
    model = MultiComponentModel(path)
    rec = tf.RecordingLayout()
    model._register_layout(rec)
    assert [c[0] for c in rec.calls] == ['layout', 'aux', 'fourier']
    assert model.aux_rows(np.zeros((3, model.num_params))).shape == (3, 15)


def test_a_field_set_registers_the_spiral_only_for_the_field_that_has_it(tmp_path):
    """The spiral field first and last among fields without the keyword: each field's proxy gets its own model's
    calls."""
    dirs = []
    for name, text in (('a', SPIRAL_TEXT), ('b', ''), ('c', ', boxiness=Uniform(loc=-1, scale=2)')):
        (tmp_path / name).mkdir()
        dirs.append(tg.write_field(tmp_path / name, sky_text=tg.SKY_PLAIN, sersic_text=text)[0])
    for order in ((0, 1, 2), (1, 2, 0)):
        models = [MultiComponentModel(dirs[k]) for k in order]
        recs = [RecordingLayout() for _ in models]
        for m, rec in zip(models, recs):
            m._register_layout(rec)
        want = {0: ['layout', 'aux', 'spiral'], 1: ['layout'], 2: ['layout', 'aux']}
        assert [[c[0] for c in rec.calls] for rec in recs] == [want[k] for k in order]
        assert [m.sersic_spiral_flags for m in models] == [[k == 0] for k in order]


def test_joint_model_shares_the_radii_and_keeps_the_winding_per_field(tmp_path):
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    kw = dict(sky_text=tg.SKY_PLAIN, sersic_text=SPIRAL_TEXT)
    a = MultiComponentModel(tg.write_field(tmp_path / 'a', **kw)[0])
    b = MultiComponentModel(tg.write_field(tmp_path / 'b', **kw)[0])
    joint = JointModel([a, b], per_field=['2_Sersic_spiral_wind'])
    assert joint.param_names.count('2_Sersic_spiral_r_out') == 1
    assert '2_Sersic_spiral_wind_f0' in joint.param_names and '2_Sersic_spiral_wind_f1' in joint.param_names
    assert '2_Sersic_spiral_wind' not in joint.param_names
    assert joint.header_flags() == {'2SERSPI': True}
    sent = []
    for f, m in enumerate(joint.field_models):
        rec = RecordingLayout()
        m._register_layout(rec, columns=joint.field_columns(f), n_params=joint.num_params)
        assert [c[0] for c in rec.calls] == ['layout', 'aux', 'spiral']
        sent.append(rec.calls[2][1][1])
    assert sent[0][1] == sent[1][1] and sent[0][4] == sent[1][4] and sent[0][2] != sent[1][2]


def test_database_round_trip_of_the_columns_and_the_flag(tmp_path):
    from psfmc_amd import database
    text = (", spiral={'r_in': Uniform(loc=0, scale=5), 'r_out': Uniform(loc=5, scale=20), "
            "'winding': Normal(loc=0, scale=200), 'alpha': Uniform(loc=0, scale=2), "
            "'inclination': Uniform(loc=0, scale=70), 'sky_angle': Uniform(loc=-90, scale=180)}")
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN, sersic_text=text)
    model = MultiComponentModel(path)

    class Chain(object):
        chain = np.arange(4.0 * 3 * model.num_params).reshape(4, 3, model.num_params)
        lnprobability = np.zeros((4, 3))
    table = database.save_database(Chain(), model, str(tmp_path / 'db.fits'))
    assert table.meta['2SERSPI'] is True or table.meta['2SERSPI'] == True          # noqa: E712
    names = ['2_Sersic_spiral_' + k for k in ('r_in', 'r_out', 'wind', 'alpha', 'incl', 'sky')]
    assert all(n in table.colnames for n in names)
    back = database.load_database(str(tmp_path / 'db.fits'))
    assert back.meta['2SERSPI'] in (True, 'T')
    for n in names:
        assert np.array_equal(np.ravel(back[n]), np.ravel(table[n]))
