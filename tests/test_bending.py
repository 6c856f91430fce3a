"""Bending modes of general components (`bending={m: a_m}` on `Sersic`, `Moffat` and `Ferrer`) on the host: the numpy
definition (`Sersic.bend`, `Sersic.bent_image`, the trailing `bending` of `radial_rho2`, `general_point` and
`general_mean_image`), the keyword's way from a model file to the packed layout and the bending layout, and the
library's table composer.  No GPU needed; the device is held to the same definition in tests/test_gpu_bending.py."""
import numpy as np
import pytest

import test_general_components as tg
import test_radial_laws as tr
import test_truncation as tt
from psfmc_amd import MultiComponentModel, engine
from psfmc_amd.ModelComponents import Sersic
from psfmc_amd.distributions import Uniform
from psfmc_amd.models import JointModel

MAG, ZP = tt.MAG, tt.ZP
FLUX = tt.FLUX
MODES, SPIRAL = tt.MODES, tt.SPIRAL
TRUNC = (4.0, 8.0, 14.0, 20.0)
BEND = [(2, 0.3), (3, -0.1)]
sersic, image = tt.sersic, tt.image


def frame(row, x, y):
    """(u, v, r_a / r_b) of the pixel coordinates (x, y), written out from the derived row."""
    x0, y0, m00, m01, m10, m11 = row[:6]
    dx, dy = x - x0, y - y0
    return m00 * dx + m01 * dy, m10 * dx + m11 * dy, np.hypot(m10, m11) / np.hypot(m00, m01)


def pixel_of(row, u, v):
    """The pixel coordinates of the point (u, v) of the component's frame."""
    x0, y0, m00, m01, m10, m11 = row[:6]
    dx, dy = np.linalg.solve(np.array([[m00, m01], [m10, m11]]), np.array([u, v]))
    return x0 + dx, y0 + dy


# -- the definition ----------------------------------------------------------------------------------------------

def test_values_at_hand_picked_points():
    """A Moffat (no centroid term): Sigma_0 (1 + g (u^2 + v'^2))^-beta with v' = v + (r_a / r_b)(a_2 u^2 + a_3 u^3)
    written out here -- at three arbitrary points, at a point on the ridge (v = -(r_a / r_b) f(u): the value of the
    major axis at that u) and at u = v = 0 (Sigma_0 itself)."""
    comp = tr.moffat(xy=(31.3, 32.6), fwhm=12.0, fwhm_b=5.0, beta=2.5, angle=0.4)
    row = comp.derived_row(ZP)
    sigma0 = Sersic.radial_central('moffat', row, (2.5, 0.0))
    g = 4.0 * np.expm1(np.log(2.0) / 2.5)
    f = lambda u: 0.3 * u ** 2 - 0.1 * u ** 3
    point = lambda x, y: Sersic.general_point('moffat', row, (2.5, 0.0), 0.0, [], None, np.float64(x), np.float64(y),
                                              None, BEND)
    for x, y in ((40.0, 20.0), (25.5, 37.25), (31.0, 50.0)):
        u, v, ratio = frame(row, x, y)
        assert abs(ratio - 12.0 / 5.0) < 1e-14
        vb = v + ratio * f(u)
        want = sigma0 * (1.0 + g * (u * u + vb * vb)) ** -2.5
        assert abs(point(x, y) / want - 1) <= 1e-13, (x, y)
        assert abs(point(x, y) / Sersic.general_point('moffat', row, (2.5, 0.0), 0.0, [], None, np.float64(x),
                                                      np.float64(y)) - 1) > 1e-3       # (and the bending acts there)
    u0 = 0.7
    x, y = pixel_of(row, u0, -(12.0 / 5.0) * f(u0))
    assert abs(point(x, y) / (sigma0 * (1.0 + g * u0 * u0) ** -2.5) - 1) <= 1e-12
    assert point(row[0], row[1]) == sigma0
    # the same through a whole image, the component's add_to_array and `bent_image`
    bent = tr.moffat(xy=(31.3, 32.6), fwhm=12.0, fwhm_b=5.0, beta=2.5, angle=0.4, bending={2: 0.3, 3: -0.1})
    img = image(bent)
    assert np.array_equal(img, Sersic.bent_image('moffat', row, (2.5, 0.0), 0.0, [], None, None, BEND, (64, 64)))
    yy, xx = np.mgrid[0:64, 0:64].astype(np.float64)
    u, v, ratio = frame(row, xx, yy)
    want = sigma0 * (1.0 + g * (u * u + (v + ratio * f(u)) ** 2)) ** -2.5
    assert np.allclose(img, want, rtol=1e-13, atol=0.0)
    # the Sersic law: the centroid term keeps the pixel plane's dx, dy
    row = sersic().derived_row(ZP)
    got = Sersic.bent_image(None, row, None, 0.0, [], None, None, [(2, 0.25)], (64, 64))
    u, v, ratio = frame(row, xx, yy)
    kappa, p, sb = row[6], row[7], row[8]
    rho2 = u * u + (v + ratio * 0.25 * u * u) ** 2
    gg = -2 * kappa * p * rho2 ** (p - 0.5)
    want = sb * np.exp(-kappa * (rho2 ** p - 1)) * (1 + gg * gg * rho2 / ((xx - row[0]) ** 2 + (yy - row[1]) ** 2) / 12)
    assert np.allclose(got, want, rtol=1e-12, atol=0.0)


def test_without_the_argument_every_function_returns_its_bits():
    row = sersic().derived_row(ZP)
    yy, xx = np.mgrid[0:24, 0:24] + 20.25
    for law, pars in ((None, None), ('moffat', (2.5, 0.0)), ('ferrer', (2.0, 1.0))):
        for modes, spiral in (([], None), (MODES, None), (MODES, SPIRAL)):
            for trunc in (None, TRUNC):
                a = Sersic.general_point(law, row, pars, 0.3, modes, spiral, xx, yy, trunc)
                b = Sersic.general_mean_image(law, row, pars, 0.3, modes, spiral, (32, 32), trunc)
                c = Sersic.truncated_image(law, row, pars, 0.3, modes, spiral, trunc, (64, 64))
                r = Sersic.radial_rho2(row, 0.3, modes, spiral, (64, 64))
                for none in (None, [], ()):
                    assert np.array_equal(a, Sersic.general_point(law, row, pars, 0.3, modes, spiral, xx, yy, trunc, none))
                    assert np.array_equal(b, Sersic.general_mean_image(law, row, pars, 0.3, modes, spiral, (32, 32),
                                                                       trunc, bending=none))
                    assert np.array_equal(c, Sersic.bent_image(law, row, pars, 0.3, modes, spiral, trunc, none,
                                                               (64, 64)), equal_nan=True)
                    for got, want in zip(Sersic.radial_rho2(row, 0.3, modes, spiral, (64, 64), none), r):
                        assert np.array_equal(got, want, equal_nan=True)
    # the parents themselves, bare, with modes and with a spiral
    assert np.array_equal(Sersic.bent_image(None, row, None, 0.3, [], None, None, None, (64, 64)),
                          Sersic.general_image(row, 0.3, (64, 64)))
    assert np.array_equal(Sersic.bent_image(None, row, None, 0.3, MODES, None, None, None, (64, 64)),
                          Sersic.fourier_image(row, 0.3, MODES, (64, 64)))
    assert np.array_equal(Sersic.bent_image(None, row, None, 0.3, MODES, SPIRAL, None, [], (64, 64)),
                          Sersic.spiral_image(row, 0.3, MODES, SPIRAL, (64, 64)))
    # a component without the keyword renders what it rendered
    assert np.array_equal(image(sersic(boxiness=0.3)), Sersic.general_image(row, 0.3, (64, 64)))
    assert not sersic(boxiness=0.3).has_bending and sersic(boxiness=0.3).bending_list() is None


def test_zero_amplitudes_give_the_parents_values():
    row = sersic().derived_row(ZP)
    zero = [(1, 0.0), (2, 0.0), (4, 0.0)]
    yy, xx = np.mgrid[0:24, 0:24] + 20.25
    for law, pars in ((None, None), ('moffat', (2.5, 0.0)), ('ferrer', (2.0, 1.0))):
        for modes, spiral in (([], None), (MODES, None), (MODES, SPIRAL)):
            for trunc in (None, TRUNC):
                assert np.array_equal(Sersic.bent_image(law, row, pars, 0.3, modes, spiral, trunc, zero, (64, 64)),
                                      Sersic.truncated_image(law, row, pars, 0.3, modes, spiral, trunc, (64, 64)))
                assert np.array_equal(Sersic.general_point(law, row, pars, 0.3, modes, spiral, xx, yy, trunc, zero),
                                      Sersic.general_point(law, row, pars, 0.3, modes, spiral, xx, yy, trunc))
        assert np.array_equal(Sersic.general_mean_image(law, row, pars, 0.3, MODES, None, (32, 32), bending=zero),
                              Sersic.general_mean_image(law, row, pars, 0.3, MODES, None, (32, 32)))
    assert np.array_equal(image(sersic(bending={2: 0.0})), image(sersic(boxiness=0.0)))


def test_ridge_sign_and_scale():
    """Angle 0, only a_2 = 0.25, r_a = 10, r_b = 3, the centre between pixel centres: with X = r_a u along and Y = r_b v
    across the major axis (at angle 0 the image's y and -x), the brightest pixel of each line X in -12 ... 12 lies
    within one pixel of Y = -r_a a_2 (X / r_a)^2 -- a banana open towards -Y, 3.6 pixels off the axis at |X| = 12."""
    comp = sersic(xy=(32.0, 32.0), reff=10.0, reff_b=3.0, index=1.0, angle=0.0, bending={2: 0.25})
    row = comp.derived_row(ZP)
    img = image(comp, (65, 65))
    yy, xx = np.mgrid[0:65, 0:65].astype(np.float64)
    u, v, _ = frame(row, xx, yy)
    big_x, big_y = np.rint(10.0 * u).astype(int), 3.0 * v
    assert np.array_equal(big_x, (yy - 32).astype(int)) and np.allclose(big_y, 32 - xx, atol=1e-13)
    for line in range(-12, 13):
        on = big_x == line
        best = np.nanargmax(np.where(on, img, -np.inf))
        want = -10.0 * 0.25 * (line / 10.0) ** 2
        assert abs(big_y.ravel()[best] - want) <= 1.0, (line, big_y.ravel()[best], want)
    assert big_y.ravel()[np.nanargmax(np.where(big_x == 12, img, -np.inf))] <= -3.0           # (and it is a displacement)


FLUX_CASES = [('moffat', {}), ('ferrer', dict(alpha=0.5, beta=0.0)), ('ferrer', dict(alpha=2.0, beta=1.0)),
              ('ferrer', dict(r_out=40.0, r_out_b=20.0, alpha=1.0, beta=-1.5))]


@pytest.mark.parametrize('amps', [{2: 0.3, 3: -0.1}, {1: 0.4, 2: -0.25, 4: 0.05}], ids=['23', '124'])
@pytest.mark.parametrize('law,kw', FLUX_CASES, ids=['moffat', 'ferrer-0.5-0', 'ferrer-2-1', 'ferrer40-1--1.5'])
def test_total_flux_is_the_parents(law, kw, amps):
    """The shear has unit Jacobian: image sum over F at 256^2, centre (127.3, 128.6), angle 0.4, at the 5e-4 of
    tests/test_radial_laws.py (a numpy prototype of the definition gave at most 2.3e-4 on these eight cases)."""
    comp = (tr.moffat if law == 'moffat' else tr.ferrer)(bending=amps, **kw)
    ratio = np.sum(tr.image(comp)) / FLUX
    print('%s %r %r: image sum / F - 1 = %.3e' % (law, kw, amps, ratio - 1))
    assert abs(ratio - 1) <= 5e-4


def test_pixel_mean_averages_the_bent_law():
    """Away from the 7 x 7 box: (2 centre + corner mean) / 3 of the bent general_point, written out here."""
    comp = sersic(boxiness=0.4, bending={1: 0.2, 3: -0.1}, truncation=tt.BOTH, pixel_mean=True)
    row, b = comp.derived_row(ZP), [(1, 0.2), (3, -0.1)]
    got = image(comp)
    # (one-element arrays: numpy's array power and its scalar power may differ in the last bit)
    g = lambda x, y: Sersic.general_point(None, row, None, 0.4, [], None, np.array([x], dtype=np.float64),
                                          np.array([y], dtype=np.float64), TRUNC, b)[0]
    for py, px in ((20, 45), (32, 40), (50, 22)):
        corners = 0.25 * ((g(px - 0.5, py - 0.5) + g(px + 0.5, py - 0.5)) + (g(px - 0.5, py + 0.5) + g(px + 0.5, py + 0.5)))
        assert got[py, px] == (2.0 * g(px, py) + corners) / 3.0
    assert np.array_equal(got, Sersic.general_mean_image(None, row, None, 0.4, [], None, (64, 64), TRUNC, b))
    assert np.all(np.isfinite(image(sersic(xy=(30.0, 32.0), bending={2: 0.3}, pixel_mean=True))))
    s = image(sersic(xy=(30.0, 32.0), bending={2: 0.3}))
    assert np.isnan(s[32, 30]) and np.isnan(s).sum() == 1          # the centre stays the centre


# -- the components --------------------------------------------------------------------------------------------------

def test_the_value_errors():
    for bad in (0, 5, -1, 1.5, True, '2'):
        with pytest.raises(ValueError, match='integers in 1 ... 4'):
            sersic(bending={bad: 0.1})
    with pytest.raises(ValueError, match='twice'):
        sersic(bending=[(2, 0.1), (2, 0.2)])
    with pytest.raises(ValueError, match='twice'):
        tr.moffat(bending=[(3, 0.1), (3.0, Uniform(loc=0, scale=1))])
    with pytest.raises(ValueError, match='pixel_mean=True'):
        sersic(bending={2: 0.1}, integrate=True)
    with pytest.raises(ValueError, match='distinct integers'):
        Sersic.bend(np.ones(9), np.ones(3), np.ones(3), [(5, 0.1)])
    with pytest.raises(ValueError, match='distinct integers'):
        Sersic.bend(np.ones(9), np.ones(3), np.ones(3), [(2, 0.1), (2, 0.1)])
    # a plain Sersic with the keyword alone is a general component at c = 0, with or without pixel_mean
    c = sersic(bending={2.0: 0.25, 4: Uniform(loc=-1, scale=2)})
    assert c.is_general and not c.has_boxiness and c.has_bending and c.bending_modes == (2, 4) and c.bending_mask == 0b1010
    assert c.free_names() == ['bend4']
    assert sersic(bending={1: 0.1}, pixel_mean=True).pixel_mean
    assert tr.ferrer(bending={1: 0.1}).bending_mask == 1 and not tr.ferrer().has_bending
    # an empty mapping names no mode: not a general component, and no excuse for pixel_mean on a plain Sersic
    assert not sersic(bending={}).is_general and not sersic(bending={}).has_bending
    with pytest.raises(ValueError, match='pixel_mean=True needs'):
        sersic(bending={}, pixel_mean=True)


def test_the_support_is_every_amplitude_finite():
    wide = lambda: Uniform(loc=-100, scale=200)
    c = sersic(bending={2: wide(), 3: 0.1, 4: wide()})
    assert c.free_names() == ['bend2', 'bend4']
    block = np.array([[0.3, -0.2], [50.0, -99.0], [np.nan, 0.1], [0.1, np.nan], [np.inf, 0.1], [0.1, -np.inf]])
    with np.errstate(all='ignore'):
        lp = c.log_priors_batch(block)
    assert np.all(np.isfinite(lp[:2])) and np.all(lp[2:] == -np.inf), lp
    for vec, want in zip(block, lp):
        c.set_stochastic_values(vec)
        with np.errstate(all='ignore'):
            got = c.log_priors()
        assert abs(got - want) <= 1e-13 * abs(want) if np.isfinite(want) else got == -np.inf
    assert Sersic._bending_ok([[0.0, 1e300], [np.nan, 0.0]]).tolist() == [True, False]


def test_packing_order_names_and_header_flags():
    U = lambda lo, hi: Uniform(loc=lo, scale=hi - lo)
    s = Sersic(xy=U(20, 40), mag=MAG, reff=U(2, 20), reff_b=3.0, index=1.0, angle=20.0, angle_degrees=True,
               bending={3: U(-1, 1), 2: U(-1, 2), 1: 0.05})
    s.update_stochastic_names(2)
    assert s.free_names() == ['bend2', 'bend3', 'reff', 'xy']
    assert s.stochastic_names() == ['2_Sersic_bend2', '2_Sersic_bend3', '2_Sersic_reff', '2_Sersic_xy']
    assert s.stochastic_names('fitsname') == ['2SER_BD2', '2SER_BD3', '2SER_RE', '2SER_xy']
    assert s.header_flags(2) == {'2SERBND': '1,2,3'}
    vals = s.values_batch(np.array([[0.25, -0.5, 9.0, 30.0, 31.0]]))
    assert np.array_equal(s._bending_values(vals, 1), [[0.05, 0.25, -0.5]])
    f = tr.ferrer(bending={4: U(-1, 1)}, truncation={'outer': (10.0, 20.0)})
    f.update_stochastic_names(3)
    assert f.stochastic_names('fitsname') == ['3FER_BD4'] and f.header_flags(3) == {
        '3SERLAW': 'ferrer', '3SERTRU': 'outer', '3SERBND': '4'}
    m = tr.moffat(bending={2: 0.3, 3: -0.1})
    m.update_stochastic_names(1)
    assert m.stochastic_names() == [] and m.bending_list() == BEND and m.header_flags(1) == {
        '1SERLAW': 'moffat', '1SERBND': '2,3'}


# -- from the model file to the layouts ------------------------------------------------------------------------

class RecordingLayout(tt.RecordingLayout):
    def set_bending_layout(self, masks, col, const):
        self.calls.append(('bending', (list(masks), list(col), list(const))))


BANANA = ', bending={2: Uniform(loc=-1.0, scale=3.0), 3: -0.1}'
MOFFAT_BENT = ('Moffat(xy=Uniform(loc=c - ms, scale=2 * ms), mag=Uniform(loc=19.0, scale=5.0), '
               'fwhm=Uniform(loc=1.0, scale=6.0), fwhm_b=2.0, beta=3.0, angle=30.0, angle_degrees=True, '
               'bending={1: Uniform(loc=-0.5, scale=1.0), 4: Uniform(loc=-0.5, scale=1.0)})\n')
DRESSED = (", boxiness=Uniform(loc=-1, scale=2), spiral={'r_in': 2.0, 'r_out': Uniform(loc=5, scale=20), 'winding': 90.0}"
           ", truncation={'outer': (14.0, Uniform(loc=15.0, scale=20.0))}")


def test_model_file_round_trip_and_the_calls(tmp_path):
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN)
    plain = MultiComponentModel(path)
    path, _ = tr.write_field(tmp_path, MOFFAT_BENT, sky_text=tg.SKY_PLAIN, sersic_text=BANANA)
    model = MultiComponentModel(path)
    new = [n for n in model.param_names if n not in plain.param_names]
    assert new == ['2_Sersic_bend2', '3_Moffat_bend1', '3_Moffat_bend4', '3_Moffat_fwhm', '3_Moffat_mag', '3_Moffat_xy']
    assert all(len(a) <= 8 for a in model.param_fits_abbrs)
    assert model.sersic_bending_masks == [0b0110, 0b1001] and model.sersic_general_flags == [True, True] and model.has_aux
    assert model.header_flags() == {'2SERBND': '2,3', '3SERLAW': 'moffat', '3SERBND': '1,4'}
    rec = RecordingLayout()
    model._register_layout(rec)
    # (no modes, spiral or truncation: the library gives a field with bending the blocks before it itself)
    assert [c[0] for c in rec.calls] == ['layout', 'aux', 'radial', 'bending']
    col = lambda n: tg.column_of(model, n)
    masks, bcol, bconst = rec.calls[3][1]
    assert masks == [0b0110, 0b1001]
    assert bcol == [-1, col('2_Sersic_bend2'), -1, -1, col('3_Moffat_bend1'), -1, -1, col('3_Moffat_bend4')]
    assert bconst == [0.0, 0.0, -0.1, 0.0, 0.0, 0.0, 0.0, 0.0]
    theta = np.arange(2.0 * model.num_params).reshape(2, -1) + 1.0
    aux = model.aux_rows(theta)
    assert aux.shape == (2, 2 + 29 * 2) and not aux[:, :28].any()
    assert np.array_equal(aux[:, 28:40], np.tile([0.0, 1.0, 0.0, 0.0, 0.0, 0.0], (2, 2)))            # the spiral's padding
    assert np.array_equal(aux[:, 44:52], np.tile([0.0, 1.0, 0.0, 1.0], (2, 2)))                      # the truncation's
    want = np.c_[np.zeros(2), theta[:, col('2_Sersic_bend2')], np.full(2, -0.1), np.zeros(2),
                 theta[:, col('3_Moffat_bend1')], np.zeros((2, 2)), theta[:, col('3_Moffat_bend4')]]
    assert np.array_equal(aux[:, 52:], want)
    # host log-priors through the model: the support
    np.random.seed(5)
    ok = np.array(model.init_params_from_priors(3))
    assert np.all(np.isfinite(model.log_priors_batch(ok)))
    ok[1, col('2_Sersic_bend2')] = np.nan
    ok[2, col('3_Moffat_bend4')] = np.inf
    with np.errstate(all='ignore'):
        lp = model.log_priors_batch(ok)
    assert np.isfinite(lp[0]) and np.all(lp[1:] == -np.inf)


def test_a_model_without_the_keyword_makes_exactly_the_calls_it_made(tmp_path):
    """Boxiness + spiral + truncation, through a recorder that has no `set_bending_layout` at all and through one that
    has: the same calls with the same arguments, and the rows the length they had."""
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN, sersic_text=DRESSED)
    model = MultiComponentModel(path)
    old, rec = tt.RecordingLayout(), RecordingLayout()
    assert not hasattr(old, 'set_bending_layout')
    model._register_layout(old)
    model._register_layout(rec)
    assert repr(old.calls) == repr(rec.calls) and [c[0] for c in old.calls] == ['layout', 'aux', 'spiral', 'truncation']
    assert model.sersic_bending_masks == [0] and model.aux_rows(np.zeros((1, model.num_params))).shape == (1, 2 + 25)
    assert 'SERBND' not in ''.join(model.header_flags())
    # ... and with the keyword added, the same calls and one more
    (tmp_path / 'bent').mkdir()
    path, _ = tg.write_field(tmp_path / 'bent', sky_text=tg.SKY_PLAIN, sersic_text=DRESSED + BANANA)
    bent = MultiComponentModel(path)
    rec = RecordingLayout()
    bent._register_layout(rec)
    assert [c[0] for c in rec.calls] == ['layout', 'aux', 'spiral', 'truncation', 'bending']
    assert bent.aux_rows(np.zeros((1, bent.num_params))).shape == (1, 2 + 29)


def test_joint_model_keeps_an_amplitude_per_field(tmp_path):
    models = []
    for name in 'ab':
        (tmp_path / name).mkdir()
        models.append(MultiComponentModel(tg.write_field(tmp_path / name, sky_text=tg.SKY_PLAIN, sersic_text=BANANA)[0]))
    joint = JointModel(models, per_field=['2_Sersic_bend2'])
    names = joint.param_names
    assert '2_Sersic_bend2' not in names and '2_Sersic_bend2_f0' in names and '2_Sersic_bend2_f1' in names
    assert joint.header_flags() == {'2SERBND': '2,3'}
    sent = []
    for f, m in enumerate(joint.field_models):
        rec = RecordingLayout()
        m._register_layout(rec, columns=joint.field_columns(f), n_params=joint.num_params)
        assert [c[0] for c in rec.calls] == ['layout', 'aux', 'bending']
        sent.append(rec.calls[2][1][1])
    assert sent[0][1] != sent[1][1] and min(sent[0][1], sent[1][1]) >= 0
    assert sent[0][:1] + sent[0][2:] == sent[1][:1] + sent[1][2:] == [-1, -1, -1]


def test_database_round_trip_of_the_columns_and_the_flag(tmp_path):
    from psfmc_amd import database
    path, _ = tr.write_field(tmp_path, MOFFAT_BENT, sky_text=tg.SKY_PLAIN, sersic_text=BANANA)
    model = MultiComponentModel(path)

    class Chain(object):
        chain = np.arange(4.0 * 3 * model.num_params).reshape(4, 3, model.num_params)
        lnprobability = np.zeros((4, 3))
    table = database.save_database(Chain(), model, str(tmp_path / 'db.fits'))
    back = database.load_database(str(tmp_path / 'db.fits'))
    for t in (table, back):
        assert t.meta['2SERBND'] == '2,3' and t.meta['3SERBND'] == '1,4' and t.meta['3SERLAW'] == 'moffat'
    for n in ('2_Sersic_bend2', '3_Moffat_bend1', '3_Moffat_bend4'):
        assert n in back.colnames and np.array_equal(np.ravel(back[n]), np.ravel(table[n]))


# -- the library's table composer ----------------------------------------------------------------------------------

N_SKY, N_SER = tt.N_SKY, tt.N_SER
BASE, FOURIER, RADIAL, PAD_SPIRAL = tt.BASE, tt.FOURIER, tt.RADIAL, tt.PAD_SPIRAL
BENDING = ([0b0010, 0b1101], [-1, 7, -1, -1, 8, -1, 9, 4], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])


def test_the_composer_appends_the_fifth_block_behind_neutral_ones():
    """n_sky = 1, n_sersic = 2: 4 base entries, 24 Fourier, 12 spiral, 4 radial, 8 truncation, 8 bending = 2 n_sky +
    29 n_sersic; Sersic k's amplitudes at 2 n_sky + 25 n_sersic + 4 k."""
    const, col, kinds, sides, bends, counts = engine.debug_aux_table(N_SKY, N_SER, base=BASE, bending=BENDING)
    assert counts == (60, 24, 12, 4, 8, 8) and len(const) == len(col) == 2 * N_SKY + 29 * N_SER
    assert list(col[:4]) == BASE[0] and list(const[:4]) == BASE[1]
    assert list(col[4:52]) == [-1] * 48 and not np.any(const[4:28]) and list(const[28:40]) == PAD_SPIRAL
    assert not np.any(const[40:52]) and list(kinds) == [0, 0] and list(sides) == [0, 0] and list(bends) == BENDING[0]
    for k in range(N_SER):
        at = 2 * N_SKY + 25 * N_SER + 4 * k
        assert list(col[at:at + 4]) == BENDING[1][4 * k:4 * k + 4] and list(const[at:at + 4]) == BENDING[2][4 * k:4 * k + 4]
    # behind registered blocks: they keep their entries
    const, col, kinds, sides, bends, counts = engine.debug_aux_table(
        N_SKY, N_SER, base=BASE, fourier=FOURIER, radial=RADIAL, truncation=tt.TRUNC, bending=BENDING)
    assert counts == (60, 24, 12, 4, 8, 8) and list(kinds) == RADIAL[0] and list(sides) == tt.TRUNC[0]
    assert list(col[4:28]) == FOURIER[1] and list(const[28:40]) == PAD_SPIRAL and list(col[40:44]) == RADIAL[1]
    assert list(col[44:52]) == tt.TRUNC[1] and list(const[44:52]) == tt.TRUNC[2]
    assert list(col[52:]) == BENDING[1] and list(const[52:]) == BENDING[2] and list(bends) == BENDING[0]
    # all-zero masks are no registration, and a field without the call has the table it had, in the shapes it had
    zero = ([0, 0],) + BENDING[1:]
    const, col, kinds, sides, bends, counts = engine.debug_aux_table(N_SKY, N_SER, base=BASE, radial=RADIAL,
                                                                     truncation=tt.TRUNC, bending=zero)
    old = engine.debug_aux_table(N_SKY, N_SER, base=BASE, radial=RADIAL, truncation=tt.TRUNC)
    assert len(old) == 5 and counts == old[4] + (0,) and len(bends) == 0
    assert all(np.array_equal(a, b) for a, b in zip((const, col, kinds, sides), old[:4]))
    assert len(engine.debug_aux_table(N_SKY, N_SER, base=BASE, radial=RADIAL)) == 4
    assert engine.debug_aux_table(N_SKY, N_SER, bending=BENDING)[5] == (0, 0, 0, 0, 0, 0)      # no aux layout, no table
    with pytest.raises(ValueError, match='4 entries per Sersic'):
        engine.debug_aux_table(N_SKY, N_SER, base=BASE, bending=(BENDING[0], BENDING[1][:6], BENDING[2][:6]))
