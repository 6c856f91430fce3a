"""Inner and outer truncation of general components (`truncation={'inner': (lo, hi), 'outer': (lo, hi)}` on `Sersic`,
`Moffat` and `Ferrer`) on the host: the numpy definition (`Sersic.truncation_weight`, `Sersic.truncated_image`, the
trailing `truncation` of `general_point` / `general_mean_image`), the keyword's way from a model file to the packed
layout and the truncation layout, the flux fraction, and the library's table composer.  No GPU needed; the device is
held to the same definition in tests/test_gpu_truncation.py."""
import numpy as np
import pytest

import test_general_components as tg
import test_radial_laws as tr
import test_spiral_arms as ts
from psfmc_amd import MultiComponentModel, engine
from psfmc_amd.ModelComponents import Sersic
from psfmc_amd.distributions import Uniform
from psfmc_amd.models import JointModel

MAG, ZP = 18.0, 25.0
FLUX = 10 ** (-0.4 * (MAG - ZP))
MODES = [(2, 0.15, 0.5), (4, 0.1, -0.8)]
SPIRAL = (2.0, 9.0, 3.0, 0.5, 0.3, 0.2)
LO, HI = 0.5 * (1.0 + np.tanh(-2.0)), 0.5 * (1.0 + np.tanh(2.0))          # the ramp at its two radii: 0.018, 0.982
BOTH = {'inner': (4.0, 8.0), 'outer': (14.0, 20.0)}


def sersic(xy=(31.3, 32.6), reff=10.0, reff_b=7.0, index=1.0, angle=0.4, **kw):
    return Sersic(xy=xy, mag=MAG, reff=reff, reff_b=reff_b, index=index, angle=angle, **kw)


def image(comp, shape=(64, 64)):
    return comp.add_to_array(np.zeros(shape), ZP)


# -- the definition ----------------------------------------------------------------------------------------------

def test_without_the_argument_every_function_returns_its_bits():
    row = sersic().derived_row(ZP)
    yy, xx = np.mgrid[0:24, 0:24] + 20.25
    for law, pars in ((None, None), ('moffat', (2.5, 0.0)), ('ferrer', (2.0, 1.0))):
        for modes, spiral in (([], None), (MODES, None), (MODES, SPIRAL)):
            a = Sersic.general_point(law, row, pars, 0.3, modes, spiral, xx, yy)
            assert np.array_equal(a, Sersic.general_point(law, row, pars, 0.3, modes, spiral, xx, yy, None))
            assert np.array_equal(a, Sersic.general_point(law, row, pars, 0.3, modes, spiral, xx, yy, truncation=None))
            b = Sersic.general_mean_image(law, row, pars, 0.3, modes, spiral, (32, 32))
            assert np.array_equal(b, Sersic.general_mean_image(law, row, pars, 0.3, modes, spiral, (32, 32), None))
    parents = [(([], None), Sersic.general_image(row, 0.3, (64, 64))),
               ((MODES, None), Sersic.fourier_image(row, 0.3, MODES, (64, 64))),
               ((MODES, SPIRAL), Sersic.spiral_image(row, 0.3, MODES, SPIRAL, (64, 64)))]
    for (modes, spiral), want in parents:
        assert np.array_equal(Sersic.truncated_image(None, row, None, 0.3, modes, spiral, None, (64, 64)), want)
    assert np.array_equal(Sersic.truncated_image('moffat', row, (2.5, 0.0), 0.3, MODES, SPIRAL, None, (64, 64)),
                          Sersic.radial_image('moffat', row, (2.5, 0.0), 0.3, MODES, SPIRAL, (64, 64)))
    # a component without the keyword renders what it rendered, whatever else it has
    assert np.array_equal(image(sersic(boxiness=0.3)), Sersic.general_image(row, 0.3, (64, 64)))
    assert not sersic(boxiness=0.3).has_truncation and sersic(boxiness=0.3).truncation_tuple() is None


def test_the_ramps_at_their_four_radii():
    """A round-number Moffat on a pixel centre with its major axis along y (angle 0): at 4, 8, 14 and 20 pixels along
    the major axis the value is the parent's times 0.018, 0.982 (the inner ramp; the outer one is 1 - 3e-9 and 1 - 6e-7
    there) and 0.982, 0.018 (the outer ramp); along the minor axis, at the same rho, the same factors."""
    plain = tr.moffat(xy=(30.0, 32.0), fwhm=12.0, fwhm_b=6.0, beta=2.5, angle=0.0)
    inner = image(tr.moffat(xy=(30.0, 32.0), fwhm=12.0, fwhm_b=6.0, beta=2.5, angle=0.0, truncation={'inner': (4.0, 8.0)}))
    outer = image(tr.moffat(xy=(30.0, 32.0), fwhm=12.0, fwhm_b=6.0, beta=2.5, angle=0.0, truncation={'outer': (14.0, 20.0)}))
    parent = image(plain)
    assert abs(LO - 0.018) < 1e-4 and abs(HI - 0.982) < 1e-4
    for img, radii, want in ((inner, (4, 8), (LO, HI)), (outer, (14, 20), (HI, LO))):
        for r, w in zip(radii, want):
            for py, px in ((32 + r, 30), (32 - r, 30), (32, 30 + r // 2), (32, 30 - r // 2)):
                assert abs(img[py, px] / parent[py, px] - w) <= 1e-13, (r, py, px)
    both = image(tr.moffat(xy=(30.0, 32.0), fwhm=12.0, fwhm_b=6.0, beta=2.5, angle=0.0, truncation=BOTH))
    assert np.allclose(both, inner * outer / parent, rtol=1e-14, atol=0.0)
    # the truncation follows the isophotes: boxy ones, and the factor is a function of rho2 alone
    row = plain.derived_row(ZP)
    rho2, centre = Sersic.radial_rho2(row, 0.8, MODES, SPIRAL, (64, 64))
    got = Sersic.truncated_image('moffat', row, (2.5, 0.0), 0.8, MODES, SPIRAL, (4.0, 8.0, None, None), (64, 64))
    par = Sersic.radial_image('moffat', row, (2.5, 0.0), 0.8, MODES, SPIRAL, (64, 64))
    s = 12.0 * np.sqrt(np.where(centre, 0.0, rho2))
    # ((1 + tanh a) / 2 without its cancellation: 6e-6 at a = -6, where the tanh form has five digits fewer)
    assert np.allclose(got, par * (1 / (1 + np.exp(-2 * (2 * (2 * s - 12.0) / 4.0)))), rtol=1e-15, atol=0.0)
    assert np.allclose(got, par * 0.5 * (1 + np.tanh(2 * (2 * s - 12.0) / 4.0)), rtol=0.0, atol=1e-15 * par)


def test_a_side_far_outside_the_image_is_one_while_the_other_acts():
    inner = image(sersic(truncation={'inner': (4.0, 8.0)}))
    far_out = image(sersic(truncation={'inner': (4.0, 8.0), 'outer': (1e4, 1.01e4)}))
    assert np.all(np.abs(far_out - inner) <= 1e-15 * inner) and np.nanmin(inner / image(sersic(boxiness=0.0))) < 0.02
    outer = image(sersic(truncation={'outer': (14.0, 20.0)}))
    far_in = image(sersic(truncation={'inner': (0.0, 1e-3), 'outer': (14.0, 20.0)}))
    # (the factor in its tail is e^(-2 a), not the 0 of a saturated tanh: 3e-34 of the parent at the far corner)
    assert np.all(np.abs(far_in - outer) <= 1e-15 * outer) and 0.0 < outer.min() < 1e-30 * outer.max()
    parent = image(sersic(boxiness=0.0))
    assert outer[32, 31] / parent[32, 31] > 0.999 and outer[60, 60] / parent[60, 60] < 1e-3


def test_the_centre_pixel_of_each_law():
    """On a pixel centre an inner-truncated Moffat is finite (Sigma_0 times the factor at s = 0), an inner-truncated
    Sersic law is NaN like its parent, and finite with pixel_mean=True."""
    cut = {'inner': (3.0, 6.0)}
    m = image(tr.moffat(xy=(30.0, 32.0), truncation=cut))
    row = tr.moffat(xy=(30.0, 32.0)).derived_row(ZP)
    s0 = Sersic.radial_central('moffat', row, (3.5, 0.0))
    assert np.all(np.isfinite(m)) and m[32, 30] == s0 * (1.0 / (1.0 + np.exp(12.0)))
    assert abs(m[32, 30] - s0 * (0.5 * (1.0 + np.tanh(-6.0)))) <= 1e-15 * s0
    f = image(tr.ferrer(xy=(30.0, 32.0), r_out=25.0, r_out_b=12.0, fourier={2: (0.1, 0.3)}, truncation=cut))
    assert np.all(np.isfinite(f)) and f[32, 30] > 0
    s = image(sersic(xy=(30.0, 32.0), truncation=cut))
    assert np.isnan(s[32, 30]) and np.isnan(s).sum() == 1
    mean = image(sersic(xy=(30.0, 32.0), truncation=cut, pixel_mean=True))
    assert np.all(np.isfinite(mean)) and 0 < mean[32, 30] < mean[32 + 8, 30]          # a hole in the middle


def test_pixel_mean_applies_its_scheme_to_the_product():
    """Away from the 7 x 7 box: (2 centre + corner mean) / 3 of general_point * inner * outer, written out here."""
    comp = sersic(boxiness=0.4, truncation=BOTH, pixel_mean=True)
    row, t = comp.derived_row(ZP), (4.0, 8.0, 14.0, 20.0)
    got = image(comp)
    # (the samples on whole grids, as the definition takes them: numpy's array and scalar `**` differ in the last bit
    # at one point in twenty, with or without a truncation)
    g = lambda x, y: Sersic.general_point(None, row, None, 0.4, [], None, x, y, t)
    yy, xx = np.mgrid[0:64, 0:64].astype(np.float64)
    cyy, cxx = np.mgrid[0:65, 0:65].astype(np.float64) - 0.5
    mid, cor = g(xx, yy), g(cxx, cyy)
    for py, px in ((20, 45), (32, 40), (50, 22)):
        corners = 0.25 * ((cor[py, px] + cor[py, px + 1]) + (cor[py + 1, px] + cor[py + 1, px + 1]))
        assert got[py, px] == (2.0 * mid[py, px] + corners) / 3.0
    assert np.array_equal(got, Sersic.general_mean_image(None, row, None, 0.4, [], None, (64, 64), truncation=t))


# -- the components --------------------------------------------------------------------------------------------------

def test_the_value_errors():
    with pytest.raises(ValueError, match='middle'):
        sersic(truncation={'middle': (1.0, 2.0)})
    with pytest.raises(ValueError, match='pair'):
        sersic(truncation={'inner': 3.0})
    with pytest.raises(ValueError, match='pair'):
        tr.moffat(truncation={'outer': (3.0, 4.0, 5.0)})
    with pytest.raises(ValueError, match='pair'):
        tr.ferrer(truncation={'outer': Uniform(loc=3.0, scale=4.0)})
    with pytest.raises(ValueError, match="'inner' or 'outer'"):
        sersic(truncation={})
    with pytest.raises(ValueError, match='pixel_mean=True'):
        sersic(truncation={'inner': (1.0, 2.0)}, integrate=True)
    with pytest.raises(ValueError, match='None'):
        Sersic.truncation_weight(np.ones(9), np.ones(3), np.zeros(3, bool), (1.0, None, None, None))
    # a plain Sersic with the keyword alone is a general component at c = 0, with or without pixel_mean
    c = sersic(truncation={'outer': (5.0, 9.0)})
    assert c.is_general and not c.has_boxiness and c.truncation_flags == 2 and c.truncation_sides == ('outer',)
    assert sersic(truncation={'inner': (5.0, 9.0)}, pixel_mean=True).pixel_mean
    row = c.derived_row(ZP)
    assert np.array_equal(image(c), Sersic.truncated_image(None, row, None, 0.0, [], None, (None, None, 5.0, 9.0), (64, 64)))


def test_the_support_of_each_side():
    wide = lambda: Uniform(loc=-100, scale=200)
    c = sersic(truncation={'inner': (wide(), wide()), 'outer': (wide(), 30.0)})
    assert c.free_names() == ['trunc_in_hi', 'trunc_in_lo', 'trunc_out_lo']
    good = [8.0, 4.0, 14.0]
    bad = [[4.0, 4.0, 14.0], [3.0, 4.0, 14.0], [8.0, -0.1, 14.0], [np.nan, 4.0, 14.0], [8.0, np.nan, 14.0],
           [np.inf, 4.0, 14.0], [8.0, 4.0, 30.0], [8.0, 4.0, -1.0], [8.0, 4.0, np.nan]]
    inside = [[8.0, 0.0, 14.0], [8.0, 4.0, 0.0], [30.0, 4.0, 2.0], [1e-3, 0.0, 29.999]]   # lo = 0; overlapping sides
    block = np.array([good] + bad + inside)
    lp = c.log_priors_batch(block)
    assert np.isfinite(lp[0]) and np.all(lp[1:1 + len(bad)] == -np.inf) and np.all(np.isfinite(lp[1 + len(bad):])), lp
    for vec, want in zip(block, lp):
        c.set_stochastic_values(vec)
        with np.errstate(all='ignore'):
            got = c.log_priors()
        assert abs(got - want) <= 1e-13 * abs(want) if np.isfinite(want) else got == -np.inf
    # an absent side is not looked at
    one = tr.moffat(truncation={'outer': (wide(), wide())})
    assert one.free_names() == ['trunc_out_hi', 'trunc_out_lo']
    assert np.isfinite(one.log_priors_batch(np.array([[20.0, 14.0]]))[0])
    assert one.log_priors_batch(np.array([[14.0, 14.0]]))[0] == -np.inf


def test_packing_order_names_and_header_flags():
    U = lambda lo, hi: Uniform(loc=lo, scale=hi - lo)
    s = Sersic(xy=U(20, 40), mag=MAG, reff=U(2, 20), reff_b=3.0, index=1.0, angle=20.0, angle_degrees=True,
               spiral={'r_in': 2.0, 'r_out': U(5, 20), 'winding': 90.0},
               truncation={'inner': (U(0, 5), U(5, 10)), 'outer': (15.0, U(16, 30))})
    s.update_stochastic_names(2)
    assert s.free_names() == ['reff', 'spiral_r_out', 'trunc_in_hi', 'trunc_in_lo', 'trunc_out_hi', 'xy']
    assert s.stochastic_names() == ['2_Sersic_reff', '2_Sersic_spiral_r_out', '2_Sersic_trunc_in_hi',
                                    '2_Sersic_trunc_in_lo', '2_Sersic_trunc_out_hi', '2_Sersic_xy']
    assert s.stochastic_names('fitsname') == ['2SER_RE', '2SER_SRO', '2SER_TIH', '2SER_TIL', '2SER_TOH', '2SER_xy']
    assert s.header_flags(2) == {'2SERSPI': True, '2SERTRU': 'inner,outer'}
    vals = s.values_batch(np.array([[9.0, 11.0, 7.0, 3.0, 22.0, 30.0, 31.0]]))
    assert np.array_equal(s._truncation_values(vals, 1), [[3.0, 7.0, 15.0, 22.0]])
    f = tr.ferrer(truncation={'outer': (U(10, 20), U(20, 40))})
    f.update_stochastic_names(3)
    assert f.stochastic_names('fitsname') == ['3FER_TOH', '3FER_TOL'] and f.header_flags(3) == {
        '3SERLAW': 'ferrer', '3SERTRU': 'outer'}
    assert np.array_equal(f._truncation_values(f.values_batch(np.array([[33.0, 12.0]])), 1), [[0.0, 1.0, 12.0, 33.0]])
    m = tr.moffat(truncation={'inner': (1.0, U(2, 9))})
    m.update_stochastic_names(1)
    assert m.stochastic_names('fitsname') == ['1MOF_TIH'] and m.header_flags(1) == {'1SERLAW': 'moffat', '1SERTRU': 'inner'}
    assert m.truncation_tuple()[0] == 1.0 and m.truncation_tuple()[2:] == (None, None)


# -- from the model file to the layouts ------------------------------------------------------------------------

class RecordingLayout(tr.RecordingLayout):
    def set_truncation_layout(self, flags, col, const):
        self.calls.append(('truncation', (list(flags), list(col), list(const))))


RING = (", truncation={'inner': (Uniform(loc=0.0, scale=6.0), Uniform(loc=6.0, scale=6.0)), "
        "'outer': (14.0, Uniform(loc=15.0, scale=20.0))}")
MOFFAT_CUT = ('Moffat(xy=Uniform(loc=c - ms, scale=2 * ms), mag=Uniform(loc=19.0, scale=5.0), '
              'fwhm=Uniform(loc=1.0, scale=6.0), fwhm_b=2.0, beta=3.0, angle=30.0, angle_degrees=True, '
              "truncation={'outer': (Uniform(loc=5.0, scale=5.0), 12.0)})\n")


def test_model_file_round_trip_and_the_calls(tmp_path):
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN)
    plain = MultiComponentModel(path)
    path, _ = tr.write_field(tmp_path, MOFFAT_CUT, sky_text=tg.SKY_PLAIN, sersic_text=RING)
    model = MultiComponentModel(path)
    new = [n for n in model.param_names if n not in plain.param_names]
    assert new == ['2_Sersic_trunc_in_hi', '2_Sersic_trunc_in_lo', '2_Sersic_trunc_out_hi', '3_Moffat_fwhm',
                   '3_Moffat_mag', '3_Moffat_trunc_out_lo', '3_Moffat_xy']
    assert all(len(a) <= 8 for a in model.param_fits_abbrs)
    assert model.sersic_truncation_flags == [3, 2] and model.sersic_general_flags == [True, True] and model.has_aux
    assert model.header_flags() == {'2SERTRU': 'inner,outer', '3SERLAW': 'moffat', '3SERTRU': 'outer'}
    rec = RecordingLayout()
    model._register_layout(rec)
    # (no modes and no spiral: the library gives a field with a truncation the blocks before it itself)
    assert [c[0] for c in rec.calls] == ['layout', 'aux', 'radial', 'truncation']
    col = lambda n: tg.column_of(model, n)
    flags, tcol, tconst = rec.calls[3][1]
    assert flags == [3, 2]
    assert tcol == [col('2_Sersic_trunc_in_lo'), col('2_Sersic_trunc_in_hi'), -1, col('2_Sersic_trunc_out_hi'), -1, -1,
                    col('3_Moffat_trunc_out_lo'), -1]
    assert tconst == [0.0, 0.0, 14.0, 0.0, 0.0, 1.0, 0.0, 12.0]
    theta = np.arange(2.0 * model.num_params).reshape(2, -1) + 1.0
    aux = model.aux_rows(theta)
    assert aux.shape == (2, 2 + 25 * 2) and not aux[:, :28].any()
    assert np.array_equal(aux[:, 28:40], np.tile([0.0, 1.0, 0.0, 0.0, 0.0, 0.0], (2, 2)))
    assert np.array_equal(aux[:, 40:44], np.c_[np.zeros((2, 2)), np.full(2, 3.0), np.zeros(2)])
    want = np.c_[theta[:, [col('2_Sersic_trunc_in_lo'), col('2_Sersic_trunc_in_hi')]], np.full(2, 14.0),
                 theta[:, col('2_Sersic_trunc_out_hi')], np.zeros(2), np.ones(2), theta[:, col('3_Moffat_trunc_out_lo')],
                 np.full(2, 12.0)]
    assert np.array_equal(aux[:, 44:], want)
    # host log-priors through the model: the support of the sides
    np.random.seed(5)
    ok = np.array(model.init_params_from_priors(4))
    assert np.all(np.isfinite(model.log_priors_batch(ok)))
    ok[1, col('2_Sersic_trunc_in_hi')] = ok[1, col('2_Sersic_trunc_in_lo')]
    ok[2, col('2_Sersic_trunc_out_hi')] = 14.0
    ok[3, col('3_Moffat_trunc_out_lo')] = 12.5
    lp = model.log_priors_batch(ok)
    assert np.isfinite(lp[0]) and np.all(lp[1:] == -np.inf)
    # a model without the keyword makes the calls it made: tr.RecordingLayout has no set_truncation_layout
    path, _ = tr.write_field(tmp_path, tr.FERRER_TEXT % ts.SPIRAL_TEXT, sky_text=tg.SKY_PLAIN)
    other = MultiComponentModel(path)
    old, rec = tr.RecordingLayout(), RecordingLayout()
    other._register_layout(old)
    other._register_layout(rec)
    assert repr(old.calls) == repr(rec.calls) and [c[0] for c in old.calls] == ['layout', 'aux', 'spiral', 'radial']
    assert other.aux_rows(np.zeros((1, other.num_params))).shape == (1, 2 + 21 * 2)


def test_joint_model_shares_one_radius_and_keeps_another_per_field(tmp_path):
    models = []
    for name in 'ab':
        (tmp_path / name).mkdir()
        models.append(MultiComponentModel(tg.write_field(tmp_path / name, sky_text=tg.SKY_PLAIN, sersic_text=RING)[0]))
    joint = JointModel(models, per_field=['2_Sersic_trunc_out_hi'])
    names = joint.param_names
    assert names.count('2_Sersic_trunc_in_hi') == 1 and '2_Sersic_trunc_out_hi' not in names
    assert '2_Sersic_trunc_out_hi_f0' in names and '2_Sersic_trunc_out_hi_f1' in names
    assert joint.header_flags() == {'2SERTRU': 'inner,outer'}
    sent = []
    for f, m in enumerate(joint.field_models):
        rec = RecordingLayout()
        m._register_layout(rec, columns=joint.field_columns(f), n_params=joint.num_params)
        assert [c[0] for c in rec.calls] == ['layout', 'aux', 'truncation']
        sent.append(rec.calls[2][1][1])
    assert sent[0][:3] == sent[1][:3] and sent[0][3] != sent[1][3] and min(sent[0][3], sent[1][3]) >= 0


def test_database_round_trip_of_the_columns_and_the_flag(tmp_path):
    from psfmc_amd import database
    path, _ = tr.write_field(tmp_path, MOFFAT_CUT, sky_text=tg.SKY_PLAIN, sersic_text=RING)
    model = MultiComponentModel(path)

    class Chain(object):
        chain = np.arange(4.0 * 3 * model.num_params).reshape(4, 3, model.num_params)
        lnprobability = np.zeros((4, 3))
    table = database.save_database(Chain(), model, str(tmp_path / 'db.fits'))
    back = database.load_database(str(tmp_path / 'db.fits'))
    for t in (table, back):
        assert t.meta['2SERTRU'] == 'inner,outer' and t.meta['3SERTRU'] == 'outer' and t.meta['3SERLAW'] == 'moffat'
    for n in ('2_Sersic_trunc_in_lo', '2_Sersic_trunc_in_hi', '2_Sersic_trunc_out_hi', '3_Moffat_trunc_out_lo'):
        assert n in back.colnames and np.array_equal(np.ravel(back[n]), np.ravel(table[n]))


# -- the flux fraction -------------------------------------------------------------------------------------------

def test_flux_fraction_of_a_ring():
    """An exponential disc (reff 12 / 9, boxiness 0.5) on 160^2 cut to a ring, inner (8, 14), outer (26, 36): ramps 6
    and 10 pixels wide, the ring inside 40 pixels of a centre 80 from the edges.  MEASURED: the pixel-mean rendering's
    sum over F against `truncation_flux_fraction` (0.474964) differs by 1.78e-7 of the fraction: asserted at twice
    that.  The sum of the definition at 8 x 8 sub-pixels: MEASURED 3.7e-13 (the midpoint rule converges spectrally on
    a smooth ring), and an outer-only cut at a hard-edge limit, (20 - 1e-6, 20 + 1e-6), against the closed form
    1 - (1 + x) e^-x, x = kappa 20 / reff: MEASURED 1.1e-16.  Both gaps are below the 1e-12 the helper asks of its
    quadrature, where twice the measured figure would test the rounding of the machine's exp and tanh and not the
    helper: they are asserted at twice that 1e-12."""
    cut = {'inner': (8.0, 14.0), 'outer': (26.0, 36.0)}
    t = (8.0, 14.0, 26.0, 36.0)
    comp = sersic(xy=(79.3, 80.6), reff=12.0, reff_b=9.0, boxiness=0.5, truncation=cut, pixel_mean=True)
    want = Sersic.truncation_flux_fraction(None, 1.0, 12.0, t)
    mean = np.sum(image(comp, (160, 160))) / FLUX
    o = (np.arange(8) + 0.5) / 8 - 0.5
    fine = np.add.outer(np.arange(160.0), o).ravel()
    sub = np.sum(Sersic.general_point(None, comp.derived_row(ZP), None, 0.5, [], None, fine[None, :], fine[:, None],
                                      t)) / 64.0 / FLUX
    print('fraction %.6f: pixel means %.3e, 8 x 8 sub-pixels %.3e off (relative)' % (
        want, mean / want - 1, sub / want - 1))
    assert 0.3 < want < 0.6
    assert abs(mean / want - 1) <= 2 * 1.78e-7 and abs(sub / want - 1) <= 2 * 1e-12
    # the same fraction whatever bends the isophotes: a Moffat through its own law
    assert abs(Sersic.truncation_flux_fraction('moffat', (2.5,), 12.0, (None, None, 1e5, 1.001e5)) - 1.0) < 1e-8
    x = Sersic.kappa(1.0) * 20.0 / 12.0
    hard = Sersic.truncation_flux_fraction(None, 1.0, 12.0, (None, None, 20.0 - 1e-6, 20.0 + 1e-6))
    print('hard edge: %.3e off the closed form' % (hard / (1 - (1 + x) * np.exp(-x)) - 1))
    assert abs(hard / (1 - (1 + x) * np.exp(-x)) - 1) <= 2 * 1e-12
    ferrer = Sersic.truncation_flux_fraction('ferrer', (2.0, 1.0), 30.0, (None, None, 29.0, 31.0))
    assert 0.9 < ferrer < 1.0                                           # (the law ends at rho = 1, the ramp is cut there)


# -- the library's table composer ----------------------------------------------------------------------------------

N_SKY, N_SER = 1, 2
BASE = ([3, -1, 5, -1], [0.0, 0.5, 0.0, 0.25])
FOURIER = ([0, 0b101], list(range(10, 34)), [0.01 * j for j in range(24)])
RADIAL = ([0, 2], [-1, -1, 6, -1], [0.0, 0.0, 0.0, 0.5])
TRUNC = ([1, 3], [-1, 7, -1, -1, 8, 9, -1, 4], [2.0, 0.0, 0.0, 1.0, 0.0, 0.0, 14.0, 0.0])
PAD_SPIRAL = [0.0, 1.0, 0.0, 0.0, 0.0, 0.0] * 2


def test_the_composer_appends_the_block_behind_neutral_ones():
    """n_sky = 1, n_sersic = 2: 4 base entries, 24 Fourier, 12 spiral, 4 radial, 8 truncation = 2 n_sky + 25 n_sersic;
    Sersic k's truncation entries at 2 n_sky + 21 n_sersic + 4 k."""
    const, col, kinds, sides, counts = engine.debug_aux_table(N_SKY, N_SER, base=BASE, truncation=TRUNC)
    assert counts == (52, 24, 12, 4, 8) and len(const) == len(col) == 2 * N_SKY + 25 * N_SER
    assert list(col[:4]) == BASE[0] and list(const[:4]) == BASE[1]
    assert list(col[4:44]) == [-1] * 40 and not np.any(const[4:28]) and list(const[28:40]) == PAD_SPIRAL
    assert not np.any(const[40:44]) and list(kinds) == [0, 0] and list(sides) == TRUNC[0]
    for k in range(N_SER):
        at = 2 * N_SKY + 21 * N_SER + 4 * k
        assert list(col[at:at + 4]) == TRUNC[1][4 * k:4 * k + 4] and list(const[at:at + 4]) == TRUNC[2][4 * k:4 * k + 4]
    # behind registered blocks: they keep their entries
    const, col, kinds, sides, counts = engine.debug_aux_table(N_SKY, N_SER, base=BASE, fourier=FOURIER, radial=RADIAL,
                                                              truncation=TRUNC)
    assert counts == (52, 24, 12, 4, 8) and list(kinds) == RADIAL[0] and list(sides) == TRUNC[0]
    assert list(col[4:28]) == FOURIER[1] and list(const[28:40]) == PAD_SPIRAL and list(col[40:44]) == RADIAL[1]
    assert list(col[44:]) == TRUNC[1] and list(const[44:]) == TRUNC[2]
    # all-zero flags are no registration, and a field without the call has the table it had
    zero = ([0, 0],) + TRUNC[1:]
    const, col, kinds, sides, counts = engine.debug_aux_table(N_SKY, N_SER, base=BASE, radial=RADIAL, truncation=zero)
    old = engine.debug_aux_table(N_SKY, N_SER, base=BASE, radial=RADIAL)
    assert counts == old[3] + (0,) and len(sides) == 0
    assert np.array_equal(const, old[0]) and np.array_equal(col, old[1]) and np.array_equal(kinds, old[2])
    assert engine.debug_aux_table(N_SKY, N_SER, truncation=TRUNC)[4] == (0, 0, 0, 0, 0)      # no aux layout, no table
