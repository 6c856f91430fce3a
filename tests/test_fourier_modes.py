"""Azimuthal Fourier modes on Sersic isophotes (`Sersic(..., fourier={m: (amplitude, phase)})`) on the host: the numpy
definition (`Sersic.fourier_image`, `Sersic.fourier_area_ratio`) and the keyword's way from a model file to the packed
layout, the auxiliary-parameter layout and the Fourier layout.  No GPU needed; the device is held to the same
definition in tests/test_gpu_fourier_modes.py."""
import numpy as np
import pytest

import test_general_components as tg
from psfmc_amd import MultiComponentModel
from psfmc_amd.ModelComponents import Sersic
from psfmc_amd.distributions import Normal, Uniform
from psfmc_amd.models import JointModel

SHAPE = (256, 256)
# the mode sets of the flux-closure check: sum |a| <= 0.4
MODE_SETS = [[(1, 0.2, 0.5)], [(3, 0.15, -0.8)], [(1, 0.1, 0.3), (2, 0.2, 1.1), (4, 0.1, -0.4)]]
# MEASURED (n = 1, r_e = 12, r_b = 8, 256^2, centre (127.3, 128.6), angle 0.4): |image sum / (a = 0, c = 0 sum) - 1|
# for the three sets, per c -- the pixel-sampling error of the profile, which DESIGN.md section 15 records for the
# boxiness alone (2.1e-4 at c = 0.7, 1.41e-3 at c = -1 with a = 0 on this component); asserted at twice the worst
#   c = 0    1.44e-4  4.6e-5   2.40e-4
#   c = 0.7  3.49e-4  2.61e-4  4.33e-4
#   c = -1   1.18e-3  1.38e-3  1.02e-3
CLOSURE_WORST = {0.0: 2.41e-4, 0.7: 4.34e-4, -1.0: 1.38e-3}


def row(x0=127.3, y0=128.6, reff=12.0, reff_b=8.0, index=1.0, angle=0.4):
    return Sersic(xy=(x0, y0), mag=18.0, reff=reff, reff_b=reff_b, index=index, angle=angle).derived_row(25.0)


# -- the definition ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', [0.0, 0.7, -1.0])
def test_zero_amplitudes_are_the_general_image(c):
    want = Sersic.general_image(row(), c, SHAPE)
    got = Sersic.fourier_image(row(), c, [(1, 0.0, 0.3), (4, 0.0, 1.0)], SHAPE)
    assert np.all(np.isfinite(want)) and np.max(np.abs(got - want) / want) <= 1e-15
    assert Sersic.fourier_area_ratio(c, [(2, 0.0, 0.7)]) == 1.0 and Sersic.fourier_area_ratio(c, []) == 1.0


def test_area_ratio_against_the_closed_form():
    """One mode at c = 0: the integral is (1 - a^2)^(-3/2); the 128-point sum is it to rounding for a <= 0.6 and
    9.4e-6 off at a = 0.9, m = 4 (which is why Q is defined as the sum)."""
    for m in range(1, 7):
        for a in (0.1, 0.3, 0.6):
            q = Sersic.fourier_area_ratio(0.0, [(m, a, 0.37)])
            assert abs(q / (1 - a * a) ** -1.5 - 1) <= 1e-12, (m, a)
    off = Sersic.fourier_area_ratio(0.0, [(4, 0.9, 0.37)]) / (1 - 0.81) ** -1.5 - 1
    assert 1e-6 < abs(off) < 1e-4


@pytest.mark.parametrize('c', [0.0, 0.7, -1.0])
def test_total_flux_does_not_depend_on_the_modes(c):
    base = np.sum(Sersic.general_image(row(), 0.0, SHAPE))
    for modes in MODE_SETS:
        err = abs(np.sum(Sersic.fourier_image(row(), c, modes, SHAPE)) / base - 1)
        print('c = %g, %d mode(s): flux closure %.3e' % (c, len(modes), err))
        assert err <= 2 * CLOSURE_WORST[c], (c, modes, err)


def test_symmetries_of_a_circular_component_on_a_pixel_corner():
    r = row(127.5, 127.5, 10.0, 10.0, 1.0, 0.0)
    im = Sersic.fourier_image(r, 0.0, [(4, 0.2, 0.3)], SHAPE)
    assert np.max(np.abs(np.rot90(im) - im)) <= 1e-12 * im.max()
    im = Sersic.fourier_image(r, 0.0, [(2, 0.2, 0.3), (4, 0.1, 0.1), (6, 0.1, -1.0)], SHAPE)
    assert np.max(np.abs(im[::-1, ::-1] - im)) <= 1e-12 * im.max()
    assert np.max(np.abs(np.rot90(im) - im)) > 1e-3 * im.max()          # (the m = 2 mode is not a quarter-turn's)
    im = Sersic.fourier_image(r, 0.0, [(1, 0.2, 0.3)], SHAPE)
    assert np.max(np.abs(im[::-1, ::-1] - im)) > 0.05 * im.max()        # MEASURED 0.16


@pytest.mark.parametrize('angle,phase', [(0.0, 0.0), (0.4, 0.7), (-1.0, 2.0)])
def test_m1_moves_the_centroid_to_pi_minus_phase(angle, phase):
    """The sign convention: r = r0 (1 + a cos(t + phi)) is largest at t = -phi ... and the flux-weighted centroid of
    the m = 1 mode lies at angle pi - phi in the (u, v) frame (MEASURED within 1.6e-4 rad, shift 3.3 ... 4.5 pixels)."""
    r = row(angle=angle)
    im = Sersic.fourier_image(r, 0.0, [(1, 0.2, phase)], SHAPE)
    yy, xx = np.mgrid[0:SHAPE[0], 0:SHAPE[1]].astype(np.float64)
    cx, cy = np.sum(im * xx) / im.sum() - r[0], np.sum(im * yy) / im.sum() - r[1]
    u, v = r[2] * cx + r[3] * cy, r[4] * cx + r[5] * cy
    d = (np.arctan2(v, u) - (np.pi - phase) + np.pi) % (2 * np.pi) - np.pi
    assert np.hypot(cx, cy) > 2.0 and abs(d) <= 0.05, (cx, cy, d)


def test_on_pixel_centre_is_nan_and_bad_mode_numbers_raise():
    im = Sersic.fourier_image(row(100.0, 90.0), 0.0, [(1, 0.2, 0.1)], SHAPE)
    assert np.isnan(im[90, 100]) and np.isfinite(np.delete(im.ravel(), 90 * 256 + 100)).all()
    for modes in ([(0, 0.1, 0.0)], [(7, 0.1, 0.0)], [(2, 0.1, 0.0), (2, 0.1, 0.5)]):
        with pytest.raises(ValueError):
            Sersic.fourier_image(row(), 0.0, modes, (8, 8))


# -- the component ---------------------------------------------------------------------------------------------------

def component(**kw):
    args = dict(xy=Uniform(loc=(20, 20), scale=(20, 20)), mag=18.0, reff=8.0, reff_b=5.0, index=1.0, angle=20.0,
                angle_degrees=True)
    args.update(kw)
    return Sersic(**args)


def test_packing_order_names_and_header_flags():
    s = component(boxiness=Uniform(loc=-1, scale=2), index=Uniform(loc=0.5, scale=4),
                  fourier={3: (0.1, Normal(loc=0, scale=30)), 1: (Uniform(loc=-0.5, scale=1), Uniform(loc=-180, scale=360))})
    s.update_stochastic_names(2)
    assert s.free_names() == ['boxiness', 'f1_amp', 'f1_phase', 'f3_phase', 'index', 'xy']
    assert s.stochastic_names() == ['2_Sersic_boxiness', '2_Sersic_f1_amp', '2_Sersic_f1_phase', '2_Sersic_f3_phase',
                                    '2_Sersic_index', '2_Sersic_xy']
    assert s.stochastic_names('fitsname')[1:4] == ['2SER_F1A', '2SER_F1P', '2SER_F3P']
    assert s.fourier_modes == (1, 3) and s.is_general
    assert s.header_flags(2) == {'2SERBOX': True, '2SERFOU': '1,3'}
    plain = component()
    assert plain.fourier_modes == () and not plain.is_general and plain.header_flags(2) == {}
    assert 'f1_amp' not in plain.values_batch(np.zeros((1, 2)))
    for bad in ({0: (0.1, 0.0)}, {7: (0.1, 0.0)}, {1.5: (0.1, 0.0)}, {2: 0.1}):
        with pytest.raises(ValueError):
            component(fourier=bad)


def test_fourier_with_integrate_raises():
    with pytest.raises(ValueError, match='integrate'):
        component(integrate=True, fourier={1: (0.1, 0.0)})


def test_support_of_the_amplitudes():
    """sum |a| >= 1 and a NaN amplitude are -inf in log_priors and log_priors_batch."""
    s = component(fourier={1: (Uniform(loc=-2, scale=4), 10.0), 2: (Uniform(loc=-2, scale=4), Uniform(loc=-180, scale=360))})
    # columns: f1_amp, f2_amp, f2_phase, x, y
    block = np.array([[0.3, -0.4, 20.0, 25.0, 25.0], [0.6, -0.4, 20.0, 25.0, 25.0], [0.5, 0.6, 20.0, 25.0, 25.0],
                      [np.nan, 0.1, 20.0, 25.0, 25.0], [0.2, 0.1, np.inf, 25.0, 25.0]])
    lp = s.log_priors_batch(block)
    assert np.isfinite(lp[0]) and np.all(lp[1:] == -np.inf)
    for vec, want in zip(block, lp):
        s.set_stochastic_values(vec)
        got = s.log_priors()
        assert (got == want) if np.isfinite(want) else (got == -np.inf)


def test_add_to_array_uses_the_definition_in_degrees_and_at_c_zero():
    s = component(xy=(30.3, 28.6), fourier={1: (0.2, 40.0), 4: (0.1, -25.0)})
    arr = np.zeros((64, 64))
    s.add_to_array(arr, 25.0)
    want = Sersic.fourier_image(s.derived_row(25.0), 0.0, [(1, 0.2, np.deg2rad(40.0)), (4, 0.1, np.deg2rad(-25.0))], (64, 64))
    assert np.array_equal(arr, want)
    s = component(xy=(30.3, 28.6), boxiness=0.7, angle_degrees=False, angle=0.3, fourier={2: (0.2, 0.5)})
    arr = np.zeros((64, 64))
    s.add_to_array(arr, 25.0)
    assert np.array_equal(arr, Sersic.fourier_image(s.derived_row(25.0), 0.7, [(2, 0.2, 0.5)], (64, 64)))


# -- from the model file to the layouts ------------------------------------------------------------------------

class RecordingLayout(tg.RecordingLayout):
    def set_fourier_layout(self, mode_masks, col, const):
        self.calls.append(('fourier', (list(mode_masks), list(col), list(const))))


FOURIER_TEXT = ', fourier={1: (Uniform(loc=-0.5, scale=1), Uniform(loc=-180, scale=360)), 3: (0.1, Normal(loc=0, scale=30))}'


def test_model_file_round_trip_and_the_calls(tmp_path):
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN)
    plain = MultiComponentModel(path)
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN, sersic_text=FOURIER_TEXT)
    model = MultiComponentModel(path)
    new = [n for n in model.param_names if n not in plain.param_names]
    assert new == ['2_Sersic_f1_amp', '2_Sersic_f1_phase', '2_Sersic_f3_phase']
    assert [n for n in model.param_names if n not in new] == plain.param_names
    assert model.param_names[model.param_names.index('2_Sersic_angle') + 1] == '2_Sersic_f1_amp'
    assert model.param_names[model.param_names.index('2_Sersic_f3_phase') + 1] == '2_Sersic_index'
    abbrs = dict(zip(model.param_names, model.param_fits_abbrs))
    assert abbrs['2_Sersic_f1_amp'] == '2SER_F1A' and abbrs['2_Sersic_f3_phase'] == '2SER_F3P'
    assert all(len(a) <= 8 for a in abbrs.values())
    assert model.sersic_general_flags == [True] and model.sersic_fourier_masks == [0b101] and model.has_aux
    assert model.header_flags() == {'2SERFOU': '1,3'}
    rec = RecordingLayout()
    model._register_layout(rec)
    assert [c[0] for c in rec.calls] == ['layout', 'aux', 'fourier']
    # no boxiness keyword: the aux entry is the neutral constant, the component flagged general (c = 0)
    assert rec.calls[1][1] == ([-1, -1, -1], [0.0, 0.0, 0.0], [False], [True])
    a1, p1, p3 = (tg.column_of(model, n) for n in new)
    masks, col, const = rec.calls[2][1]
    assert masks == [0b101]
    assert col == [a1, p1, -1, -1, -1, p3] + [-1] * 6
    assert const == [0.0, 0.0, 0.0, 0.0, 0.1, 0.0] + [0.0] * 6
    main_cols = list(rec.calls[0][1][2])
    assert not {a1, p1, p3} & set(main_cols)
    # aux rows: the three existing columns (slope x 2, boxiness), then the twelve entries
    theta = np.arange(2.0 * model.num_params).reshape(2, -1)
    aux = model.aux_rows(theta)
    assert aux.shape == (2, 15) and not aux[:, :3].any()
    assert np.array_equal(aux[:, [3, 4, 8]], theta[:, [a1, p1, p3]]) and np.all(aux[:, 7] == 0.1)
    assert not aux[:, [5, 6, 9, 10, 11, 12, 13, 14]].any()


def test_a_model_without_the_keyword_makes_the_parents_calls(tmp_path):
    """`tg.RecordingLayout` has no `set_fourier_layout`: a call would raise."""
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN)
    model = MultiComponentModel(path)
    rec = tg.RecordingLayout()
    model._register_layout(rec)
    assert [c[0] for c in rec.calls] == ['layout'] and model.sersic_fourier_masks == [0]
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_TILTED, sersic_text=', boxiness=Uniform(loc=-1, scale=2)')
    model = MultiComponentModel(path)
    rec = tg.RecordingLayout()
    model._register_layout(rec)
    assert [c[0] for c in rec.calls] == ['layout', 'aux']
    assert rec.calls[1][1] == ([1, 2, 7], [0.0, 0.0, 0.0], [True], [True])
    assert model.aux_rows(np.zeros((3, model.num_params))).shape == (3, 3)


def test_joint_model_shares_an_amplitude_and_keeps_phases_per_field(tmp_path):
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    kw = dict(sky_text=tg.SKY_PLAIN, sersic_text=FOURIER_TEXT)
    a = MultiComponentModel(tg.write_field(tmp_path / 'a', **kw)[0])
    b = MultiComponentModel(tg.write_field(tmp_path / 'b', **kw)[0])
    joint = JointModel([a, b], per_field=['2_Sersic_f1_phase'])
    assert joint.param_names.count('2_Sersic_f1_amp') == 1
    assert '2_Sersic_f1_phase_f0' in joint.param_names and '2_Sersic_f1_phase_f1' in joint.param_names
    assert joint.header_flags() == {'2SERFOU': '1,3'}
    sent = []
    for f, m in enumerate(joint.field_models):
        rec = RecordingLayout()
        m._register_layout(rec, columns=joint.field_columns(f), n_params=joint.num_params)
        assert [c[0] for c in rec.calls] == ['layout', 'aux', 'fourier']
        sent.append(rec.calls[2][1][1])
    assert sent[0][0] == sent[1][0] and sent[0][1] != sent[1][1] and sent[0][5] == sent[1][5]


def test_database_header_records_the_modes(tmp_path):
    from psfmc_amd import database
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN, sersic_text=FOURIER_TEXT)
    model = MultiComponentModel(path)

    class Chain(object):
        chain = np.zeros((4, 3, model.num_params))
        lnprobability = np.zeros((4, 3))
    table = database.save_database(Chain(), model, str(tmp_path / 'db.fits'))
    assert table.meta['2SERFOU'] == '1,3'
    assert '2_Sersic_f1_amp' in table.colnames
