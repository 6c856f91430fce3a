"""Radial laws other than the Sersic law (`Moffat`, `Ferrer`) on the host: the numpy definition
(`Sersic.radial_image`) and the classes' way from a model file to the packed layout and the auxiliary, Fourier, spiral
and radial layouts.  No GPU needed; the device is held to the same definition in tests/test_gpu_radial_laws.py."""
import numpy as np
import pytest
from scipy.special import beta as beta_fn

import test_general_components as tg
import test_spiral_arms as ts
import psfmc_amd
from psfmc_amd import MultiComponentModel
from psfmc_amd.ModelComponents import Ferrer, Moffat, Sersic
from psfmc_amd.distributions import Normal, Uniform
from psfmc_amd.models import JointModel

SHAPE = (256, 256)
CENTRE = (127.3, 128.6)
MAG, ZP = 18.0, 25.0
FLUX = 10 ** (-0.4 * (MAG - ZP))
MODES = [(2, 0.15, 0.5), (4, 0.1, -0.8)]
SPIRAL = (2.0, 9.0, 3.0, 0.5, 0.3, 0.2)
NEUTRAL_SPIRAL = (2.0, 9.0, 0.0, 0.5, 0.0, 0.0)


def moffat(xy=CENTRE, fwhm=9.0, fwhm_b=6.0, beta=3.5, angle=0.4, **kw):
    return Moffat(xy=xy, mag=MAG, fwhm=fwhm, fwhm_b=fwhm_b, beta=beta, angle=angle, **kw)


def ferrer(xy=CENTRE, r_out=60.0, r_out_b=35.0, alpha=2.0, beta=1.0, angle=0.4, **kw):
    return Ferrer(xy=xy, mag=MAG, r_out=r_out, r_out_b=r_out_b, alpha=alpha, beta=beta, angle=angle, **kw)


def image(comp, shape=SHAPE):
    return comp.add_to_array(np.zeros(shape), ZP)


# -- the definition ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', [-0.7, 0.0, 1.0])
def test_total_flux_of_the_moffat(c):
    """fwhm 9 / 6, beta 3.5 on 256^2: MEASURED 1 + 2.9e-5, 1 - 0.8e-6, 1 - 2.9e-6 for c = -0.7, 0, 1."""
    ratio = np.sum(image(moffat(boxiness=c))) / FLUX
    print('moffat c = %g: image sum / F - 1 = %.3e' % (c, ratio - 1))
    assert abs(ratio - 1) <= 5e-4


@pytest.mark.parametrize('c', [-0.7, 0.0, 1.0])
@pytest.mark.parametrize('alpha,beta', [(0.5, 0.0), (2.0, 1.0), (1.0, -1.5)])
def test_total_flux_of_the_ferrer(c, alpha, beta):
    """r_out 60 / 35 on 256^2: MEASURED within 2.2e-5 of 1 in all nine cases."""
    ratio = np.sum(image(ferrer(alpha=alpha, beta=beta, boxiness=c))) / FLUX
    print('ferrer c = %g, alpha = %g, beta = %g: image sum / F - 1 = %.3e' % (c, alpha, beta, ratio - 1))
    assert abs(ratio - 1) <= 5e-4


def test_moffat_half_maximum_on_both_axes():
    """angle = 0 turns the major axis along y: half a FWHM from an on-pixel centre along either axis the value is
    half the centre's, Sigma_0 = F g (beta - 1) / (pi fwhm fwhm_b) written out here."""
    for beta in (1.5, 3.5):
        im = image(moffat(xy=(100.0, 90.0), fwhm=12.0, fwhm_b=8.0, beta=beta, angle=0.0))
        g = 4.0 * (2.0 ** (1.0 / beta) - 1.0)
        sigma0 = FLUX * g * (beta - 1.0) / (np.pi * 12.0 * 8.0)
        assert abs(im[90, 100] - sigma0) <= 1e-14 * sigma0
        for y, x in ((96, 100), (84, 100), (90, 104), (90, 96)):
            assert abs(im[y, x] - 0.5 * sigma0) <= 1e-14 * sigma0, (beta, y, x)


def test_ferrer_edge_flat_core_and_monotone_profile():
    """angle = 0, an on-pixel centre: 0 at and beyond rho = 1 on both axes, exactly Sigma_0 inside at alpha = 0,
    decreasing along the axes at alpha > 0."""
    im = image(ferrer(xy=(100.0, 90.0), r_out=20.0, r_out_b=10.0, alpha=2.0, beta=0.5, angle=0.0))
    assert im[110, 100] == 0.0 and im[70, 100] == 0.0 and im[90, 110] == 0.0 and im[90, 90] == 0.0
    assert np.all(im[111:, :] == 0.0) and np.all(im[:, 111:] == 0.0) and im[109, 100] > 0.0 and im[90, 109] > 0.0
    assert np.all(np.diff(im[90:111, 100]) < 0) and np.all(np.diff(im[90, 100:111]) < 0)
    sigma0 = FLUX / (np.pi * 20.0 * 10.0 * (2.0 / 1.5) * beta_fn(2.0 / 1.5, 3.0))
    assert abs(im[90, 100] - sigma0) <= 1e-14 * sigma0
    flat = image(ferrer(xy=(100.0, 90.0), r_out=20.0, r_out_b=10.0, alpha=0.0, beta=0.5, angle=0.0))
    inside = flat > 0
    assert inside[90, 100] and inside.sum() > 500 and np.all(flat[inside] == flat[90, 100])
    assert abs(flat[90, 100] - FLUX / (np.pi * 20.0 * 10.0)) <= 1e-14 * flat[90, 100]
    assert flat[110, 100] == 0.0 and flat[109, 100] == flat[90, 100]


@pytest.mark.parametrize('law', ['moffat', 'ferrer'])
def test_on_pixel_centre_is_finite_and_sigma_0_with_modes_and_a_spiral(law):
    row = Sersic(xy=(100.0, 90.0), mag=MAG, reff=9.0, reff_b=6.0, index=1.0, angle=0.4).derived_row(ZP)
    pars = (3.5, 0.0) if law == 'moffat' else (2.0, 1.0)
    for modes, spiral in (([], None), (MODES, None), ([], SPIRAL), (MODES, SPIRAL)):
        im = Sersic.radial_image(law, row, pars, 0.7, modes, spiral, SHAPE)
        assert np.all(np.isfinite(im))
        assert im[90, 100] == Sersic.radial_central(law, row, pars, 0.7, modes, spiral) and im[90, 100] == im.max()


@pytest.mark.parametrize('law', ['moffat', 'ferrer'])
def test_neutral_keywords_give_the_same_bits(law):
    row = Sersic(xy=CENTRE, mag=MAG, reff=40.0, reff_b=25.0, index=1.0, angle=0.4).derived_row(ZP)
    pars = (3.5, 0.0) if law == 'moffat' else (2.0, 1.0)
    bare = Sersic.radial_image(law, row, pars, 0.0, [], None, SHAPE)
    zero_modes = [(2, 0.0, 0.5), (4, 0.0, -0.8)]
    for modes, spiral in ((zero_modes, None), ([], NEUTRAL_SPIRAL), (zero_modes, NEUTRAL_SPIRAL)):
        assert np.array_equal(Sersic.radial_image(law, row, pars, 0.0, modes, spiral, SHAPE), bare)
    cls = moffat if law == 'moffat' else ferrer
    with_kw = cls(boxiness=0.0, fourier={2: (0.0, 0.5), 4: (0.0, -0.8)},
                  spiral={'r_in': 2.0, 'r_out': 9.0, 'winding': 0.0, 'alpha': 0.5})
    assert np.array_equal(image(with_kw), image(cls()))


# -- the components --------------------------------------------------------------------------------------------------

def test_each_support_violation_is_minus_infinity_on_both_host_paths():
    wide = lambda: Uniform(loc=-100, scale=200)
    m = Moffat(xy=(30.0, 30.0), mag=MAG, fwhm=wide(), fwhm_b=wide(), beta=wide(), angle=0.3)
    f = Ferrer(xy=(30.0, 30.0), mag=MAG, r_out=wide(), r_out_b=wide(), alpha=wide(), beta=wide(), angle=0.3)
    assert m.free_names() == ['beta', 'fwhm', 'fwhm_b'] and f.free_names() == ['alpha', 'beta', 'r_out', 'r_out_b']
    for comp, good, bad in ((m, [2.5, 9.0, 6.0], [[1.0, 9.0, 6.0], [0.5, 9.0, 6.0], [np.nan, 9.0, 6.0],
                                                  [np.inf, 9.0, 6.0], [2.5, 6.0, 9.0]]),
                            (f, [0.5, 1.0, 9.0, 6.0], [[0.5, 2.0, 9.0, 6.0], [0.5, 3.0, 9.0, 6.0], [0.5, np.nan, 9.0, 6.0],
                                                       [-0.1, 1.0, 9.0, 6.0], [np.nan, 1.0, 9.0, 6.0],
                                                       [0.5, 1.0, 6.0, 9.0]])):
        block = np.array([good] + bad)
        lp = comp.log_priors_batch(block)
        assert np.isfinite(lp[0]) and np.all(lp[1:] == -np.inf), lp
        for vec, want in zip(block, lp):
            comp.set_stochastic_values(vec)
            with np.errstate(all='ignore'):
                got = comp.log_priors()
            assert abs(got - want) <= 1e-13 * abs(want) if np.isfinite(want) else got == -np.inf
    edge = np.array([[0.0, 1.9999, 9.0, 9.0], [0.0, -50.0, 9.0, 6.0]])              # alpha = 0, beta < 2: inside
    assert np.all(np.isfinite(f.log_priors_batch(edge)))


def test_packing_order_names_degrees_and_header_flags():
    f = Ferrer(xy=Uniform(loc=(20, 20), scale=(20, 20)), mag=MAG, r_out=Uniform(loc=5, scale=40),
               r_out_b=Uniform(loc=5, scale=40), alpha=Uniform(loc=0, scale=4), beta=1.0, angle=20.0, angle_degrees=True,
               boxiness=Uniform(loc=-1, scale=2), fourier={3: (Uniform(loc=-0.3, scale=0.6), 40.0)},
               spiral={'r_in': 2.0, 'r_out': Uniform(loc=5, scale=20), 'winding': 90.0, 'alpha': Uniform(loc=0, scale=2)})
    f.update_stochastic_names(2)
    assert f.free_names() == ['alpha', 'boxiness', 'f3_amp', 'r_out', 'r_out_b', 'spiral_alpha', 'spiral_r_out', 'xy']
    assert f.stochastic_names()[3:7] == ['2_Ferrer_r_out', '2_Ferrer_r_out_b', '2_Ferrer_spiral_alpha',
                                         '2_Ferrer_spiral_r_out']
    assert f.stochastic_names('fitsname') == ['2FER_ALP', '2FER_BOX', '2FER_F3A', '2FER_RO', '2FER_ROB', '2FER_SAL',
                                              '2FER_SRO', '2FER_xy']
    assert f.device_kind == 'sersic' and isinstance(f, Sersic) and f.is_general and f.index == 1.0 and not f.integrate
    assert f.header_flags(2) == {'2SERBOX': True, '2SERFOU': '3', '2SERSPI': True, '2SERLAW': 'ferrer'}
    vals = f.values_batch(np.array([[1.5, 0.2, 0.1, 30.0, 12.0, 0.4, 11.0, 25.0, 26.0]]))
    assert vals['reff'][0] == 30.0 and vals['reff_b'][0] == 12.0 and vals['index'][0] == 1.0
    assert np.array_equal(f._radial_values(vals, 1), [[1.5, 1.0]])
    # degrees reach the angles only: the winding of the spiral, not the law's parameters
    assert np.allclose(f._spiral_values(vals, 1), [[2.0, 11.0, 0.5 * np.pi, 0.4, 0.0, 0.0]], rtol=1e-15)
    m = Moffat(xy=(30.0, 30.0), mag=Uniform(loc=15, scale=8), fwhm=Uniform(loc=1, scale=10), fwhm_b=3.0,
               beta=Uniform(loc=1, scale=9), angle=Uniform(loc=0, scale=180), angle_degrees=True)
    m.update_stochastic_names(1)
    assert m.free_names() == ['angle', 'beta', 'fwhm', 'mag']
    assert m.stochastic_names('fitsname') == ['1MOF_ANG', '1MOF_BET', '1MOF_FW', '1MOF_mag']
    assert m.is_general and not m.has_boxiness and m.header_flags(1) == {'1SERLAW': 'moffat'}
    assert np.array_equal(m._radial_values(m.values_batch(np.array([[10.0, 2.5, 4.0, 18.0]])), 1), [[2.5, 0.0]])
    assert Sersic(xy=(1, 1), mag=MAG, reff=3.0, reff_b=2.0, index=1.0, angle=0.0).header_flags(1) == {}
    assert psfmc_amd.Moffat is Moffat and psfmc_amd.Ferrer is Ferrer


def test_the_value_errors():
    with pytest.raises(TypeError, match='integrate'):
        moffat(integrate=True)
    with pytest.raises(TypeError, match='integrate'):
        ferrer(integrate=True)
    with pytest.raises(TypeError):
        moffat(reff=3.0)
    with pytest.raises(ValueError, match='pitch'):
        ferrer(spiral={'r_in': 1.0, 'r_out': 5.0, 'winding': 1.0, 'pitch': 0.3})
    with pytest.raises(ValueError, match='1 ... 6'):
        moffat(fourier={7: (0.1, 0.0)})
    with pytest.raises(ValueError, match='moffat, ferrer'):
        Sersic.radial_image('king', np.ones(9), (1.0, 1.0), 0.0, [], None, (8, 8))


def test_add_to_array_uses_the_definition_in_degrees_and_beside_the_other_keywords():
    f = ferrer(xy=(30.3, 28.6), r_out=25.0, r_out_b=10.0, angle=20.0, angle_degrees=True, boxiness=0.7,
               fourier={2: (0.2, 30.0)}, spiral={'r_in': 2.0, 'r_out': 9.0, 'winding': 150.0, 'inclination': 40.0})
    row = Sersic(xy=(30.3, 28.6), mag=MAG, reff=25.0, reff_b=10.0, index=1.0, angle=20.0,
                 angle_degrees=True).derived_row(ZP)
    assert np.array_equal(f.derived_row(ZP), row)
    want = Sersic.radial_image('ferrer', row, (2.0, 1.0), 0.7, [(2, 0.2, np.deg2rad(30.0))],
                               (2.0, 9.0, np.deg2rad(150.0), 0.0, np.deg2rad(40.0), 0.0), (64, 64))
    assert np.array_equal(image(f, (64, 64)), want) and want.max() > 0
    m = moffat(xy=(30.3, 28.6))
    row = Sersic(xy=(30.3, 28.6), mag=MAG, reff=9.0, reff_b=6.0, index=1.0, angle=0.4).derived_row(ZP)
    assert np.array_equal(image(m, (64, 64)), Sersic.radial_image('moffat', row, (3.5, 0.0), 0.0, [], None, (64, 64)))


# -- from the model file to the layouts ------------------------------------------------------------------------

class RecordingLayout(ts.RecordingLayout):
    def set_radial_layout(self, kinds, col, const):
        self.calls.append(('radial', (list(kinds), list(col), list(const))))


FERRER_TEXT = ('Ferrer(xy=Uniform(loc=c - ms, scale=2 * ms), mag=Uniform(loc=19.0, scale=5.0), '
               'r_out=Uniform(loc=5.0, scale=20.0), r_out_b=Uniform(loc=2.0, scale=10.0), alpha=Uniform(loc=0, scale=4), '
               'beta=Uniform(loc=-2, scale=3.5), angle=Uniform(loc=0, scale=180), angle_degrees=True, '
               'boxiness=Uniform(loc=-1, scale=2)%s)\n')
MOFFAT_TEXT = ('Moffat(xy=Uniform(loc=c - ms, scale=2 * ms), mag=Uniform(loc=19.0, scale=5.0), '
               'fwhm=Uniform(loc=1.0, scale=6.0), fwhm_b=2.0, beta=Uniform(loc=1.1, scale=8), angle=30.0, '
               'angle_degrees=True)\n')


def write_field(directory, more, **kw):
    path, fld = tg.write_field(directory, **kw)
    with open(path, 'a') as f:
        f.write(more)
    return path, fld


def test_model_file_round_trip_and_the_calls(tmp_path):
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN)
    plain = MultiComponentModel(path)
    path, _ = write_field(tmp_path, FERRER_TEXT % '' + MOFFAT_TEXT, sky_text=tg.SKY_PLAIN)
    model = MultiComponentModel(path)
    new = [n for n in model.param_names if n not in plain.param_names]
    assert new == ['3_Ferrer_alpha', '3_Ferrer_angle', '3_Ferrer_beta', '3_Ferrer_boxiness', '3_Ferrer_mag',
                   '3_Ferrer_r_out', '3_Ferrer_r_out_b', '3_Ferrer_xy', '4_Moffat_beta', '4_Moffat_fwhm', '4_Moffat_mag',
                   '4_Moffat_xy']
    assert [n for n in model.param_names if n not in new] == plain.param_names
    assert all(len(a) <= 8 for a in model.param_fits_abbrs)
    assert model.sersic_radial_kinds == [0, 2, 1] and model.sersic_general_flags == [False, True, True]
    assert model.sersic_spiral_flags == [False] * 3 and model.sersic_fourier_masks == [0] * 3 and model.has_aux
    assert model.header_flags() == {'3SERBOX': True, '3SERLAW': 'ferrer', '4SERLAW': 'moffat'}
    rec = RecordingLayout()
    model._register_layout(rec)
    # (no modes and no spiral: the library gives a field with a law both blocks itself)
    assert [c[0] for c in rec.calls] == ['layout', 'aux', 'radial']
    col = lambda n: tg.column_of(model, n)
    slot_col, slot_const = rec.calls[0][1][2], rec.calls[0][1][3]
    # slots: sky | ps mag x y | per Sersic angle index mag reff reff_b x y | psf
    assert slot_col[4:11] == [col('2_Sersic_' + n) for n in ('angle', 'index', 'mag', 'reff', 'reff_b')] + \
        [col('2_Sersic_xy'), col('2_Sersic_xy') + 1]
    assert slot_col[11:18] == [col('3_Ferrer_angle'), -1, col('3_Ferrer_mag'), col('3_Ferrer_r_out'),
                               col('3_Ferrer_r_out_b'), col('3_Ferrer_xy'), col('3_Ferrer_xy') + 1]
    assert slot_const[12] == 1.0
    assert slot_col[18:25] == [-1, -1, col('4_Moffat_mag'), col('4_Moffat_fwhm'), -1, col('4_Moffat_xy'),
                               col('4_Moffat_xy') + 1]
    assert slot_const[18:23] == [30.0, 1.0, 0.0, 0.0, 2.0]
    assert rec.calls[1][1] == ([-1, -1, -1, col('3_Ferrer_boxiness'), -1], [0.0] * 5, [False], [False, True, True])
    kinds, rcol, rconst = rec.calls[2][1]
    assert kinds == [0, 2, 1]
    assert rcol == [-1, -1, col('3_Ferrer_alpha'), col('3_Ferrer_beta'), col('4_Moffat_beta'), -1] and rconst == [0.0] * 6
    # aux rows: slope x 2, three boxinesses, 36 (empty) Fourier entries, 18 spiral entries inside the support, the six
    theta = np.arange(2.0 * model.num_params).reshape(2, -1) + 1.0
    aux = model.aux_rows(theta)
    assert aux.shape == (2, 2 + 21 * 3) and not aux[:, :3].any() and not aux[:, 5:41].any()
    assert np.array_equal(aux[:, 3], theta[:, col('3_Ferrer_boxiness')])
    assert np.array_equal(aux[:, 41:59], np.tile([0.0, 1.0, 0.0, 0.0, 0.0, 0.0], (2, 3)))
    assert np.array_equal(aux[:, 59:], np.c_[np.zeros((2, 2)), theta[:, [col('3_Ferrer_alpha'), col('3_Ferrer_beta'),
                                                                       col('4_Moffat_beta')]], np.zeros(2)])
    # host log-priors through the model: the support of the laws
    ok = np.array(model.init_params_from_priors(4))
    assert np.all(np.isfinite(model.log_priors_batch(ok)))
    ok[1, col('4_Moffat_beta')] = 1.0
    ok[2, col('3_Ferrer_beta')] = 2.0
    ok[3, col('3_Ferrer_r_out_b')] = ok[3, col('3_Ferrer_r_out')] + 1.0
    lp = model.log_priors_batch(ok)
    assert np.isfinite(lp[0]) and np.all(lp[1:] == -np.inf)
    # beside modes and a spiral: layout, aux, fourier, spiral, radial -- the radial call last
    path, _ = write_field(tmp_path, FERRER_TEXT % (", fourier={2: (Uniform(loc=-0.3, scale=0.6), 10.0)}" + ts.SPIRAL_TEXT),
                          sky_text=tg.SKY_PLAIN)
    both = MultiComponentModel(path)
    rec = RecordingLayout()
    both._register_layout(rec)
    assert [c[0] for c in rec.calls] == ['layout', 'aux', 'fourier', 'spiral', 'radial']
    assert both.header_flags() == {'3SERBOX': True, '3SERFOU': '2', '3SERSPI': True, '3SERLAW': 'ferrer'}


def test_a_model_without_the_classes_makes_exactly_the_calls_it_made(tmp_path):
    """`ts.RecordingLayout` has no `set_radial_layout` (a call would raise); the recorded calls of a boxiness + spiral
    model are those of the same model registered on an engine that has the method."""
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_TILTED,
                             sersic_text=', boxiness=Uniform(loc=-1, scale=2)' + ts.SPIRAL_TEXT)
    model = MultiComponentModel(path)
    old, new = ts.RecordingLayout(), RecordingLayout()
    model._register_layout(old)
    model._register_layout(new)
    assert [c[0] for c in old.calls] == ['layout', 'aux', 'spiral'] and model.sersic_radial_kinds == [0]
    assert repr(old.calls) == repr(new.calls)
    assert model.aux_rows(np.zeros((3, model.num_params))).shape == (3, 21)
    path, _ = tg.write_field(tmp_path, sky_text=tg.SKY_PLAIN)
    model = MultiComponentModel(path)
    rec = tg.RecordingLayout()
    model._register_layout(rec)
    assert [c[0] for c in rec.calls] == ['layout'] and model.aux_rows(np.zeros((1, model.num_params))) is None


def test_a_component_without_a_rasteriser_names_the_supported_ones(tmp_path):
    from psfmc_amd.ModelComponents.ComponentBase import ComponentBase
    path, _ = tg.write_field(tmp_path)
    comps = psfmc_amd.model_parser.component_list_from_file(path) + [ComponentBase()]
    with pytest.raises(NotImplementedError, match='Sersic, Moffat, Ferrer'):
        MultiComponentModel(comps)


def test_a_field_set_registers_the_laws_only_for_the_field_that_has_them(tmp_path):
    dirs = []
    for name, more, text in (('a', FERRER_TEXT % '', ''), ('b', '', ''), ('c', '', ts.SPIRAL_TEXT)):
        (tmp_path / name).mkdir()
        dirs.append(write_field(tmp_path / name, more, sky_text=tg.SKY_PLAIN, sersic_text=text)[0])
    for order in ((0, 1, 2), (1, 2, 0)):
        models = [MultiComponentModel(dirs[k]) for k in order]
        recs = [RecordingLayout() for _ in models]
        for m, rec in zip(models, recs):
            m._register_layout(rec)
        want = {0: ['layout', 'aux', 'radial'], 1: ['layout'], 2: ['layout', 'aux', 'spiral']}
        assert [[c[0] for c in rec.calls] for rec in recs] == [want[k] for k in order]
        assert [any(m.sersic_radial_kinds) for m in models] == [k == 0 for k in order]


def test_joint_model_shares_the_ferrer_beta_and_keeps_r_out_per_field(tmp_path):
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    a = MultiComponentModel(write_field(tmp_path / 'a', FERRER_TEXT % '', sky_text=tg.SKY_PLAIN)[0])
    b = MultiComponentModel(write_field(tmp_path / 'b', FERRER_TEXT % '', sky_text=tg.SKY_PLAIN)[0])
    joint = JointModel([a, b], per_field=['3_Ferrer_r_out'])
    assert joint.param_names.count('3_Ferrer_beta') == 1 and '3_Ferrer_r_out' not in joint.param_names
    assert '3_Ferrer_r_out_f0' in joint.param_names and '3_Ferrer_r_out_f1' in joint.param_names
    assert joint.header_flags() == {'3SERBOX': True, '3SERLAW': 'ferrer'}
    sent, radii = [], []
    for f, m in enumerate(joint.field_models):
        rec = RecordingLayout()
        m._register_layout(rec, columns=joint.field_columns(f), n_params=joint.num_params)
        assert [c[0] for c in rec.calls] == ['layout', 'aux', 'radial']
        sent.append(rec.calls[2][1][1])
        radii.append(rec.calls[0][1][2][14])                                   # the Ferrer slot's reff place
    assert sent[0] == sent[1] and sent[0][2] >= 0 and sent[0][3] >= 0 and radii[0] != radii[1]
    theta = np.zeros((2, joint.num_params))
    # (the draws come from numpy's global generator: seeded here, because field 0's own r_out beside field 1's draw of
    # the shared r_out_b is inside the support for some draws only, and the state a test inherits depends on which
    # tests ran before it -- a run of every test on a GPU machine met r_out < r_out_b here)
    np.random.seed(3)
    for f in range(2):
        theta[:, joint.field_columns(f)] = joint.field_models[f].init_params_from_priors(2)
    assert np.all(np.isfinite(joint.log_priors_batch(theta)))
    theta[1, joint.param_names.index('3_Ferrer_r_out_f1')] = 1.0               # below r_out_b (>= 2): outside
    assert joint.log_priors_batch(theta)[1] == -np.inf


def test_database_round_trip_of_the_columns_and_the_flag(tmp_path):
    from psfmc_amd import database
    path, _ = write_field(tmp_path, FERRER_TEXT % '' + MOFFAT_TEXT, sky_text=tg.SKY_PLAIN)
    model = MultiComponentModel(path)

    class Chain(object):
        chain = np.arange(4.0 * 3 * model.num_params).reshape(4, 3, model.num_params)
        lnprobability = np.zeros((4, 3))
    table = database.save_database(Chain(), model, str(tmp_path / 'db.fits'))
    back = database.load_database(str(tmp_path / 'db.fits'))
    for t in (table, back):
        assert t.meta['3SERLAW'] == 'ferrer' and t.meta['4SERLAW'] == 'moffat' and t.meta['3SERBOX'] in (True, 'T')
    names = ['3_Ferrer_alpha', '3_Ferrer_beta', '3_Ferrer_r_out', '3_Ferrer_r_out_b', '4_Moffat_beta', '4_Moffat_fwhm']
    for n in names:
        assert n in back.colnames and np.array_equal(np.ravel(back[n]), np.ravel(table[n]))
