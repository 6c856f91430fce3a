"""Boxy / disky Sersic isophotes (`Sersic(..., boxiness=...)`) and the tilted sky (`Sky(..., slope=...)`) on the
host: the numpy definitions (`Sersic.general_image`, `Sky.tilted_image`) and the keywords' way from a model file to
the packed layout and the auxiliary-parameter layout.  No GPU needed; the device is held to the same definitions in
tests/test_gpu_general_components.py."""
import os

import numpy as np
import pytest

import helpers
import psfmc_oracle as orc
import synth_field
from psfmc_amd import MultiComponentModel, fits_io
from psfmc_amd.ModelComponents import Configuration, PointSource, Sersic, Sky
from psfmc_amd.distributions import Normal, Uniform
from psfmc_amd.models import JointModel

GALFIT = np.load(os.path.join(helpers.GOLDEN, 'galfit.npz'))
TAGS = ('0p5', '1p0', '3p1', '4p0', '6p5')
# general_image at c = 0 against the oracle's Sersic image on the five GALFIT parameter sets: the MEASURED maximum
# relative difference over the finite pixels (two formulations of one expression: |u|^2 through a power, A(0) through
# lgamma; DESIGN.md, "General components"), asserted at ten times it
C0_MEASURED = 1.7e-13


# -- the keywords from the model file to the layouts -----------------------------------------------------------

def write_field(directory, side=64, sky_text=None, sersic_text=''):
    fld = synth_field.make_field(side, 1, seed=0)
    for key, name in (('sci', 'sci.fits'), ('ivm', 'ivm.fits'), ('psf', 'psf.fits'), ('psf_ivm', 'psf_ivm.fits')):
        fits_io.write_image(os.path.join(str(directory), name), fld[key])
    text = synth_field.model_file_text(side, 1).replace('angle_degrees=True)', 'angle_degrees=True%s)' % sersic_text)
    if sky_text is not None:
        text = text.replace('PointSource(', sky_text + '\nPointSource(', 1)
    path = os.path.join(str(directory), 'model.py')
    with open(path, 'w') as f:
        f.write(text)
    return path, fld


class RecordingLayout(object):
    """Stands in for an engine context: keeps what `_register_layout` sends."""

    def __init__(self):
        self.calls = []

    def set_layout(self, *args):
        self.calls.append(('layout', args))

    def set_priors(self, *args):
        self.calls.append(('priors', args))

    def set_sersic_integrate(self, flags):
        self.calls.append(('integrate', list(flags)))

    def set_aux_layout(self, aux_col, aux_const, sky_flags, sersic_flags):
        self.calls.append(('aux', (list(aux_col), list(aux_const), list(sky_flags), list(sersic_flags))))


def column_of(model, name):
    """First theta column of a named parameter."""
    return int(np.concatenate([[0], np.cumsum(model.param_lens)])[model.param_names.index(name)])


SKY_PLAIN = 'Sky(adu=Normal(loc=0, scale=0.01))'
SKY_TILTED = 'Sky(adu=Normal(loc=0, scale=0.01), slope=Normal(loc=(0, 0), scale=(1e-4, 1e-4)))'


def test_model_file_parses_and_names_follow_component_order(tmp_path):
    path, _ = write_field(tmp_path, sky_text=SKY_PLAIN)
    plain = MultiComponentModel(path)
    path, _ = write_field(tmp_path, sky_text=SKY_TILTED, sersic_text=', boxiness=Uniform(loc=-1, scale=2)')
    model = MultiComponentModel(path)
    new = [n for n in model.param_names if n not in plain.param_names]
    assert new == ['0_Sky_slope', '2_Sersic_boxiness']
    assert [n for n in model.param_names if n not in new] == plain.param_names
    # alphabetical inside the component, components in file order
    assert model.param_names[:2] == ['0_Sky_adu', '0_Sky_slope']
    assert model.param_names[model.param_names.index('2_Sersic_angle') + 1] == '2_Sersic_boxiness'
    assert model.num_params == plain.num_params + 3
    abbrs = dict(zip(model.param_names, model.param_fits_abbrs))
    assert abbrs['0_Sky_slope'] == '0Sky_SLP' and abbrs['2_Sersic_boxiness'] == '2SER_BOX'
    assert all(len(a) <= 8 for a in abbrs.values())
    assert model.sky_slope_flags == [True] and model.sersic_general_flags == [True] and model.has_aux
    assert model.header_flags() == {'0SKYSLP': True, '2SERBOX': True}
    rec = RecordingLayout()
    model._register_layout(rec)
    assert [c[0] for c in rec.calls] == ['layout', 'aux']
    # theta columns: adu, slope x 2, ps mag x y, then the Sersic's angle, boxiness, ...
    box = column_of(model, '2_Sersic_boxiness')
    assert box == 7 and rec.calls[1][1] == ([1, 2, box], [0.0, 0.0, 0.0], [True], [True])
    # the main slots do not know the new columns
    main_cols = list(rec.calls[0][1][2])
    assert 1 not in main_cols and 2 not in main_cols and box not in main_cols


def test_a_model_without_the_keywords_is_the_parents(tmp_path):
    path, _ = write_field(tmp_path, sky_text=SKY_PLAIN)
    model = MultiComponentModel(path)
    assert model.param_names == ['0_Sky_adu', '1_PointSource_mag', '1_PointSource_xy', '2_Sersic_angle',
                                 '2_Sersic_index', '2_Sersic_mag', '2_Sersic_reff', '2_Sersic_reff_b', '2_Sersic_xy']
    assert not model.has_aux and model.header_flags() == {} and model.aux_rows(np.zeros((2, 11))) is None
    rec = RecordingLayout()
    model._register_layout(rec)
    assert [c[0] for c in rec.calls] == ['layout']
    assert list(rec.calls[0][1][2]) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, -1]

    class RowEngine(object):                      # the row-based calls carry no new keyword either
        def loglike(self, rows, skip):
            return np.zeros(len(rows))

        def images(self, rows, kinds):
            return {'raw_model': np.zeros((len(rows), 2, 2))}
    model._engine = RowEngine()
    theta = np.tile(np.r_[0.0, synth_field.make_field(64, 1)['truth']], (2, 1))
    assert model.log_likelihood_batch(theta).shape == (2,)
    assert model.sample_images(theta, ('raw_model',))['raw_model'].shape == (2, 2, 2)
    model._engine = None


def test_fixed_values_still_select_the_new_path(tmp_path):
    path, _ = write_field(tmp_path, sky_text='Sky(adu=Normal(loc=0, scale=0.01), slope=(0, 0))',
                          sersic_text=', boxiness=0.0')
    model = MultiComponentModel(path)
    path, _ = write_field(tmp_path, sky_text=SKY_PLAIN)
    assert model.param_names == MultiComponentModel(path).param_names
    rec = RecordingLayout()
    model._register_layout(rec)
    assert rec.calls[-1] == ('aux', ([-1, -1, -1], [0.0, 0.0, 0.0], [True], [True]))
    aux = model.aux_rows(np.zeros((3, model.num_params)))
    assert aux.shape == (3, 3) and not aux.any()
    assert model.header_flags() == {'0SKYSLP': True, '2SERBOX': True}


def test_aux_rows_follow_theta(tmp_path):
    path, _ = write_field(tmp_path, sky_text=SKY_TILTED, sersic_text=', boxiness=Uniform(loc=-1, scale=2)')
    model = MultiComponentModel(path)
    theta = np.arange(2.0 * model.num_params).reshape(2, -1)
    box = column_of(model, '2_Sersic_boxiness')
    assert np.array_equal(model.aux_rows(theta), theta[:, [1, 2, box]])


def test_joint_model_links_and_unlinks_the_new_parameters(tmp_path):
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    kw = dict(sky_text=SKY_TILTED, sersic_text=', boxiness=Uniform(loc=-1, scale=2)')
    a = MultiComponentModel(write_field(tmp_path / 'a', **kw)[0])
    b = MultiComponentModel(write_field(tmp_path / 'b', **kw)[0])
    joint = JointModel([a, b], per_field=['0_Sky_slope'])
    assert '0_Sky_slope_f0' in joint.param_names and '0_Sky_slope_f1' in joint.param_names
    assert joint.param_names.count('2_Sersic_boxiness') == 1
    assert joint.header_flags() == {'0SKYSLP': True, '2SERBOX': True}
    sent = []
    for f, m in enumerate(joint.field_models):
        rec = RecordingLayout()
        m._register_layout(rec, columns=joint.field_columns(f), n_params=joint.num_params)
        assert [c[0] for c in rec.calls] == ['layout', 'aux']
        sent.append(rec.calls[1][1][0])
    assert sent[0][:2] != sent[1][:2] and sent[0][2] == sent[1][2]        # own slopes, one boxiness
    # a shared boxiness needs equal priors
    c = MultiComponentModel(write_field(tmp_path / 'b', sky_text=SKY_TILTED,
                                        sersic_text=', boxiness=Uniform(loc=-0.5, scale=1)')[0])
    with pytest.raises(ValueError, match='boxiness'):
        JointModel([a, c])


# -- general_image ------------------------------------------------------------------------------------------

def galfit_row(tag):
    xc, yc, mag, re, n, ar, pa, zp = GALFIT['pars_' + tag]
    comp = Sersic(xy=(xc - 1, yc - 1), mag=mag, reff=re, reff_b=re * ar, index=n, angle=pa, angle_degrees=True)
    return comp.derived_row(zp), dict(xy=(xc - 1, yc - 1), mag=mag, reff=re, reff_b=re * ar, index=n, angle=pa), zp


def test_general_image_at_zero_is_the_reference_formula():
    worst = 0.0
    for tag in TAGS:
        row, pars, zp = galfit_row(tag)
        shape = GALFIT['galfit_' + tag].shape
        want = orc.add_sersic(np.zeros(shape), pars['xy'], pars['mag'], pars['reff'], pars['reff_b'], pars['index'],
                              pars['angle'], True, zp, orc.array_coords(shape))
        got = Sersic.general_image(row, 0.0, shape)
        ok = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), ok)
        err = np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))
        print('n=%s: general_image(c=0) against the oracle, max relative difference %.3e' % (tag, err))
        worst = max(worst, err)
    assert worst <= 10 * C0_MEASURED


NORM_ROW = dict(xy=(127.3, 128.6), mag=18.0, reff=12.0, reff_b=8.0, index=1.0, angle=0.6)


def test_total_flux_does_not_depend_on_the_boxiness():
    """The image sum at c in {-1, -0.5, 0.5, 1, 2} is within 2e-3 of the c = 0 sum (1.44e-3 at c = -1 as computed
    with numpy; without 1 / A(c) the ratio would be A(c): 0.64 at c = -1)."""
    row = Sersic(**NORM_ROW).derived_row(25.0)
    base = Sersic.general_image(row, 0.0, (256, 256)).sum()
    for c in (-1.0, -0.5, 0.5, 1.0, 2.0):
        ratio = Sersic.general_image(row, c, (256, 256)).sum() / base
        print('c = %+.1f: sum / sum(c = 0) - 1 = %+.3e   A(c) = %.4f' % (c, ratio - 1, Sersic.superellipse_area_ratio(c)))
        assert abs(ratio - 1) <= 2e-3
    assert abs(Sersic.superellipse_area_ratio(0.0) - 1) <= 1e-15
    assert abs(Sersic.superellipse_area_ratio(-1.0) - 2 / np.pi) <= 1e-15          # the diamond |u| + |v| = 1
    assert abs(Sersic.superellipse_area_ratio(1e9) - 4 / np.pi) <= 1e-8            # the square


def test_shape_boxy_disky_and_reflections():
    """Round, axis-aligned component (angle -pi/2: u along x, v along y), centre on a pixel corner: at the
    elliptical radius of the axis pixel, the value on the 45-degree diagonal relative to the value on the axis
    -- normalisation out -- is larger for c > 0 and smaller for c < 0; the image has the component's reflections."""
    comp = Sersic(xy=(31.5, 31.5), mag=18.0, reff=6.0, reff_b=6.0, index=1.5, angle=-0.5 * np.pi)
    row = comp.derived_row(25.0)
    assert abs(row[3]) < 1e-15 and abs(row[4]) < 1e-15
    ratio = {}
    for c in (-1.0, -0.4, 0.0, 0.6, 2.0):
        img = Sersic.general_image(row, c, (64, 64))
        assert np.all(np.isfinite(img))
        assert np.allclose(img, img[::-1, :], rtol=1e-13, atol=0) and np.allclose(img, img[:, ::-1], rtol=1e-13, atol=0)
        assert np.allclose(img, img.T, rtol=1e-13, atol=0)
        # pixel (36, 36) is at Euclidean distance 4.5 sqrt 2 = 6.36 on the diagonal; pixel (38, 32) at (6.5, 0.5):
        # distance 6.52 -- compare through the exact radial profile instead: on-axis value at the same rho
        sb = row[8] / Sersic.superellipse_area_ratio(c)
        rho = 4.5 * np.sqrt(2.0) / 6.0
        on_axis = sb * np.exp(-row[6] * np.expm1(np.log(rho ** 2) * row[7]))       # (|u|^e)^(2/e) = u^2 for every c
        ratio[c] = img[36, 36] / on_axis
    assert ratio[-1.0] < ratio[-0.4] < ratio[0.0] < ratio[0.6] < ratio[2.0]
    assert abs(ratio[0.0] - 1) < 2e-2                                             # (the centroid term only)
    # a rotated, flattened component keeps its point symmetry about a half-pixel centre
    comp = Sersic(xy=(31.5, 31.5), mag=18.0, reff=9.0, reff_b=4.0, index=2.0, angle=0.4)
    img = Sersic.general_image(comp.derived_row(25.0), 0.8, (64, 64))
    assert np.allclose(img, img[::-1, ::-1], rtol=1e-13, atol=0)


def test_zero_coordinate_and_on_pixel_centre():
    """A centre at x + 0.5 on a pixel row (u or v exactly 0 along a line) is finite; an on-pixel centre stays NaN."""
    comp = Sersic(xy=(10.5, 12.0), mag=18.0, reff=5.0, reff_b=5.0, index=1.0, angle=-0.5 * np.pi)
    for c in (-1.0, 0.0, 0.7, 2.0):
        assert np.all(np.isfinite(Sersic.general_image(comp.derived_row(25.0), c, (24, 24))))
    comp = Sersic(xy=(10.0, 12.0), mag=18.0, reff=5.0, reff_b=3.0, index=1.0, angle=0.3)
    img = Sersic.general_image(comp.derived_row(25.0), 0.7, (24, 24))
    assert np.isnan(img[12, 10]) and np.isnan(img).sum() == 1


def test_add_to_array_uses_the_definitions():
    args = dict(xy=(11.3, 12.8), mag=20.0, reff=4.0, reff_b=3.0, index=2.0, angle=0.3)
    comp = Sersic(boxiness=0.5, **args)
    want = Sersic.general_image(Sersic(**args).derived_row(26.0), 0.5, (24, 24))
    assert np.array_equal(comp.add_to_array(np.zeros((24, 24)), 26.0), want)
    sky = Sky(adu=0.3, slope=(1e-3, -2e-3))
    assert np.array_equal(sky.add_to_array(np.zeros((6, 9))), Sky.tilted_image(0.3, (1e-3, -2e-3), (6, 9)))
    assert np.array_equal(Sky(adu=0.3).add_to_array(np.zeros((6, 9))), np.full((6, 9), 0.3))


# -- tilted_image --------------------------------------------------------------------------------------------

def test_tilted_image_is_a_plane_through_the_centre():
    for shape in ((7, 9), (8, 10), (7, 10)):
        img = Sky.tilted_image(0.25, (0.5, -0.125), shape)          # (values exact in binary)
        ny, nx = shape
        yy, xx = np.mgrid[0:ny, 0:nx]
        assert np.array_equal(img, 0.25 + 0.5 * (xx - (nx - 1) / 2) - 0.125 * (yy - (ny - 1) / 2))
        assert np.array_equal(np.diff(img, axis=1), np.full((ny, nx - 1), 0.5))
        assert np.array_equal(np.diff(img, axis=0), np.full((ny - 1, nx), -0.125))
        # the level is the value at the image centre: a pixel of odd sides, the mean of the central ones otherwise
        centre = img[(ny - 1) // 2:ny // 2 + 1, (nx - 1) // 2:nx // 2 + 1].mean()
        assert centre == 0.25 and img.mean() == 0.25
    assert np.array_equal(Sky.tilted_image(0.25, (0, 0), (5, 6)), np.full((5, 6), 0.25))


# -- guards ---------------------------------------------------------------------------------------------------

def host_model(boxiness, slope=None):
    fld = synth_field.make_field(64, 1, seed=0)
    c = np.array((32.5, 32.5))
    comps = [Configuration(fld['sci'], fld['ivm'], fld['psf'], fld['psf_ivm'], mag_zeropoint=fld['mag_zp']),
             Sky(adu=Normal(loc=0, scale=0.01), **({} if slope is None else {'slope': slope})),
             PointSource(xy=Uniform(loc=c - 8, scale=16 * np.ones(2)), mag=Uniform(loc=18.0, scale=2.0)),
             Sersic(xy=Uniform(loc=c - 8, scale=16 * np.ones(2)), mag=Uniform(loc=19.0, scale=5.0),
                    reff=Uniform(loc=2.0, scale=4.0), reff_b=Uniform(loc=2.0, scale=4.0),
                    index=Uniform(loc=0.5, scale=6), angle=Uniform(loc=0, scale=180), angle_degrees=True,
                    boxiness=boxiness)]
    return MultiComponentModel(comps, backend='fused', max_walkers=8), fld


def test_boxiness_outside_its_support_is_minus_infinity_on_the_host():
    model, fld = host_model(Uniform(loc=-3, scale=6))
    theta = np.tile(np.r_[0.001, fld['truth']], (4, 1))
    theta = np.insert(theta, column_of(model, '2_Sersic_boxiness'), [0.3, -2.0, -2.5, np.nan], axis=1)
    assert theta.shape[1] == model.num_params
    lp = model.log_priors_batch(theta)
    assert np.isfinite(lp[0]) and lp[1] == -np.inf and lp[2] == -np.inf and not np.isfinite(lp[3])
    model.param_values = theta[1]
    assert model.log_priors() == -np.inf
    model.param_values = theta[0]
    assert np.isfinite(model.log_priors())

    class NoDevice(object):                       # every walker outside the support: the host path asks nothing
        def loglike(self, *args, **kwargs):
            raise AssertionError('a skipped walker reached the device')
    model._engine = NoDevice()
    assert np.all(model.log_posterior_batch_host(theta[1:3]) == -np.inf)
    model._engine = None
    # a fixed boxiness outside the support too
    fixed, _ = host_model(-2.0)
    assert np.all(fixed.log_priors_batch(np.tile(np.r_[0.001, fld['truth']], (2, 1))) == -np.inf)


def test_boxiness_with_integrate_raises():
    args = dict(xy=(1, 2), mag=20, reff=3, reff_b=2, index=1, angle=0)
    with pytest.raises(ValueError, match='boxiness'):
        Sersic(integrate=True, boxiness=0.0, **args)
    with pytest.raises(ValueError, match='boxiness'):
        Sersic(integrate=True, boxiness=Uniform(loc=-1, scale=2), **args)
    assert Sersic(integrate=True, **args).has_boxiness is False
    assert Sersic(boxiness=0.0, **args).header_flags(3) == {'3SERBOX': True}
    with pytest.raises(ValueError, match='two'):
        Sky(adu=0.0, slope=1e-3)


def test_database_header_records_the_flags(tmp_path):
    from psfmc_amd.database import load_database, save_database
    for k, (sky, ser, want) in enumerate(((SKY_TILTED, ', boxiness=Uniform(loc=-1, scale=2)', (True, True)),
                                          (SKY_PLAIN, ', boxiness=0.0', (None, True)),
                                          (SKY_PLAIN, '', (None, None)))):
        path, _ = write_field(tmp_path, sky_text=sky, sersic_text=ser)
        model = MultiComponentModel(path)

        class Chain(object):
            chain = np.zeros((2, 3, model.num_params))
            lnprobability = np.arange(6.0).reshape(2, 3)
        name = os.path.join(str(tmp_path), 'db%d.fits' % k)
        db = save_database(Chain(), model, name)
        for meta in (db.meta, load_database(name).meta):
            assert (meta.get('0SKYSLP'), meta.get('2SERBOX')) == want
        if want[0]:
            assert '0_Sky_slope' in db.colnames and '2_Sersic_boxiness' in db.colnames      # ordinary columns
