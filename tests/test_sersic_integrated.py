"""The pixel-integrated Sersic profile (`Sersic(..., integrate=True)`) on the host: the numpy definition
(`Sersic.integrated_image`) against GALFIT's renderings and against the same scheme with every constant pushed far
up, and the keyword's way from a model file to the packed layout.  No GPU needed; the device is held to the same
definition in tests/test_gpu_sersic_integrated.py."""
import os

import numpy as np
import pytest

import helpers
import synth_field
from psfmc_amd import MultiComponentModel, fits_io
from psfmc_amd.ModelComponents import Sersic
from psfmc_amd.models import FieldSet, JointModel

GALFIT = np.load(os.path.join(helpers.GOLDEN, 'galfit.npz'))
TAGS = ('0p5', '1p0', '3p1', '4p0', '6p5')
# The contract against the GALFIT fixtures, pixels brighter than 1e-3 of the peak: (max relative error, median
# relative error, total-flux error) as MEASURED ("Pixel-integrated Sersic profile"); asserted at twice
# these (the fixtures are float32 and GALFIT's own quadrature has a floor).
GALFIT_MEASURED = {
    '0p5': (1.464e-02, 3.626e-03, 1.159e-03),
    '1p0': (3.975e-03, 2.712e-03, 8.055e-04),
    '3p1': (2.961e-03, 7.003e-04, 3.218e-04),
    '4p0': (2.931e-03, 6.560e-04, 3.458e-04),
    '6p5': (9.885e-03, 5.778e-04, 1.713e-03),
}


def galfit_component(tag, integrate):
    xc, yc, mag, re, n, ar, pa, zp = GALFIT['pars_' + tag]
    comp = Sersic(xy=(xc - 1, yc - 1), mag=mag, reff=re, reff_b=re * ar, index=n, angle=pa, angle_degrees=True,
                  integrate=integrate)
    return comp, zp


@pytest.mark.parametrize('tag', TAGS)
def test_contract_against_galfit(tag):
    ref = GALFIT['galfit_' + tag].astype(np.float64)
    comp, zp = galfit_component(tag, True)
    new = comp.add_to_array(np.zeros(ref.shape), zp)
    plain, _ = galfit_component(tag, False)
    old = plain.add_to_array(np.zeros(ref.shape), zp)
    # the default mode's host meaning is the reference's formula: the fixture's own psfmc_* image
    fixture = GALFIT['psfmc_' + tag]
    ok = np.isfinite(fixture)
    assert np.max(np.abs(old[ok] - fixture[ok]) / np.abs(fixture[ok])) <= 1e-12
    sel = ref > 1e-3 * ref.max()
    err_new, err_old = np.abs(new - ref)[sel] / ref[sel], np.abs(old - ref)[sel] / ref[sel]
    flux_new = abs(new.sum() - ref.sum()) / ref.sum()
    flux_old = abs(old.sum() - ref.sum()) / ref.sum()
    print('n=%s: max %.3e (formula %.3e)  median %.3e  flux %.3e (formula %.3e)'
          % (tag, err_new.max(), err_old.max(), np.median(err_new), flux_new, flux_old))
    m_max, m_med, m_flux = GALFIT_MEASURED[tag]
    assert err_new.max() <= 2 * m_max
    assert np.median(err_new) <= 2 * m_med
    assert flux_new <= 2 * m_flux
    # whatever the measurement: closer than the reference formula in the worst pixel in all five cases, and in
    # total flux except at n = 6.5 (where the formula's 3e-4 is a cancellation)
    assert err_new.max() < err_old.max()
    if tag != '6p5':
        assert flux_new < flux_old


# (name, r_e, b/a, n, centre): a small host, an on-pixel centre, a high index on a pixel corner, a flat profile, an
# elongated one, a centre on a pixel edge; then the MEASURED (max relative error over pixels above 1e-4 of the peak,
# total-flux error) of the contract against the converged scheme, asserted at 1.5 times these
CONVERGENCE = [
    ('small host', 2.0, 0.6, 4.0, (31.3, 32.7), (7.248e-03, 1.779e-03)),
    ('small host, on-pixel centre', 1.5, 0.9, 1.0, (32.0, 32.0), (3.195e-03, 8.532e-04)),
    ('high index, pixel corner', 4.0, 0.5, 6.5, (31.5, 31.5), (6.073e-03, 6.691e-04)),
    ('flat', 10.0, 0.7, 0.5, (30.2, 33.9), (1.045e-04, 1.097e-05)),
    ('elongated', 6.3, 0.5, 4.0, (31.3, 32.7), (4.800e-03, 5.630e-04)),
    ('pixel edge', 3.0, 0.8, 2.5, (31.5, 32.2), (2.699e-03, 4.697e-04)),
]


@pytest.mark.parametrize('name,re,ar,n,xy,measured', CONVERGENCE, ids=[c[0] for c in CONVERGENCE])
def test_contract_against_converged_quadrature(name, re, ar, n, xy, measured):
    comp = Sersic(xy=xy, mag=20.0, reff=re, reff_b=re * ar, index=n, angle=25.0, angle_degrees=True, integrate=True)
    row = comp.derived_row(26.0)
    shape = (64, 64)
    fine = Sersic.integrated_image(row, shape, half_box=10, grid=lambda d: 24, split=4, levels=14, sub=8)
    got = Sersic.integrated_image(row, shape)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(fine))
    sel = fine > 1e-4 * fine.max()
    err = (np.abs(got - fine) / fine)[sel].max()
    flux = abs(got.sum() - fine.sum()) / fine.sum()
    print('%s: max rel %.3e  flux %.3e' % (name, err, flux))
    assert err <= 1.5 * measured[0]
    assert flux <= 1.5 * measured[1]
    assert err <= 1e-2                    # (the small hosts: enlarge the constants rather than this)


def test_last_level_and_sample_on_the_centre():
    """The refinement's last level samples every sub-cell on an even grid, which never holds its cell's centre,
    edges or corners; a centre that coincides with a sample all the same meets the profile's finite peak."""
    comp = Sersic(xy=(8.0, 8.0), mag=20.0, reff=3.0, reff_b=2.0, index=4.0, angle=0.3, integrate=True)
    row = comp.derived_row(26.0)
    peak = Sersic._plain(row, np.array(8.0), np.array(8.0))[0]
    assert np.isfinite(peak) and peak == row[8] * np.exp(row[6])
    with pytest.raises(ValueError):
        Sersic.integrated_image(row, (16, 16), sub=3)
    # one level only: the cell that holds the centre is sampled at the last level, on points off the centre
    coarse = Sersic.integrated_image(row, (16, 16), levels=0)
    assert np.all(np.isfinite(coarse))
    # a centre put exactly on a last-level sample: sample (k + 1/2) / 4 of the last level's sub-cells, pitch 4^-(L+1)
    from psfmc_amd.ModelComponents.Sersic import INTEG_LEVELS, INTEG_SPLIT, INTEG_SUB
    pitch = float(INTEG_SPLIT) ** -(INTEG_LEVELS + 1)
    comp.xy = (8.0 - 0.5 + 0.5 / INTEG_SUB * pitch, 8.0)
    img = Sersic.integrated_image(comp.derived_row(26.0), (16, 16))
    assert np.all(np.isfinite(img)) and img[8, 8] < peak


def test_on_pixel_centre_is_finite_only_with_the_keyword():
    args = dict(xy=(10.0, 12.0), mag=21.0, reff=4.0, reff_b=3.0, index=2.5, angle=40.0, angle_degrees=True)
    default = Sersic(**args).add_to_array(np.zeros((24, 24)), 26.0)
    assert np.isnan(default[12, 10]) and np.isfinite(np.delete(default.ravel(), 12 * 24 + 10)).all()
    integ = Sersic(integrate=True, **args).add_to_array(np.zeros((24, 24)), 26.0)
    assert np.all(np.isfinite(integ)) and integ[12, 10] == integ.max()
    # away from the core both are the plain profile times a second-order term of a per cent or so (1-D against 2-D):
    # they agree to the size of that term
    far = np.hypot(*np.mgrid[0:24, 0:24] - np.array([12, 10])[:, None, None]) > 6
    assert np.max(np.abs(integ[far] - default[far]) / default[far]) < 2e-2


def test_centre_outside_the_image_clips_the_box():
    comp = Sersic(xy=(-1.6, 5.2), mag=20.0, reff=5.0, reff_b=4.0, index=1.5, angle=0.0, integrate=True)
    img = comp.add_to_array(np.zeros((16, 16)), 26.0)
    assert np.all(np.isfinite(img)) and np.all(img > 0)
    comp.xy = (-40.0, 50.0)
    assert np.all(np.isfinite(comp.add_to_array(np.zeros((16, 16)), 26.0)))


# -- the keyword from the model file to the packed layout ---------------------------------------------------

def write_field(directory, side=64, integrate_text=', integrate=True', n_sersic=1):
    fld = synth_field.make_field(side, n_sersic, seed=0)
    for key, name in (('sci', 'sci.fits'), ('ivm', 'ivm.fits'), ('psf', 'psf.fits'), ('psf_ivm', 'psf_ivm.fits')):
        fits_io.write_image(os.path.join(str(directory), name), fld[key])
    text = synth_field.model_file_text(side, n_sersic).replace('angle_degrees=True)',
                                                              'angle_degrees=True%s)' % integrate_text)
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


def test_keyword_default_and_model_file(tmp_path):
    assert Sersic(xy=(1, 2), mag=20, reff=3, reff_b=2, index=1, angle=0).integrate is False
    path, _ = write_field(tmp_path, integrate_text='')
    model = MultiComponentModel(path)
    assert model.sersic_integrate == [False] and model.header_flags() == {}
    rec = RecordingLayout()
    model._register_layout(rec)
    assert [c[0] for c in rec.calls] == ['layout']         # a model without the keyword makes the calls it made

    path, _ = write_field(tmp_path, integrate_text=', integrate=True')
    model = MultiComponentModel(path)
    assert model.sersic_integrate == [True]
    rec = RecordingLayout()
    model._register_layout(rec)
    assert rec.calls[0] == ('integrate', [True]) and rec.calls[1][0] == 'layout'
    # the flag is no free parameter, and the database header records it beside the component's keys
    assert model.num_params == 10 and not any('integrate' in n for n in model.param_names)
    assert model.header_flags() == {'1SERINT': True}


def test_mixed_components_keep_their_own_flags(tmp_path):
    path, _ = write_field(tmp_path, n_sersic=2, integrate_text='')
    with open(path) as f:
        text = f.read()
    head, _, tail = text.rpartition('angle_degrees=True)')
    with open(path, 'w') as f:
        f.write(head + 'angle_degrees=True, integrate=True)' + tail)
    model = MultiComponentModel(path)
    assert model.sersic_integrate == [False, True]
    assert model.header_flags() == {'2SERINT': True}


def test_joint_model_and_field_set_keep_per_field_flags(tmp_path):
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    path_a, _ = write_field(tmp_path / 'a', integrate_text=', integrate=True')
    path_b, _ = write_field(tmp_path / 'b', integrate_text=', integrate=False')
    a, b = MultiComponentModel(path_a), MultiComponentModel(path_b)
    joint = JointModel([a, b])
    assert [m.sersic_integrate for m in joint.field_models] == [[True], [False]]
    assert joint.header_flags() == {'1SERINT': 'TF'}
    sent = []
    for m in joint.field_models:
        rec = RecordingLayout()
        m._register_layout(rec, columns=joint.field_columns(0), n_params=joint.num_params)
        sent.append([c for c in rec.calls if c[0] == 'integrate'])
    assert sent == [[('integrate', [True])], []]
    # (a FieldSet registers its fields through the same `_register_layout`, one proxy per field)
    assert FieldSet.__init__.__code__.co_names.count('_register_layout') == 1


def test_database_header_records_the_flag(tmp_path):
    from psfmc_amd.database import load_database, save_database

    class Chain(object):
        chain = np.zeros((2, 3, 10))
        lnprobability = np.arange(6.0).reshape(2, 3)
    for text, want in ((', integrate=True', True), ('', None)):
        path, _ = write_field(tmp_path, integrate_text=text)
        model = MultiComponentModel(path)
        db = save_database(Chain(), model, os.path.join(str(tmp_path), 'db%d.fits' % bool(want)))
        assert db.meta.get('1SERINT') == want
        assert load_database(os.path.join(str(tmp_path), 'db%d.fits' % bool(want))).meta.get('1SERINT') == want
