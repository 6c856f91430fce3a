"""psfmc_fisher_rows for the fields of a set: `FieldSetContext.fisher_rows`, `FieldView.fisher_rows` and therefore
`fs.models[f].fisher(theta)`, for every field of a mixed-shape `FieldSet` -- field 0 included.

Three fields of different image and PSF sizes in one shared transform: 62 x 66 (PSF side 21; 4092 pixels, not whole
slabs of 64), 70 x 64 (17; with a mask, weights <= 0 and NaN pixels) and 64 x 64 (11).  Each has two PSFs, whose
free index is not a differentiated column; the walkers of field f use its PSF f % 2, so that a field's
`field * n_psf_field` offset into the kernel spectra counts.  A FieldSet's fields share their component lists, so
every field carries the sky, the point source and the Sersic.

Per field: F and g within `fisher_error_bound` of the definition on the ORACLE's images of that field (a bound, not
bit equality: the shared transform is not the field's own); within `fisher_rounding_bound` of the long-double
definition on the set's own `sample_images` of that field; the log-likelihood bit for bit `FieldSetContext.loglike`'s
and the oracle's to 1e-9 (tests/test_gpu_fisher.py's tolerance); the same bits whatever the order the fields are
called in (the stash and the partial tiles only grow, and the fields differ in pixel count); and a context that
never calls fisher_rows reports the options of one that did."""
import numpy as np
import pytest

import mode_helpers as mh
import test_gpu_fisher as tgf
from psfmc_amd import mode

pytestmark = pytest.mark.gpu

# (ny, nx, PSF side, mask + weights <= 0 + NaN pixels)
FIELDS = [(62, 66, 21, False), (70, 64, 17, True), (64, 64, 11, False)]
K = 11                           # sky, point source (3), Sersic (7); the PSF index stays at its base value


def _make(f):
    ny, nx, pk, spoil = FIELDS[f]

    def make():
        case = tgf._edge_case((ny, nx), [dict(type='sky', adu=0.004), tgf._ps(nx, ny), tgf._sersic(nx, ny)], n_psf=2,
                              spoil=spoil, psf_side=pk, seed=5200 + f)
        case['theta'] = case['theta'].copy()
        case['theta'][-1] = f % 2
        return case
    return make


@pytest.fixture(scope='module')
def fieldset():
    from psfmc_amd import FieldSet
    refs = [tgf.reference('set-field-%d' % f, _make(f)) for f in range(len(FIELDS))]
    fs = FieldSet([ref['case']['build']('fused', 1) for ref in refs], max_walkers=64)
    yield refs, fs
    fs.close()


def test_set_geometry_and_conditions(fieldset):
    refs, fs = fieldset
    assert fs.context.shapes == [(ny, nx) for ny, nx, _, _ in FIELDS]
    assert len({pk for _, _, pk, _ in FIELDS}) == 3 and all(max(ny, nx) <= 72 for ny, nx, _, _ in FIELDS)
    assert (62 * 66) % 64 != 0
    for f, ref in enumerate(refs):
        case = ref['case']
        assert case['has_psf_index'] and len(ref['columns']) == K == fs.num_params - 1
        assert case['layout'][0] == ('sky',) and ref['columns'][0] == 0
        assert case['theta'][-1] == f % 2
        assert fs.models[f].config.obs_data.shape == FIELDS[f][:2]
    spoilt = refs[1]['case']['field'].bad_px
    assert spoilt.sum() >= 7 * 12 + 4 and not refs[0]['case']['field'].bad_px[-1, -1]


def _fisher(fs, f, refs):
    return fs.models[f].fisher(refs[f]['case']['theta'])


def test_every_field_against_the_oracle_and_its_own_images(fieldset):
    refs, fs = fieldset
    for f, ref in enumerate(refs):
        case, model = ref['case'], fs.models[f]
        out = _fisher(fs, f, refs)
        assert np.array_equal(out['columns'], ref['columns']) and np.array_equal(out['step'], ref['step'][0])
        assert out['F'].shape == (K, K) and np.array_equal(out['F'], out['F'].T)
        err_f, err_g = mh.fisher_errors(out['F'], out['grad'], ref['F'], ref['g'])
        print('field %d: normalised error F %.3g (bound %.3g), g %.3g (bound %.3g)' % (
            f, err_f, ref['bounds'][0], err_g, ref['bounds'][1]))
        assert err_f <= ref['bounds'][0] and err_g <= ref['bounds'][1], f
        vecs = mode.stencil(case['theta'], ref['step'], ref['columns'])[0]
        tgf.held_to_own_images(model, vecs, out, 0.5 / ref['step'][0], 'field %d of the set' % f)
        base = model.derived_rows(case['theta'][None, :])
        assert out['loglike'] == fs.context.loglike(f, base)[0], f
        want_ll = ref['imgs']['ll'][0]
        assert abs(out['loglike'] - want_ll) <= 1e-9 * abs(want_ll), f


def test_the_order_of_the_fields_does_not_matter(fieldset):
    refs, fs = fieldset
    first = {f: _fisher(fs, f, refs) for f in (0, 1, 2)}
    second = {f: _fisher(fs, f, refs) for f in (2, 0, 1)}
    for f in range(3):
        for key in ('F', 'grad', 'loglike'):
            assert np.array_equal(first[f][key], second[f][key]), (f, key)
    assert not np.array_equal(first[0]['F'], first[2]['F'])


def test_a_set_that_never_calls_it_reports_the_same_options(fieldset):
    from psfmc_amd import FieldSet
    refs, fs = fieldset
    _fisher(fs, 1, refs)
    fresh = FieldSet([ref['case']['build']('fused', 1) for ref in refs], max_walkers=64)
    theta = [ref['case']['theta'][None, :] for ref in refs]
    want = fresh.log_posterior_batch(theta)
    for key in tgf.OPTION_KEYS:
        assert fresh.context.get_option(key) == fs.context.get_option(key), key
    got = fs.log_posterior_batch(theta)
    for f in range(3):
        assert np.array_equal(got[f], want[f]), f
    fresh.close()
