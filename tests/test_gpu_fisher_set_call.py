"""psfmc_fisher_rows_fields: stencils of DIFFERENT fields of a set in one call (`FieldSetContext.fisher_rows_fields`,
`FieldSet.fisher`), on the mixed set of tests/test_gpu_fisher_fields.py -- 62 x 66 (PSF side 21; 4092 pixels, not
whole waves of 64), 70 x 64 (17; a mask, weights <= 0 and NaN pixels) and 64 x 64 (11), K = 11.

The contract is bit equality: a stencil's F, g and lnlike are those of `fisher_rows` on it alone, whatever stands
beside it, in whatever field order, wherever a pass boundary falls.  Each field's result is also held, through
`test_gpu_fisher.held_to_own_images`, to the long-double definition on the set's own sample images."""
import numpy as np
import pytest

import test_gpu_fisher as tgf
import test_gpu_fisher_fields as tgff
from psfmc_amd import engine, mode

pytestmark = pytest.mark.gpu

K = tgff.K
N_ST = 2 * K + 1
MAX_WALKERS = 6 * N_ST            # room for the four-stencil call and more


def _build(refs, max_walkers=MAX_WALKERS):
    from psfmc_amd import FieldSet
    return FieldSet([ref['case']['build']('fused', 1) for ref in refs], max_walkers=max_walkers)


def _stencil(fs, refs, f, theta=None):
    """(rows [2K+1, row_len], inv2h [K]) of field f's stencil at theta (default: the case's vector)."""
    ref = refs[f]
    theta = ref['case']['theta'] if theta is None else theta
    vecs = mode.stencil(theta, ref['step'], ref['columns'])[0]
    return fs.models[f].derived_rows(vecs), 0.5 / ref['step'][0]


@pytest.fixture(scope='module')
def fieldset():
    refs = [tgf.reference('set-field-%d' % f, tgff._make(f)) for f in range(len(tgff.FIELDS))]
    fs = _build(refs)
    stencils = [_stencil(fs, refs, f) for f in range(3)]
    alone = [fs.context.fisher_rows(f, rows[None], inv2h[None]) for f, (rows, inv2h) in enumerate(stencils)]
    yield dict(refs=refs, fs=fs, stencils=stencils, alone=alone)
    fs.close()


def _call(fs, stencils, order):
    return fs.context.fisher_rows_fields(order, np.array([stencils[i][0] for i in range(len(order))]),
                                         np.array([stencils[i][1] for i in range(len(order))]))


def _same(got, s, want):
    for key, a, b in zip(('F', 'g', 'lnlike'), got, want):
        assert np.array_equal(a[s], b[0]), key


def test_one_call_is_three_calls_bit_for_bit(fieldset):
    c = fieldset
    assert c['fs'].context.shapes == [(ny, nx) for ny, nx, _, _ in tgff.FIELDS] and 3 * N_ST <= MAX_WALKERS
    got = _call(c['fs'], c['stencils'], [0, 1, 2])
    for f in range(3):
        _same(got, f, c['alone'][f])
        assert np.array_equal(got[0][f], got[0][f].T) and np.all(np.isfinite(got[0][f]))
    assert not np.array_equal(got[0][0], got[0][2])
    again = _call(c['fs'], c['stencils'], [0, 1, 2])                 # a repeated call: the same bits
    for a, b in zip(got, again):
        assert np.array_equal(a, b)


def test_any_field_order_and_two_stencils_of_one_field(fieldset):
    c = fieldset
    fs, refs = c['fs'], c['refs']
    other = refs[0]['case']['theta'].copy()
    other[1] += 0.37                                                # field 0 again, the point source elsewhere
    second = _stencil(fs, refs, 0, other)
    second_alone = fs.context.fisher_rows(0, second[0][None], second[1][None])
    got = _call(fs, [c['stencils'][2], c['stencils'][0], c['stencils'][1], second], [2, 0, 1, 0])
    _same(got, 0, c['alone'][2])
    _same(got, 1, c['alone'][0])
    _same(got, 2, c['alone'][1])
    _same(got, 3, second_alone)
    assert not np.array_equal(got[0][1], got[0][3])


def test_a_pass_boundary_inside_a_stencil_and_between_fields(fieldset):
    c = fieldset
    fs = _build(c['refs'])
    try:
        # passes of 16 walkers: boundaries at 16 and 32 fall inside stencils 0 and 1; passes of 23: on the seam
        # between two fields' stencils
        for size in (16, N_ST):
            fs.context.set_option('chunk_walkers', size)
            assert int(fs.context.get_option('chunk_walkers')) == size
            stencils = [_stencil(fs, c['refs'], f) for f in range(3)]
            got = _call(fs, stencils, [0, 1, 2])
            for f in range(3):
                _same(got, f, c['alone'][f])
    finally:
        fs.close()


def test_each_field_is_held_to_its_own_images(fieldset):
    c = fieldset
    got = _call(c['fs'], c['stencils'], [0, 1, 2])
    for f, ref in enumerate(c['refs']):
        vecs = mode.stencil(ref['case']['theta'], ref['step'], ref['columns'])[0]
        tgf.held_to_own_images(c['fs'].models[f], vecs, dict(F=got[0][f], grad=got[1][f]), 0.5 / ref['step'][0],
                               'field %d in a three-field call' % f)


def test_a_nan_row_spoils_its_own_stencil_only(fieldset):
    c = fieldset
    stencils = [(rows.copy(), inv2h) for rows, inv2h in c['stencils']]
    stencils[1][0][3, 1] = np.nan                                    # the point source's flux in the +h row of column 1
    got = _call(c['fs'], stencils, [0, 1, 2])
    assert not np.all(np.isfinite(got[0][1])) and not np.all(np.isfinite(got[1][1]))
    _same(got, 0, c['alone'][0])
    _same(got, 2, c['alone'][2])
    assert got[2][1] == c['alone'][1][2][0]                          # the base row is untouched: its lnlike stands


def test_fieldset_fisher_returns_these_values(fieldset):
    c = fieldset
    fs, refs = c['fs'], c['refs']
    outs = fs.fisher([ref['case']['theta'] for ref in refs])
    for f, (out, ref) in enumerate(zip(outs, refs)):
        assert np.array_equal(out['columns'], ref['columns']) and np.array_equal(out['step'], ref['step'][0])
        assert out['F'].shape == (K, K)
        assert np.array_equal(out['F'], c['alone'][f][0][0]) and np.array_equal(out['grad'], c['alone'][f][1][0])
        assert out['loglike'] == c['alone'][f][2][0]
        own = fs.models[f].fisher(ref['case']['theta'])
        for key in ('F', 'grad', 'loglike', 'step', 'columns'):
            assert np.array_equal(out[key], own[key]), (f, key)
    # fields left out, several bases of one field, other columns: two groups of K, so two calls
    thetas = [np.vstack([refs[0]['case']['theta']] * 2), None, refs[2]['case']['theta'][None, :]]
    some = fs.fisher(thetas, columns=[None, None, [0, 2, 5]])
    assert some[1] is None and some[0]['F'].shape == (2, K, K) and some[2]['F'].shape == (1, 3, 3)
    assert np.array_equal(some[0]['F'][0], c['alone'][0][0][0]) and np.array_equal(some[0]['F'][1], some[0]['F'][0])
    own = fs.models[2].fisher(thetas[2], columns=[0, 2, 5])
    assert np.array_equal(some[2]['F'], own['F']) and np.array_equal(some[2]['grad'], own['grad'])


def test_refusals(fieldset):
    c = fieldset
    ctx = c['fs'].context
    row_len = c['stencils'][0][0].shape[1]
    refused = (ValueError, engine.NativeError)
    with pytest.raises(refused):                                     # 7 x 23 walkers > 138
        ctx.fisher_rows_fields([0] * 7, np.zeros((7, N_ST, row_len)), np.ones((7, K)))
    with pytest.raises(refused):                                     # K = 64
        ctx.fisher_rows_fields([0], np.zeros((1, 129, row_len)), np.ones((1, 64)))
    with pytest.raises(refused):
        ctx.fisher_rows_fields([3], np.zeros((1, N_ST, row_len)), np.ones((1, K)))
    # the library's own checks, past the Python layer's
    lib, dp = ctx._lib, engine._dp
    fields = np.zeros(7, dtype=np.int32)
    ip = fields.ctypes.data_as(engine.ctypes.POINTER(engine.ctypes.c_int))
    rows, inv2h = np.zeros((7, 129, row_len)), np.ones((7, 64))
    out_f, out_g, out_l = np.zeros((7, 64, 64)), np.zeros((7, 64)), np.zeros(7)
    assert lib.psfmc_fisher_rows_fields(ctx._ctx, 7, K, ip, dp(rows), dp(inv2h), dp(out_f), dp(out_g), dp(out_l)) != 0
    assert lib.psfmc_fisher_rows_fields(ctx._ctx, 1, 64, ip, dp(rows), dp(inv2h), dp(out_f), dp(out_g), dp(out_l)) != 0
    fields[0] = 3
    assert lib.psfmc_fisher_rows_fields(ctx._ctx, 1, K, ip, dp(rows), dp(inv2h), dp(out_f), dp(out_g), dp(out_l)) != 0
    assert lib.psfmc_fisher_rows_fields(ctx._ctx, 0, K, ip, dp(rows), dp(inv2h), dp(out_f), dp(out_g), dp(out_l)) != 0
    got = _call(c['fs'], c['stencils'], [0, 1, 2])                   # and the context still answers
    _same(got, 1, c['alone'][1])


def test_a_set_that_never_calls_it_reports_the_same(fieldset):
    c = fieldset
    _call(c['fs'], c['stencils'], [0, 1, 2])
    fresh = _build(c['refs'])
    theta = [ref['case']['theta'][None, :] for ref in c['refs']]
    want = fresh.log_posterior_batch(theta)
    for key in tgf.OPTION_KEYS:
        assert fresh.context.get_option(key) == c['fs'].context.get_option(key), key
    got = c['fs'].log_posterior_batch(theta)
    for f in range(3):
        assert np.array_equal(got[f], want[f]), f
    fresh.close()
