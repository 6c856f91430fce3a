"""psfmc_fisher_rows_joint: the Fisher matrix and gradient of a joint fit (`JointModel.fisher`,
`FieldSetContext.fisher_rows_joint`) against the definition `mode.joint_fisher` of the fields' own
psfmc_fisher_rows results -- bit for bit -- and against the long-double definition on the fields' own sample images.

First case: the three fields of tests/test_gpu_fisher_fields.py (62 x 66, 70 x 64 spoilt, 64 x 64; PSF sides 21, 17,
11) as ONE model with the sky level and the two positions fitted per field and the rest shared: K_field = 11,
K_joint = 21.  Second case: sky + point source + three Sersics with every parameter per field on three 64 x 64
fields, K_field = 25 and K_joint = 75 -- more columns than the matrix-unit kernel holds in one stencil."""
import numpy as np
import pytest

import mode_helpers as mh
import test_gpu_fisher as tgf
import test_gpu_fisher_fields as tgff
from psfmc_amd import engine, mode

pytestmark = pytest.mark.gpu

K_FIELD, K_JOINT = 11, 21


def _field_parts(joint, theta, columns, step):
    """Per field: (own differentiated columns, their joint places among `columns`, own vector, own steps)."""
    place = np.full(joint.num_params, -1, dtype=np.int64)
    place[columns] = np.arange(len(columns))
    parts = []
    for f in range(len(joint.field_models)):
        jc = joint.field_columns(f)
        own = np.flatnonzero(place[jc] >= 0)
        col_of = place[jc[own]]
        parts.append((own, col_of, theta[jc], step[col_of]))
    return parts


def _alone(joint, parts):
    """Each field's stencil through psfmc_fisher_rows on its own: [(F, g, lnlike)]."""
    out = []
    for m, (own, _, th, h) in zip(joint.field_models, parts):
        vecs = mode.stencil(th, h[None, :], own)[0]
        fisher, grad, ll = m.engine.fisher_rows(m.derived_rows(vecs)[None], (0.5 / h)[None])
        out.append((fisher[0], grad[0], ll[0]))
    return out


@pytest.fixture(scope='module')
def linked():
    from psfmc_amd import JointModel
    refs = [tgf.reference('set-field-%d' % f, tgff._make(f)) for f in range(3)]
    models = [ref['case']['build']('fused', 1) for ref in refs]
    per_field = [n for n in models[0].param_names if n.endswith('_xy') or 'Sky' in n]
    joint = JointModel(models, per_field=per_field, max_walkers=2 * 3 * (2 * K_FIELD + 1))
    theta = np.zeros(joint.num_params)
    for f, ref in enumerate(refs):
        theta[joint.field_columns(f)] = ref['case']['theta']
    columns = mode.default_columns(joint)
    step = mode.default_steps(joint, theta, columns)[0]
    out = joint.fisher(theta)
    parts = _field_parts(joint, theta, columns, step)
    yield dict(refs=refs, joint=joint, theta=theta, columns=columns, step=step, out=out, parts=parts,
               alone=_alone(joint, parts))
    joint.close()


def test_joint_fisher_is_the_link_of_the_fields_results(linked):
    c = linked
    out, joint = c['out'], c['joint']
    assert joint.num_params == K_JOINT + 3 and len(c['columns']) == K_JOINT
    assert all(len(p[0]) == K_FIELD for p in c['parts'])
    assert np.array_equal(out['columns'], c['columns']) and np.array_equal(out['step'], c['step'])
    want_f, want_g = mode.joint_fisher([a[0] for a in c['alone']], [a[1] for a in c['alone']],
                                       [p[1] for p in c['parts']], K_JOINT)
    assert out['F'].shape == (K_JOINT, K_JOINT) and np.all(np.isfinite(out['F']))
    assert np.array_equal(out['grad'], want_g)
    assert np.array_equal(out['F'], want_f)
    assert np.array_equal(out['F'], out['F'].T)
    # a column of one field against a column of another: nothing reads both
    sky = [int(p[1][0]) for p in c['parts']]
    assert out['F'][sky[0], sky[1]] == 0.0 and out['F'][sky[1], sky[2]] == 0.0
    # the entry's own lnlike: the fields' row-based log-likelihoods summed in field order
    rows = np.stack([m.derived_rows(mode.stencil(th, h[None, :], own)[0])
                     for m, (own, _, th, h) in zip(joint.field_models, c['parts'])])[None]
    inv2h = np.stack([0.5 / p[3] for p in c['parts']])[None]
    got_f, got_g, got_ll = joint.context.fisher_rows_joint(np.array([p[1] for p in c['parts']]), rows, inv2h, K_JOINT)
    assert np.array_equal(got_f[0], out['F']) and np.array_equal(got_g[0], out['grad'])
    assert got_ll[0] == (c['alone'][0][2] + c['alone'][1][2]) + c['alone'][2][2]
    # ... which the raw-vector path's lnL matches to rounding, not in its bits: the rows are the host's
    assert abs(got_ll[0] - out['loglike']) <= 1e-11 * abs(out['loglike'])


def test_joint_loglike_is_the_joint_posteriors_likelihood_term(linked):
    """`JointModel.fisher`'s `loglike` is `log_likelihood_and_prior_batch`'s lnL, bit for bit: the model evaluates the
    base vectors once more from raw vectors, as the samplers do.  (The C entry's own lnlike, from host-derived rows,
    measured -169648.7607040153 against -169648.7607039787 here: 2.2e-13 relative.  DESIGN.md section 31.)"""
    c = linked
    want = c['joint'].log_likelihood_and_prior_batch(c['theta'])[0][0]
    print('joint loglike %.17g against log_likelihood_and_prior_batch: %.17g' % (c['out']['loglike'], want))
    assert np.isfinite(want)
    assert c['out']['loglike'] == want
    two = np.vstack([c['theta'], c['theta']])
    two[1, c['columns'][5]] += 0.21
    assert np.array_equal(c['joint'].fisher(two)['loglike'], c['joint'].log_likelihood_and_prior_batch(two)[0])


def test_joint_fisher_against_the_long_double_definition(linked):
    """The fields' rounding bounds (`mode_helpers.fisher_rounding_bound`, made absolute with the reference's diagonal
    and scattered to the joint columns) added, plus (n_fields - 1) u sum_f |F_f| for the link's additions, against the
    fields' long-double references summed in long double."""
    c = linked
    ld = np.longdouble
    ref_f, ref_g = np.zeros((K_JOINT, K_JOINT), dtype=ld), np.zeros(K_JOINT, dtype=ld)
    bound_f, bound_g = np.zeros((K_JOINT, K_JOINT)), np.zeros(K_JOINT)
    link_f, link_g = np.zeros((K_JOINT, K_JOINT)), np.zeros(K_JOINT)
    for m, (own, col_of, th, h), alone in zip(c['joint'].field_models, c['parts'], c['alone']):
        vecs = mode.stencil(th, h[None, :], own)[0]
        dev = m.sample_images(vecs, ('convolved_model', 'composite_ivm'))
        args = (dev['convolved_model'], dev['composite_ivm'], np.asarray(m.config.obs_data, dtype=np.float64),
                ~np.asarray(m.config.bad_px, dtype=bool), 0.5 / h)
        want_f, want_g = mh.fisher_reference_longdouble(*args)
        norm_f, norm_g = mh.fisher_rounding_bound(*args)
        diag = np.sqrt(np.diag(want_f).astype(np.float64))
        ix = np.ix_(col_of, col_of)
        ref_f[ix] += want_f
        ref_g[col_of] += want_g
        bound_f[ix] += norm_f * np.outer(diag, diag)
        bound_g[col_of] += norm_g * diag
        link_f[ix] += np.abs(alone[0])
        link_g[col_of] += np.abs(alone[1])
    n_f = len(c['parts'])
    bound_f += (n_f - 1) * mh.U64 * link_f
    bound_g += (n_f - 1) * mh.U64 * link_g
    err_f = np.abs(c['out']['F'] - ref_f).astype(np.float64)
    err_g = np.abs(c['out']['grad'] - ref_g).astype(np.float64)
    read = bound_f > 0
    print('joint F against the long-double references: largest error / bound %.3g; g %.3g' % (
        np.max(err_f[read] / bound_f[read]), np.max(err_g / bound_g)))
    assert np.all(err_f <= bound_f) and np.all(err_g <= bound_g)
    assert np.all(c['out']['F'][~read] == 0.0)


def test_two_bases_in_one_call_equal_each_alone(linked):
    c = linked
    other = c['theta'].copy()
    other[c['columns'][5]] += 0.21
    both = c['joint'].fisher(np.vstack([c['theta'], other]))
    alone = c['joint'].fisher(other)
    for key in ('F', 'grad', 'loglike'):
        assert np.array_equal(both[key][0], c['out'][key]), key
        assert np.array_equal(both[key][1], alone[key]), key
    assert not np.array_equal(both['F'][0], both['F'][1])


def test_one_field_joint_is_that_fields_fisher_rows(linked):
    from psfmc_amd import JointModel
    ref = linked['refs'][1]
    one = JointModel([ref['case']['build']('fused', 1)], max_walkers=2 * K_FIELD + 1)
    try:
        theta = ref['case']['theta']
        out = one.fisher(theta)
        assert np.array_equal(out['columns'], ref['columns']) and np.array_equal(out['step'], ref['step'][0])
        m = one.field_models[0]
        vecs = mode.stencil(theta, ref['step'], ref['columns'])[0]
        fisher, grad, ll = m.engine.fisher_rows(m.derived_rows(vecs)[None], 0.5 / ref['step'])
        assert np.array_equal(out['F'], fisher[0]) and np.array_equal(out['grad'], grad[0])
        got = one.context.fisher_rows_joint(np.arange(K_FIELD)[None], m.derived_rows(vecs)[None, None],
                                            0.5 / ref['step'][None], K_FIELD)
        assert np.array_equal(got[0][0], fisher[0]) and np.array_equal(got[1][0], grad[0]) and got[2][0] == ll[0]
        assert out['loglike'] == one.log_likelihood_and_prior_batch(theta)[0][0]
    finally:
        one.close()


def test_more_joint_columns_than_one_stencil_holds():
    from psfmc_amd import JointModel
    comps = [dict(type='sky', adu=0.004), tgf._ps(64, 64)] + [tgf._sersic(64, 64, k) for k in range(3)]
    cases = [tgf._edge_case((64, 64), comps, seed=6100 + f) for f in range(3)]
    models = [case['build']('fused', 1) for case in cases]
    joint = JointModel(models, per_field=models[0].param_names, max_walkers=3 * 51)
    try:
        assert joint.num_params == 75 > engine.FISHER_MAX_COLUMNS and models[0].num_params == 25
        theta = np.zeros(75)
        for f, case in enumerate(cases):
            theta[joint.field_columns(f)] = case['theta']
        out = joint.fisher(theta)
        assert out['F'].shape == (75, 75) and np.all(np.isfinite(out['F'])) and np.all(np.isfinite(out['grad']))
        assert np.array_equal(out['F'], out['F'].T)
        for f in range(3):
            cols = joint.field_columns(f)
            own = joint.field_models[f].fisher(cases[f]['theta'])
            assert np.array_equal(own['step'], out['step'][cols])
            assert np.array_equal(out['F'][np.ix_(cols, cols)], own['F']), f
            assert np.array_equal(out['grad'][cols], own['grad']), f
            for g in range(f + 1, 3):
                assert np.all(out['F'][np.ix_(cols, joint.field_columns(g))] == 0.0)
    finally:
        joint.close()


def test_joint_refusals(linked):
    c = linked
    ctx = c['joint'].context
    row_len = ctx._lib.psfmc_row_len(ctx._ctx)
    n_st = 2 * K_FIELD + 1
    col_of = np.array([p[1] for p in c['parts']])
    rows, inv2h = np.zeros((1, 3, n_st, row_len)), np.ones((1, 3, K_FIELD))
    twice = col_of.copy()
    twice[1, 4] = twice[1, 3]
    with pytest.raises(engine.NativeError, match='injective'):
        ctx.fisher_rows_joint(twice, rows, inv2h, K_JOINT)
    past = col_of.copy()
    past[2, 0] = K_JOINT
    with pytest.raises(engine.NativeError, match='outside'):
        ctx.fisher_rows_joint(past, rows, inv2h, K_JOINT)
    with pytest.raises((ValueError, engine.NativeError)):           # 3 bases x 3 fields x 23 walkers > 138
        ctx.fisher_rows_joint(col_of, np.zeros((3, 3, n_st, row_len)), np.ones((3, 3, K_FIELD)), K_JOINT)
    lib, dp = ctx._lib, engine._dp
    ip = np.ascontiguousarray(col_of, dtype=np.int32)
    big_rows, big_h = np.zeros((3, 3, n_st, row_len)), np.ones((3, 3, K_FIELD))
    out_f, out_g, out_l = np.zeros((3, K_JOINT, K_JOINT)), np.zeros((3, K_JOINT)), np.zeros(3)
    assert lib.psfmc_fisher_rows_joint(ctx._ctx, 3, K_JOINT, K_FIELD, ip.ctypes.data_as(
        engine.ctypes.POINTER(engine.ctypes.c_int)), dp(big_rows), dp(big_h), dp(out_f), dp(out_g), dp(out_l)) != 0
    again = c['joint'].fisher(c['theta'])                            # and the context still answers
    assert np.array_equal(again['F'], c['out']['F'])
