"""The joint fit's Fisher matrix on the CPU, driven by the numpy oracle alone: `mode.joint_fisher` -- the definition
psfmc_fisher_rows_joint's link kernel is held to -- against `mode.fisher_from_stencil` on the exposures' pixels
concatenated, its gradient against central differences of the oracle's joint log-likelihood, and an oracle-driven
joint `mode.lm_search`.

Two exposures of one scene: the 64 x 64 synthetic field of `mode_helpers.synth_field_64` and a second noise
realisation of it (the oracle's convolved model at the truth plus Gaussian noise of the composite variance, seed 1).
The point source's and the Sersic's positions are fitted per exposure, everything else is shared: K_field = 10,
K_joint = 14, in `JointModel`'s column order."""
import numpy as np
import pytest

import helpers
import mode_helpers as mh
import psfmc_oracle as orc
from psfmc_amd import mode

K_FIELD, K_JOINT = 10, 14
# field f's column k (point source mag, x, y; Sersic angle, index, mag, reff, reff_b, x, y) -> joint column
COL_OF = np.array([[0, 1, 2, 5, 6, 7, 8, 9, 10, 11],
                   [0, 3, 4, 5, 6, 7, 8, 9, 12, 13]])
SHARED = [0, 5, 6, 7, 8, 9]
# Truncation error of the joint central-difference gradient at h_k = 1e-4 max(|theta_k|, 1), measured at the truth
# against central differences of the oracle's joint log-likelihood at the same steps: 4.5e-4 of max |g| (both are
# O(h^2) estimates of one derivative, as in tests/test_mode_definition.py).  The bound is 4 x.
G_TRUNCATION = 4.5e-4
G_BOUND = 4 * G_TRUNCATION
U = 2.0 ** -53


def second_exposure(fld, field):
    """A second noise realisation of a synth field: the oracle's convolved model at the truth plus Gaussian noise of
    the composite variance (seed 1) -> the field's dict with the new science image."""
    comps, psf = helpers.comps_from_theta(mh.SYNTH_LAYOUT, fld['truth'])
    _, imgs = orc.evaluate(field, comps, psf, raw_dtype=np.float64)
    rng = np.random.RandomState(1)
    sci = imgs['convolved_model'] + rng.normal(size=imgs['convolved_model'].shape) / np.sqrt(imgs['composite_ivm'])
    return dict(fld, sci=sci.astype(np.float32))


def two_exposures():
    """(oracle fields [2], joint truth [14], the exposures' synth field dicts [2])."""
    fld, field0 = mh.synth_field_64()
    fld1 = second_exposure(fld, field0)
    field1 = orc.make_field(fld1['sci'], fld['ivm'], [fld['psf']], [fld['psf_ivm']], mag_zp=fld['mag_zp'])
    truth = np.zeros(K_JOINT)
    truth[COL_OF[0]] = fld['truth']
    truth[COL_OF[1]] = fld['truth']
    return [field0, field1], truth, [fld, fld1]


def joint_steps(theta):
    return mode.STEP_FRACTION * np.maximum(np.abs(np.atleast_2d(theta)), 1.0)


def field_stencils(fields, theta, step):
    """Per exposure (F_f, g_f, images of its own 21-vector stencil) at the joint vector theta, joint steps `step`."""
    own = np.arange(K_FIELD)
    return [mh.oracle_fisher(field, mh.SYNTH_LAYOUT, theta[COL_OF[f]], step[COL_OF[f]][None, :], own)
            for f, field in enumerate(fields)]


def oracle_joint(fields, theta, step):
    parts = field_stencils(fields, theta, step)
    return mode.joint_fisher([p[0] for p in parts], [p[1] for p in parts], COL_OF, K_JOINT) + (parts,)


def joint_loglike(fields, thetas):
    thetas = np.atleast_2d(thetas)
    return sum(mh.oracle_loglike(field, mh.SYNTH_LAYOUT, thetas[:, COL_OF[f]]) for f, field in enumerate(fields))


@pytest.fixture(scope='module')
def case():
    fields, truth, _ = two_exposures()
    step = joint_steps(truth)[0]
    fisher, grad, parts = oracle_joint(fields, truth, step)
    return dict(fields=fields, truth=truth, step=step, F=fisher, g=grad, parts=parts)


def test_joint_fisher_adds_in_field_order_from_zero():
    rng = np.random.RandomState(3)
    f_list = [rng.normal(size=(2, 3, 3)) for _ in range(3)]
    g_list = [rng.normal(size=(2, 3)) for _ in range(3)]
    col_of = [[0, 1, 4], [0, 2, 4], [4, 3, 0]]
    fisher, grad = mode.joint_fisher(f_list, g_list, col_of, 6)
    assert fisher.shape == (2, 6, 6) and grad.shape == (2, 6)
    assert np.array_equal(fisher[:, 0, 0], ((0.0 + f_list[0][:, 0, 0]) + f_list[1][:, 0, 0]) + f_list[2][:, 2, 2])
    assert np.array_equal(fisher[:, 0, 4], ((0.0 + f_list[0][:, 0, 2]) + f_list[1][:, 0, 2]) + f_list[2][:, 2, 0])
    assert np.array_equal(grad[:, 4], ((0.0 + g_list[0][:, 2]) + g_list[1][:, 2]) + g_list[2][:, 0])
    assert np.array_equal(fisher[:, 1, 1], f_list[0][:, 1, 1]) and np.array_equal(fisher[:, 3, 0], f_list[2][:, 1, 2])
    assert np.all(fisher[:, 1, 2] == 0) and np.all(fisher[:, 1, 3] == 0) and np.all(fisher[:, 2, 3] == 0)
    assert np.all(fisher[:, 5] == 0) and np.all(fisher[:, :, 5] == 0) and np.all(grad[:, 5] == 0)   # nobody's column
    one_f, one_g = mode.joint_fisher(f_list[:1], g_list[:1], [[0, 1, 2]], 3)
    assert np.array_equal(one_f, f_list[0]) and np.array_equal(one_g, g_list[0])
    for bad in ([[0, 1, 1]], [[0, 1, 6]], [[-1, 1, 2]]):
        with pytest.raises(ValueError):
            mode.joint_fisher(f_list[:1], g_list[:1], bad, 6)


def test_joint_fisher_is_the_definition_on_the_concatenated_pixels(case):
    """`fisher_from_stencil` of ONE 29-vector stencil whose images are the two exposures' side by side, a column an
    exposure does not read having its base images on both sides (a zero derivative image).  Both sum the same
    n = 2 n_good products per element in different orders: they agree within 2 n u sum |term|."""
    fields, parts = case['fields'], case['parts']
    resid, ivm, good = [], [], []
    for f, (_, _, imgs) in enumerate(parts):
        pick = np.zeros(2 * K_JOINT + 1, dtype=np.int64)                   # the exposure's own vector behind each joint one
        for k, j in enumerate(COL_OF[f]):
            pick[1 + 2 * j], pick[2 + 2 * j] = 1 + 2 * k, 2 + 2 * k
        resid.append(imgs['resid'][pick].reshape(len(pick), -1))
        ivm.append(imgs['ivm'][pick].reshape(len(pick), -1))
        good.append(~fields[f].bad_px.ravel())
    resid, ivm, good = np.concatenate(resid, axis=1), np.concatenate(ivm, axis=1), np.concatenate(good)
    inv2h = 0.5 / case['step']
    want_f, want_g = mode.fisher_from_stencil(resid, ivm, good, inv2h)
    keep = good & np.isfinite(ivm[0])
    r, w = resid[0][keep], ivm[0][keep]
    dmu = -(resid[1::2][:, keep] - resid[2::2][:, keep]) * inv2h[:, None]
    dv = (1.0 / ivm[1::2][:, keep] - 1.0 / ivm[2::2][:, keep]) * inv2h[:, None]
    n_terms = 2 * int(keep.sum())
    bound_f = 2 * n_terms * U * (np.dot(np.abs(dmu) * w, np.abs(dmu).T) + 0.5 * np.dot(np.abs(dv) * w * w, np.abs(dv).T))
    bound_g = 2 * n_terms * U * (np.dot(np.abs(dmu), np.abs(r * w)) + 0.5 * np.dot(np.abs(dv), np.abs(r * r * w * w - w)))
    err_f, err_g = np.abs(case['F'] - want_f), np.abs(case['g'] - want_g)
    print('joint_fisher against the concatenated definition: largest |dF| / bound %.3g, |dg| / bound %.3g' % (
        np.max(err_f[bound_f > 0] / bound_f[bound_f > 0]), np.max(err_g / bound_g)))
    assert np.all(err_f <= bound_f) and np.all(err_g <= bound_g)
    # blocks of columns that belong to different exposures: exactly zero on both sides
    for a, b in ((1, 3), (2, 4), (10, 12), (11, 13), (1, 12)):
        assert case['F'][a, b] == 0.0 and want_f[a, b] == 0.0


def test_joint_gradient_matches_differences_of_the_joint_likelihood(case):
    vecs = mode.stencil(case['truth'], case['step'], np.arange(K_JOINT))[0]
    ll = joint_loglike(case['fields'], vecs)
    want = (ll[1::2] - ll[2::2]) / (2 * case['step'])
    err = np.max(np.abs(case['g'] - want)) / np.max(np.abs(want))
    print('joint gradient against differences of the joint lnL: %.3g of max |g| (bound %.3g)' % (err, G_BOUND))
    assert err <= G_BOUND


def test_joint_search_converges_and_tightens_the_shared_columns(case):
    fields, truth = case['fields'], case['truth']
    columns = np.arange(K_JOINT)
    sigma = np.sqrt(np.diag(np.linalg.inv(case['F'])))
    start = truth + 30.0 * sigma * np.where(np.arange(K_JOINT) % 2, -1.0, 1.0)

    def curvature(thetas):
        pairs = [oracle_joint(fields, t, joint_steps(t)[0])[:2] for t in thetas]
        return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])

    res = mode.lm_search(curvature, lambda th: joint_loglike(fields, th), start, columns, max_iter=30)[0]
    print('joint search from 30 sigma off: %r, %d iterations' % (res, res.iterations))
    assert res.converged and res.ok
    assert res.lnpost >= joint_loglike(fields, truth)[0]
    for f, (fisher_f, _, _) in enumerate(field_stencils(fields, res.theta, joint_steps(res.theta)[0])):
        single = np.diag(np.linalg.inv(fisher_f))
        for j in SHARED:
            k = int(np.flatnonzero(COL_OF[f] == j)[0])
            assert res.cov[j, j] < single[k], (f, j)
