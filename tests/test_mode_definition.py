"""The posterior-mode definitions of psfmc_amd/mode.py on the CPU, driven by the numpy oracle alone: the Fisher matrix
and gradient from a stencil of images (`fisher_from_stencil`), the Levenberg-Marquardt search (`lm_search`) and the
rule `model_galaxy_mcmc(start='mode')` draws its walkers by (`draw_about_mode`).  The field is
`tools/synth_field.make_field(64, 1, seed=0)`: one point source and one Sersic, K = 10 free columns."""
import numpy as np
import pytest

import mode_helpers as mh
import psfmc_oracle as orc
from psfmc_amd import mode

# Truncation error of the central-difference gradient at h_k = 1e-4 max(|theta_k|, 1), measured at the truth vector
# against central differences of the oracle's log-likelihood at the same steps: 4.6e-4 of max |g| (both are O(h^2)
# estimates of one derivative; they differ in which function is differenced).  The bound is 4 x that.
G_TRUNCATION = 4.6e-4
G_BOUND = 4 * G_TRUNCATION
K = 10


@pytest.fixture(scope='module')
def truth_case():
    fld, field = mh.synth_field_64()
    truth = fld['truth']
    columns = np.arange(len(truth))
    step = mh.scale_steps(truth, columns)
    fisher, grad, imgs = mh.oracle_fisher(field, mh.SYNTH_LAYOUT, truth, step, columns)
    return dict(fld=fld, field=field, truth=truth, columns=columns, step=step, F=fisher, g=grad, imgs=imgs)


def test_stencil_order():
    vecs = mode.stencil([1.0, 2.0, 3.0], [[0.1, 0.2]], [2, 0])
    assert vecs.shape == (1, 5, 3)
    assert np.array_equal(vecs[0], [[1, 2, 3], [1, 2, 3.1], [1, 2, 2.9], [1.2, 2, 3], [0.8, 2, 3]])


def test_fisher_is_symmetric_positive_definite(truth_case):
    fisher = truth_case['F']
    assert fisher.shape == (K, K)
    diag = np.sqrt(np.diag(fisher))
    assert np.max(np.abs(fisher - fisher.T) / np.outer(diag, diag)) <= 1e-13
    assert np.linalg.eigvalsh(0.5 * (fisher + fisher.T)).min() > 0
    np.linalg.cholesky(fisher)


def test_gradient_matches_differences_of_the_likelihood(truth_case):
    c = truth_case
    vecs = mode.stencil(c['truth'], c['step'], c['columns'])[0]
    ll = mh.oracle_loglike(c['field'], mh.SYNTH_LAYOUT, vecs)
    want = (ll[1::2] - ll[2::2]) / (2 * c['step'][0])
    err = np.max(np.abs(c['g'] - want)) / np.max(np.abs(want))
    print('gradient against differences of lnL: %.3g of max |g| (bound %.3g)' % (err, G_BOUND))
    assert err <= G_BOUND
    # the base log-likelihood from the stencil's own images is the oracle's
    got = mode.loglike_from_images(c['imgs']['resid'][0], c['imgs']['ivm'][0], ~c['field'].bad_px)
    assert abs(got - ll[0]) <= 1e-12 * abs(ll[0])


def test_halving_the_step_changes_little(truth_case):
    c = truth_case
    half, _, _ = mh.oracle_fisher(c['field'], mh.SYNTH_LAYOUT, c['truth'], c['step'] / 2, c['columns'])
    diag = np.sqrt(np.diag(c['F']))
    change = np.max(np.abs(half - c['F']) / np.outer(diag, diag))
    print('normalised F, h against h / 2: %.3g (bound %.3g)' % (change, G_BOUND))
    assert change <= G_BOUND


def test_nan_under_a_masked_pixel_changes_nothing(truth_case):
    c = truth_case
    fld = c['fld']
    mask = np.zeros(fld['sci'].shape, dtype=bool)
    mask[20:24, 30:37] = True
    mask[5, 5] = True
    field = orc.make_field(fld['sci'], fld['ivm'], [fld['psf']], [fld['psf_ivm']], mask=mask, mag_zp=fld['mag_zp'])
    assert field.bad_px.sum() == mask.sum()
    fisher, grad, imgs = mh.oracle_fisher(field, mh.SYNTH_LAYOUT, c['truth'], c['step'], c['columns'])
    assert not np.array_equal(fisher, c['F'])                       # the mask counts
    resid = imgs['resid'].copy()
    resid[:, mask] = np.nan                                          # what a NaN sci under the mask gives
    ivm = imgs['ivm'].copy()
    ivm[1:, mask] = np.nan
    again = mode.fisher_from_stencil(resid, ivm, ~field.bad_px, 0.5 / c['step'][0])
    assert np.array_equal(again[0], fisher) and np.array_equal(again[1], grad)
    # a weight that is not finite takes its pixel out like a mask
    ivm2 = imgs['ivm'].copy()
    ivm2[0][mask] = np.inf
    good = np.ones(mask.shape, dtype=bool)
    third = mode.fisher_from_stencil(imgs['resid'], ivm2, good, 0.5 / c['step'][0])
    assert np.array_equal(third[0], fisher) and np.array_equal(third[1], grad)


def test_search_converges_from_thirty_sigma():
    out = mh.cpu_mode_search(max_iter=30)
    res = out['result']
    print('CPU search: %d iterations, lnL %.6f' % (res.iterations, res.lnpost))
    assert res.converged and res.ok and res.iterations <= 30
    assert np.all(np.abs(out['start'] - out['fld']['truth']) >= 29.9 * out['sigma'])
    grad = mh.oracle_fisher(out['field'], mh.SYNTH_LAYOUT, res.theta, mh.scale_steps(res.theta, out['columns']),
                            out['columns'])[1]
    rel = np.max(np.abs(grad) / np.sqrt(np.diag(res.hessian)))
    print('|g_k| / sqrt(F_kk) at the result: %.3g' % rel)
    assert rel < 1e-3
    assert res.lnpost >= mh.oracle_loglike(out['field'], mh.SYNTH_LAYOUT, out['fld']['truth'])[0]
    assert np.isfinite(res.laplace_log_evidence)
    assert np.allclose(np.dot(res.cov, res.hessian), np.eye(K), atol=1e-8)


def test_search_stops_on_the_edge_of_a_support():
    """The likelihood's maximum has reff = 6.20 (as reff_b: the search above is free to swap the axes); inside the box
    of tools/synth_field.py's priors, where reff ends at 6, the maximum sits ON that edge.  With `feasible` the search
    walks the edge column to it and converges there, from the truth and from a start that first runs into it."""
    out = mh.cpu_mode_search(max_iter=30)
    field, columns = out['field'], out['columns']
    free = out['result']
    assert max(free.theta[6], free.theta[7]) > 6.0
    lo = np.array([18, 24.5, 24.5, 0, 0, 19, 2, 2, 24.5, 24.5])
    hi = np.array([20, 40.5, 40.5, 180, np.inf, 24, 6, 6, 40.5, 40.5])
    inside = lambda th: np.all((th >= lo) & (th <= hi), axis=1) & (th[:, 7] <= th[:, 6])
    lnpost = lambda th: np.where(inside(th), mh.oracle_loglike(field, mh.SYNTH_LAYOUT, th), -np.inf)

    def curvature(thetas):
        pairs = [mh.oracle_fisher(field, mh.SYNTH_LAYOUT, t, mh.scale_steps(t, columns), columns)[:2] for t in thetas]
        return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])

    truth = out['fld']['truth']
    far = truth + np.array([0, 0, 0, 0, 0, 0, 0.45, 0, 0, 0])        # reff = 5.95: the first step crosses the edge
    found = mode.lm_search(curvature, lnpost, np.array([truth, far]), columns, max_iter=30, feasible=inside)
    for res in found:
        assert res.converged and res.ok and res.iterations <= 30
        assert 6.0 - 1e-9 <= res.theta[6] <= 6.0 and res.theta[7] < 6.0
        assert truth_ll(field, truth) < res.lnpost < free.lnpost
    assert abs(found[0].lnpost - found[1].lnpost) <= 1e-9 * abs(found[0].lnpost)
    # without `feasible` the same start is left where its steps stop being accepted, short of the edge's value
    stuck = mode.lm_search(curvature, lnpost, far, columns, max_iter=30)[0]
    assert stuck.lnpost <= found[0].lnpost


def truth_ll(field, truth):
    return mh.oracle_loglike(field, mh.SYNTH_LAYOUT, truth)[0]


def test_walkers_drawn_about_the_mode_sit_in_it():
    """64 draws of the start='mode' rule at the mode the CPU search found: conditions, not measurements (the oracle
    alone gives a median deficit of 4.8 and a maximum of 10.2 for K = 10; K / 2 is the expectation)."""
    out = mh.cpu_mode_search(max_iter=30)
    res = out['result']
    walkers = mode.draw_about_mode(res.theta, res.cov, res.columns, 64, np.random.RandomState(5))
    assert walkers.shape == (64, K)
    ll = mh.oracle_loglike(out['field'], mh.SYNTH_LAYOUT, walkers)
    assert np.all(np.isfinite(ll))
    deficit = res.lnpost - ll
    print('deficit below the mode: median %.2f, maximum %.2f' % (np.median(deficit), deficit.max()))
    assert np.median(deficit) <= K
    assert deficit.max() <= 3 * K


def test_draws_outside_the_prior_are_redrawn_then_refused():
    theta, cov = np.array([0.0, 5.0]), np.eye(1)
    inside = lambda th: np.where(th[:, 0] > 0, 0.0, -np.inf)
    got = mode.draw_about_mode(theta, cov, [0], 32, np.random.RandomState(1), log_prior=inside)
    assert np.all(got[:, 0] > 0) and np.all(got[:, 1] == 5.0)
    with pytest.raises(ValueError):
        mode.draw_about_mode(theta, cov, [0], 4, np.random.RandomState(1),
                             log_prior=lambda th: np.full(len(th), -np.inf))
    others = np.tile([9.0, 7.0], (4, 1))
    got = mode.draw_about_mode(theta, cov, [0], 4, np.random.RandomState(1), others=others)
    assert np.all(got[:, 1] == 7.0) and not np.any(got[:, 0] == 9.0)


def test_prior_derivatives():
    log_prior = lambda th: -0.5 * ((th[:, 0] - 1.0) / 2.0) ** 2 + np.where(np.abs(th[:, 1]) < 1, 0.0, -np.inf)
    theta = np.array([[3.0, 0.5], [0.0, 1.0 - 1e-6]])
    first, second = mode.prior_derivatives(log_prior, theta, np.full((2, 2), 1e-3), [0, 1])
    assert np.allclose(first[:, 0], [-0.5, 0.25], rtol=1e-6) and np.allclose(second[:, 0], -0.25, rtol=1e-4)
    assert np.array_equal(first[:, 1], [0.0, 0.0]) and np.array_equal(second[:, 1], [0.0, 0.0])


def test_start_keyword():
    """An unknown `start` raises before anything is built, and the header keys of start='mode' exist only there."""
    from collections import OrderedDict
    import psfmc_amd
    from psfmc_amd import fitting
    assert psfmc_amd.find_mode is mode.find_mode
    with pytest.raises(ValueError, match='start'):
        fitting.model_galaxy_mcmc('no_such_model.py', start='posterior')

    class Chain(object):
        chain = np.zeros((4, 7, 3))
        acceptance_fraction = np.full(4, 0.25)
    prior = fitting._chain_meta(Chain(), 0, 4, False, None, **OrderedDict())
    assert list(prior) == ['MCITER', 'MCBURN', 'MCCHAINS', 'MCCONVRG', 'MCACCEPT']
    found = fitting._chain_meta(Chain(), 0, 4, False, None, **OrderedDict([('MCSTART', 'mode'), ('MCMODELP', -3.5)]))
    assert found['MCSTART'] == 'mode' and found['MCMODELP'] == -3.5
