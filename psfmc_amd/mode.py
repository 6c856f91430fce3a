"""The posterior mode: Fisher matrix and gradient of the Gaussian log-likelihood from a central-difference stencil
of images, and a Levenberg-Marquardt search on the log-posterior built on them.

The definition and the search take images or callables, not a model, so that they run on the CPU against the numpy
oracle; `find_mode` drives them with a `MultiComponentModel`, whose `fisher` evaluates the same sums on the device
(psfmc_fisher_rows).

The likelihood (models.py:233-236) is  lnL = -1/2 sum_good [ r^2 w - ln(w / 2 pi) ],  r = sci - conv,
w = 1 / (model_var + obs_var): a Gaussian whose mean AND variance depend on the parameters, so its Fisher
information has a mean term and a variance term, and so has its gradient."""
from __future__ import division

import numpy as np

STEP_FRACTION = 1e-4             # default step: this fraction of the prior's standard deviation (or of max(|theta|, 1))
CONVERGED_SIGMA = 1e-2           # the search stops when no column moves by more than this many sigma
MAX_REDRAWS = 100                # `draw_about_mode`: tries per walker


def stencil(theta, step, columns):
    """The 2K+1 vectors per base of a central-difference stencil: theta [n, P], step [n, K], columns [K] ->
    [n, 2K+1, P]; vector 0 is the base, 1 + 2k and 2 + 2k are theta + h_k e_k and theta - h_k e_k."""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    step = np.broadcast_to(np.asarray(step, dtype=np.float64), (theta.shape[0], len(columns)))
    out = np.repeat(theta[:, None, :], 2 * len(columns) + 1, axis=1)
    for k, col in enumerate(columns):
        out[:, 1 + 2 * k, col] += step[:, k]
        out[:, 2 + 2 * k, col] -= step[:, k]
    return out


def fisher_from_stencil(resid, ivm, good, inv2h):
    """Fisher matrix and gradient of lnL from the images of one stencil.

    resid, ivm  [2K+1, ...] residual and composite weight images of the stencil's vectors (`stencil`'s order)
    good        [...] the pixels the likelihood counts (not in bad_px); pixels whose base weight is not finite
                are left out as well
    inv2h       [K] 1 / (2 h_k)

    With v = 1 / w, and w, r of the base:
        dmu_k = -(r[1+2k] - r[2+2k]) inv2h_k          dv_k = (v[1+2k] - v[2+2k]) inv2h_k
        F_kl  = sum_good w dmu_k dmu_l + 1/2 sum_good w^2 dv_k dv_l
        g_k   = sum_good r w dmu_k     + 1/2 sum_good (r^2 w^2 - w) dv_k
    -> (F [K, K], g [K]): the exact Fisher information and d lnL / d theta of a Gaussian whose mean and variance both
    depend on theta, with the derivatives as central differences."""
    inv2h = np.asarray(inv2h, dtype=np.float64)
    n_st = 2 * len(inv2h) + 1
    resid = np.asarray(resid, dtype=np.float64).reshape(n_st, -1)
    ivm = np.asarray(ivm, dtype=np.float64).reshape(n_st, -1)
    good = np.asarray(good, dtype=bool).ravel() & np.isfinite(ivm[0])
    r_all, w_all = resid[:, good], ivm[:, good]
    with np.errstate(all='ignore'):
        v_all = 1.0 / w_all
        r, w = r_all[0], w_all[0]
        dmu = -(r_all[1::2] - r_all[2::2]) * inv2h[:, None]
        dv = (v_all[1::2] - v_all[2::2]) * inv2h[:, None]
        fisher = np.dot(dmu * w, dmu.T) + 0.5 * np.dot(dv * (w * w), dv.T)
        grad = np.dot(dmu, r * w) + 0.5 * np.dot(dv, r * r * w * w - w)
    return fisher, grad


def joint_fisher(f_list, g_list, col_of, k_joint):
    """Fisher matrix and gradient of a JOINT fit -- the log-likelihood is the fields' sum -- from the fields' own: the
    definition psfmc_fisher_rows_joint's link kernel is held to.

    f_list, g_list  per field F_f [..., K_f, K_f] and g_f [..., K_f] over that field's differentiated columns
    col_of          per field [K_f] the joint column of each of them (injective, in [0, k_joint))
    Element (r, c) starts at +0.0 and adds, for f = 0, 1, ... in that order, F_f[kr, kc] with col_of[f][kr] = r and
    col_of[f][kc] = c; a field that does not read both columns adds nothing.  A joint column no field reads is a zero
    row and column.  -> (F [..., k_joint, k_joint], g [..., k_joint])."""
    lead = np.shape(g_list[0])[:-1]
    fisher, grad = np.zeros(lead + (k_joint, k_joint)), np.zeros(lead + (k_joint,))
    for f_f, g_f, cols in zip(f_list, g_list, col_of):
        cols = np.asarray(cols, dtype=np.int64)
        if len(set(cols.tolist())) != len(cols) or (len(cols) and (cols.min() < 0 or cols.max() >= k_joint)):
            raise ValueError('col_of must be injective per field with values in [0, {})'.format(k_joint))
        fisher[..., cols[:, None], cols[None, :]] += np.asarray(f_f, dtype=np.float64)
        grad[..., cols] += np.asarray(g_f, dtype=np.float64)
    return fisher, grad


def loglike_from_images(resid, ivm, good):
    """lnL of one vector's residual and weight images over the good pixels (NaN / inf preserved)."""
    good = np.asarray(good, dtype=bool)
    r, w = np.asarray(resid)[good], np.asarray(ivm)[good]
    with np.errstate(all='ignore'):
        return -0.5 * np.sum(r * r * w - np.log(0.5 / np.pi * w))


# ---------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------
class ModeResult(object):
    """What a mode search found.

    theta       [P] the mode
    lnpost      its log-posterior
    columns     [K] the differentiated columns (the others stayed at their start values)
    cov         [K, K] H^-1 over `columns`, H = F + diag(-d^2 ln prior / d theta^2) at the mode; None, with
                ok = False, where H is not positive definite
    iterations  iterations the search ran;  converged: whether its last step was below 1e-2 sigma in every column
    laplace_log_evidence   lnpost + K/2 ln 2 pi - 1/2 ln det H: the Laplace approximation to the evidence over the
                differentiated columns.  It is an approximation to set beside `model_galaxy_ptmcmc`'s thermodynamic
                integral, NOT a replacement for it: it assumes one Gaussian mode inside the prior's support."""

    def __init__(self, theta, lnpost, columns, hessian, iterations, converged):
        self.theta = np.array(theta, dtype=np.float64)
        self.lnpost = float(lnpost)
        self.columns = np.array(columns, dtype=np.int64)
        self.iterations, self.converged = int(iterations), bool(converged)
        self.hessian = None if hessian is None else np.array(hessian, dtype=np.float64)
        self.cov, self.ok, self.laplace_log_evidence = None, False, float('nan')
        chol = _cholesky(self.hessian)
        if chol is not None:
            inv_l = np.linalg.solve(chol, np.eye(len(chol)))
            self.cov = np.dot(inv_l.T, inv_l)
            self.ok = True
            k = len(self.columns)
            self.laplace_log_evidence = (self.lnpost + 0.5 * k * np.log(2 * np.pi)
                                         - float(np.sum(np.log(np.diag(chol)))))

    def __repr__(self):
        return 'ModeResult(lnpost={!r}, iterations={}, converged={}, ok={})'.format(
            self.lnpost, self.iterations, self.converged, self.ok)


def _cholesky(matrix):
    """The lower Cholesky factor of a finite, positive definite matrix, else None."""
    if matrix is None or not np.all(np.isfinite(matrix)):
        return None
    try:
        return np.linalg.cholesky(matrix)
    except np.linalg.LinAlgError:
        return None


def _damped_step(hess, grad, lam, free):
    """The step over the `free` columns of (H + lambda diag H) delta = grad, zeros elsewhere, and the largest
    |delta_k| / sigma_k over them (sigma from the inverse of H's free block; inf where that block is not positive
    definite); None where the damped block is not positive definite either."""
    delta = np.zeros(len(grad))
    if not free.any():
        return delta, 0.0
    h_f, g_f = hess[np.ix_(free, free)], grad[free]
    chol = _cholesky(h_f + lam * np.diag(np.diag(h_f))) if np.all(np.isfinite(g_f)) else None
    if chol is None:
        return None, np.inf
    delta[free] = np.linalg.solve(chol.T, np.linalg.solve(chol, g_f))
    plain = _cholesky(h_f)
    if plain is None:
        return delta, np.inf
    inv_l = np.linalg.solve(plain, np.eye(len(g_f)))
    return delta, float(np.max(np.abs(delta[free]) / np.sqrt(np.sum(inv_l * inv_l, axis=0))))


def _to_the_edge(feasible, theta, columns, delta):
    """Which columns' own steps leave the support (`feasible` false for theta + delta_k e_k), and for those the
    largest fraction of the step that stays inside, by bisection: -> (blocked [K] bool, fraction [K])."""
    k = len(columns)
    single = np.tile(theta, (k, 1))
    single[np.arange(k), columns] += delta
    blocked = ~np.asarray(feasible(single), dtype=bool)
    lo, hi = np.zeros(k), np.ones(k)
    which = np.flatnonzero(blocked)
    for _ in range(40 if len(which) else 0):          # to 1e-12 of the step
        mid = 0.5 * (lo + hi)
        probe = np.tile(theta, (len(which), 1))
        probe[np.arange(len(which)), columns[which]] += mid[which] * delta[which]
        ok = np.asarray(feasible(probe), dtype=bool)
        lo[which] = np.where(ok, mid[which], lo[which])
        hi[which] = np.where(ok, hi[which], mid[which])
    return blocked, lo


def lm_search(curvature, lnpost, starts, columns, max_iter=50, lam0=1e-3, feasible=None):
    """Levenberg-Marquardt ascent of a log-posterior from several starts side by side.

    curvature(thetas [m, P]) -> (H [m, K, K], grad [m, K]): curvature (Fisher matrix plus the priors' negative second
                derivatives) and gradient of the log-posterior over `columns`
    lnpost(thetas [m, P])    -> [m] log-posteriors; -inf or NaN (outside a support) is a rejected step
    starts [n, P]
    feasible(thetas [m, P])  -> [m] bool, optional and cheap (the priors alone): is the vector inside the support?

    Every iteration makes one `curvature` call (for the starts that moved) and one `lnpost` call for all starts that
    still run.  A step solves (H + lambda diag H) delta = grad; it is accepted when the log-posterior rises, and then
    lambda shrinks tenfold; otherwise lambda grows tenfold.  With `feasible`, a step that leaves the support is bent
    before it is tried: the columns whose own step leaves it go as far as the edge (bisection on `feasible`), the
    others take the step of the system without them -- a mode ON the edge of a prior's support is then a point the
    search can reach and stop at.  A start stops when a step taken with lambda <= 1 is below 1e-2 sigma in every
    column (sigma from H^-1 over the columns that are free to move).
    Returns a list of `ModeResult`, one per start."""
    steps = _lm_steps(starts, columns, max_iter, lam0, feasible)
    try:
        kind, thetas = next(steps)
        while True:
            if kind == 'curvature':
                answer = curvature(thetas)
            else:
                with np.errstate(all='ignore'):
                    answer = lnpost(thetas)
            kind, thetas = steps.send(answer)
    except StopIteration as done:
        return done.value


def _lm_steps(starts, columns, max_iter, lam0, feasible):
    """`lm_search` as a generator, so that several searches can advance side by side with their device calls shared
    (`find_modes`): it yields ('lnpost', thetas [m, P]) or ('curvature', thetas [m, P]), is sent what `lm_search`'s
    callable of that name returns for them, and returns the list of `ModeResult`.  Per iteration at most one
    'curvature' request, then one 'lnpost' request."""
    starts = np.atleast_2d(np.asarray(starts, dtype=np.float64))
    columns = np.asarray(columns, dtype=np.int64)
    n, k = starts.shape[0], len(columns)
    cur = starts.copy()
    f_cur = np.asarray((yield 'lnpost', cur), dtype=np.float64).copy()
    f_cur[~np.isfinite(f_cur)] = -np.inf
    hess, grad = np.full((n, k, k), np.nan), np.full((n, k), np.nan)
    stale = np.ones(n, dtype=bool)                   # H, grad are not those of `cur`
    lam = np.full(n, float(lam0))
    running = np.isfinite(f_cur)
    converged = np.zeros(n, dtype=bool)
    iters = np.zeros(n, dtype=np.int64)
    everything = np.ones(k, dtype=bool)
    for _ in range(max_iter):
        if not running.any():
            break
        need = np.flatnonzero(running & stale)
        if len(need):
            h_new, g_new = yield 'curvature', cur[need]
            hess[need], grad[need] = h_new, g_new
            stale[need] = False
        idx = np.flatnonzero(running)
        trial = cur[idx].copy()
        small = np.zeros(len(idx), dtype=bool)
        solved = np.zeros(len(idx), dtype=bool)
        for j, i in enumerate(idx):
            delta, size = _damped_step(hess[i], grad[i], lam[i], everything)
            if delta is None:
                continue
            step = cur[i].copy()
            step[columns] += delta
            if feasible is not None and not np.all(feasible(step[None, :])):
                blocked, part = _to_the_edge(feasible, cur[i], columns, delta)
                if blocked.any():
                    inner, size = _damped_step(hess[i], grad[i], lam[i], ~blocked)
                    if inner is None:
                        continue
                    edge = np.where(blocked, part * delta, 0.0)
                    delta = inner + edge
                    with np.errstate(all='ignore'):
                        sigma = 1.0 / np.sqrt(np.diag(hess[i]))
                    size = max(size, float(np.max(np.abs(edge) / sigma)))
            trial[j, columns] = cur[i][columns] + delta
            solved[j] = True
            small[j] = lam[i] <= 1.0 and size < CONVERGED_SIGMA
        f_trial = np.asarray((yield 'lnpost', trial), dtype=np.float64)
        for j, i in enumerate(idx):
            iters[i] += 1
            if solved[j] and np.isfinite(f_trial[j]) and f_trial[j] > f_cur[i]:
                cur[i], f_cur[i] = trial[j], f_trial[j]
                stale[i] = True
                lam[i] = max(lam[i] * 0.1, 1e-12)
            else:
                lam[i] *= 10.0
            if small[j]:
                converged[i], running[i] = True, False
            elif lam[i] > 1e12:                      # nothing uphill at any step length
                running[i] = False
    need = np.flatnonzero(stale & np.isfinite(f_cur))
    if len(need):                                    # the curvature AT the result
        h_new, g_new = yield 'curvature', cur[need]
        hess[need], grad[need] = h_new, g_new
    return [ModeResult(cur[i], f_cur[i], columns, hess[i], iters[i], converged[i]) for i in range(n)]


# ---------------------------------------------------------------------------
# a model's columns, steps and priors
# ---------------------------------------------------------------------------
def _column_priors(model):
    """[(prior, element)] per column of the model's parameter vector; for a `JointModel`, of the joint vector (its
    column blocks stand in joint column order)."""
    out = []
    if hasattr(model, 'field_models'):
        for prior, cols, _ in model._blocks:
            out += [(prior, j) for j in range(cols.stop - cols.start)]
        return out
    for comp in model.components:
        for name, width in zip(comp.free_names(), comp.stochastic_lens()):
            out += [(comp._priors[name], j) for j in range(width)]
    return out


def default_columns(model):
    """Every free column whose prior is not discrete (the PSF index and its like stay at the base value)."""
    return np.array([c for c, (prior, _) in enumerate(_column_priors(model)) if not prior.discrete], dtype=np.int64)


def default_steps(model, theta, columns):
    """[n, K] steps: 1e-4 x the prior's standard deviation (scipy's frozen `.std()`) where that is finite and
    positive, else 1e-4 x max(|theta_k|, 1)."""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    sds = getattr(model, '_prior_sd', None)          # scipy's frozen .std() costs a millisecond a column: once per model
    if sds is None:
        sds = model._prior_sd = _prior_sds(model)
    step = np.empty((theta.shape[0], len(columns)))
    for k, col in enumerate(columns):
        sd = sds[col]
        if np.isfinite(sd) and sd > 0:
            step[:, k] = STEP_FRACTION * sd
        else:
            step[:, k] = STEP_FRACTION * np.maximum(np.abs(theta[:, col]), 1.0)
    return step


def _prior_sds(model):
    """[P] standard deviation of every column's prior, NaN where there is none to ask."""
    out = []
    for prior, elem in _column_priors(model):
        sd = np.nan
        rv = getattr(prior, 'rv_frozen', None)
        if rv is not None:
            try:
                with np.errstate(all='ignore'):
                    all_sd = np.ravel(np.asarray(rv.std(), dtype=np.float64))
                sd = all_sd[elem if all_sd.size > 1 else 0]
            except Exception:
                sd = np.nan
        out.append(sd)
    return np.array(out, dtype=np.float64)


def prior_derivatives(log_prior, theta, step, columns):
    """Central differences of a separable log-prior: log_prior([m, P]) -> [m]; -> (d ln prior / d theta_k [n, K],
    d^2 ln prior / d theta_k^2 [n, K]).  Zero where a stencil point leaves the support (and for a Uniform prior)."""
    sten = stencil(theta, step, columns)
    n, n_st, p = sten.shape
    with np.errstate(all='ignore'):
        lp = np.asarray(log_prior(sten.reshape(-1, p)), dtype=np.float64).reshape(n, n_st)
    step = np.broadcast_to(np.asarray(step, dtype=np.float64), (n, len(columns)))
    plus, minus, base = lp[:, 1::2], lp[:, 2::2], lp[:, :1]
    with np.errstate(all='ignore'):
        first = (plus - minus) / (2 * step)
        second = (plus - 2 * base + minus) / (step * step)
    ok = np.isfinite(plus) & np.isfinite(minus) & np.isfinite(base)
    return np.where(ok, first, 0.0), np.where(ok, second, 0.0)


def find_mode(model, start=None, n_draws=1024, n_starts=4, max_iter=50, rng=None):
    """The posterior mode of a `MultiComponentModel` -- or of a `JointModel`, over its joint columns -- by
    Levenberg-Marquardt on the log-posterior, with the Fisher matrix and gradient of the likelihood from the device
    (`model.fisher`) and the priors' derivatives from central differences of `log_priors_batch` on the host.  A joint
    result is in joint terms: `cov` and `laplace_log_evidence` over the continuous joint columns, the discrete ones
    (every exposure's PSF index) left at their start values.

    start     [P] or [n, P] start vectors; None: `n_draws` prior draws are evaluated in one batch and the best
              `n_starts` run side by side (one `fisher` and one `log_posterior_batch` call per iteration for all)
    rng       a numpy RandomState (or a seed) for the prior draws; None: numpy's global generator, like
              `init_params_from_priors`
    Returns the best start's `ModeResult` (theta, lnpost, cov, columns, iterations, converged, ok,
    laplace_log_evidence -- an approximation to set beside `model_galaxy_ptmcmc`'s evidence, not a replacement)."""
    columns = default_columns(model)
    if len(columns) == 0:
        raise ValueError('the model has no continuous free parameter')
    if start is None:
        draws = _prior_draws(model, int(n_draws), rng)
        lp = np.asarray(model.log_posterior_batch(draws), dtype=np.float64)
        lp = np.where(np.isfinite(lp), lp, -np.inf)
        order = np.argsort(-lp, kind='mergesort')[:max(int(n_starts), 1)]
        order = order[np.isfinite(lp[order])]
        if len(order) == 0:
            raise ValueError('none of the {} prior draws has a finite log-posterior'.format(n_draws))
        starts = draws[order]
    else:
        starts = np.atleast_2d(np.asarray(start, dtype=np.float64))

    def curvature(thetas):
        step = default_steps(model, thetas, columns)
        fi = model.fisher(thetas, step=step, columns=columns)
        first, second = prior_derivatives(model.log_priors_batch, thetas, step, columns)
        hess = fi['F'].copy()
        hess[:, np.arange(len(columns)), np.arange(len(columns))] -= second
        return hess, fi['grad'] + first

    inside = lambda thetas: np.isfinite(model.log_priors_batch(thetas))
    results = lm_search(curvature, model.log_posterior_batch, starts, columns, max_iter=max_iter, feasible=inside)
    return max(results, key=lambda r: (r.lnpost if np.isfinite(r.lnpost) else -np.inf))


def _pack_fields(parts, capacity):
    """Consecutive slices of several fields' rows in calls of at most `capacity` rows: parts [(field, n_rows)] ->
    list of calls, each a list of (field, lo, hi)."""
    calls, room = [[]], capacity
    for f, n in parts:
        lo = 0
        while lo < n:
            if room == 0:
                calls.append([])
                room = capacity
            hi = min(n, lo + room)
            calls[-1].append((f, lo, hi))
            room -= hi - lo
            lo = hi
    return [c for c in calls if c]


def _set_log_posteriors(fieldset, thetas):
    """`FieldSet.log_posterior_batch` of {field: [m, P]} in as few calls as `max_walkers` allows -> {field: [m]}."""
    out = {f: np.empty(len(t)) for f, t in thetas.items()}
    for call in _pack_fields([(f, len(thetas[f])) for f in sorted(thetas)], fieldset.max_walkers):
        batch = [None] * len(fieldset.models)
        for f, lo, hi in call:
            batch[f] = thetas[f][lo:hi]
        got = fieldset.log_posterior_batch(batch)
        for f, lo, hi in call:
            out[f][lo:hi] = got[f]
    return out


def find_modes(fieldset, start=None, n_draws=1024, n_starts=4, max_iter=50, rng=None):
    """`find_mode` for every field of a `FieldSet` at once: the fields' searches advance side by side under
    `lm_search`'s rule, and one iteration is ONE `FieldSet.fisher` call and ONE `FieldSet.log_posterior_batch` call for
    all fields and starts (split only where `max_walkers` is too small); the priors' derivatives and the edge
    bisection stay on the host.  Field f's result is what `find_mode(fieldset.models[f], ...)` finds from the same
    starts.

    start   None, or one [n, P] (or [P]) array per field
    rng     one RandomState or seed for all fields' prior draws (taken in field order), or a list of one per field
    Returns a list of `ModeResult`, one per field."""
    models = fieldset.models
    n_f = len(models)
    columns = [default_columns(m) for m in models]
    if any(len(c) == 0 for c in columns):
        raise ValueError('the model has no continuous free parameter')
    if start is None:
        rngs = list(rng) if isinstance(rng, (list, tuple)) else [rng] * n_f
        if len(rngs) != n_f:
            raise ValueError('rng: one generator, or one per field ({} given for {} fields)'.format(len(rngs), n_f))
        if rng is not None and not isinstance(rng, (list, tuple, np.random.RandomState)):
            rngs = [np.random.RandomState(rng)] * n_f          # one seed: one stream, the fields in order
        draws = {f: _prior_draws(m, int(n_draws), rngs[f]) for f, m in enumerate(models)}
        lps = _set_log_posteriors(fieldset, draws)
        starts = []
        for f in range(n_f):
            lp = np.where(np.isfinite(lps[f]), lps[f], -np.inf)
            order = np.argsort(-lp, kind='mergesort')[:max(int(n_starts), 1)]
            order = order[np.isfinite(lp[order])]
            if len(order) == 0:
                raise ValueError('field {}: none of the {} prior draws has a finite log-posterior'.format(f, n_draws))
            starts.append(draws[f][order])
    else:
        if len(start) != n_f:
            raise ValueError('start: one [n, P] array per field ({} given for {} fields)'.format(len(start), n_f))
        starts = [np.atleast_2d(np.asarray(s, dtype=np.float64)) for s in start]

    def curvatures(thetas):
        fields = sorted(thetas)
        steps = {f: default_steps(models[f], thetas[f], columns[f]) for f in fields}
        fis = fieldset.fisher([thetas.get(f) for f in range(n_f)], step=[steps.get(f) for f in range(n_f)],
                              columns=columns)
        out = {}
        for f in fields:
            first, second = prior_derivatives(models[f].log_priors_batch, thetas[f], steps[f], columns[f])
            hess = fis[f]['F'].copy()
            hess[:, np.arange(len(columns[f])), np.arange(len(columns[f]))] -= second
            out[f] = (hess, fis[f]['grad'] + first)
        return out

    def inside(model):
        return lambda thetas: np.isfinite(model.log_priors_batch(thetas))

    serve = (('curvature', curvatures), ('lnpost', lambda thetas: _set_log_posteriors(fieldset, thetas)))
    searches = [_lm_steps(starts[f], columns[f], max_iter, 1e-3, inside(models[f])) for f in range(n_f)]
    pending = [next(s) for s in searches]
    results = [None] * n_f
    while any(p is not None for p in pending):
        for kind, call in serve:                     # every search asks for curvatures first, then log-posteriors
            who = [f for f in range(n_f) if pending[f] is not None and pending[f][0] == kind]
            if not who:
                continue
            with np.errstate(all='ignore'):
                answers = call({f: pending[f][1] for f in who})
            for f in who:
                try:
                    pending[f] = searches[f].send(answers[f])
                except StopIteration as done:
                    pending[f], results[f] = None, done.value
    return [max(res, key=lambda r: (r.lnpost if np.isfinite(r.lnpost) else -np.inf)) for res in results]


def _prior_draws(model, n, rng):
    """n vectors from the priors (`init_params_from_priors`, which draws from numpy's global generator), from `rng`
    if given: the global generator's state is put back afterwards."""
    if rng is None:
        return model.init_params_from_priors(n)
    if not isinstance(rng, np.random.RandomState):
        rng = np.random.RandomState(rng)
    keep = np.random.get_state()
    np.random.set_state(rng.get_state())
    try:
        return model.init_params_from_priors(n)
    finally:
        rng.set_state(np.random.get_state())
        np.random.set_state(keep)


def draw_about_mode(theta, cov, columns, n_walkers, random, log_prior=None, others=None):
    """Walker start positions around a mode: theta[columns] + L z, L L^T = cov, z standard normal from the
    RandomState `random`; the other columns from `others` [n_walkers, P] (prior draws of the discrete columns;
    default: the mode's values).  A walker whose `log_prior` ([m, P] -> [m]) is not finite is drawn again, at most
    100 times, then ValueError."""
    theta = np.asarray(theta, dtype=np.float64)
    columns = np.asarray(columns, dtype=np.int64)
    chol = np.linalg.cholesky(np.asarray(cov, dtype=np.float64))
    out = np.tile(theta, (n_walkers, 1)) if others is None else np.array(others, dtype=np.float64)
    todo = np.arange(n_walkers)
    for _ in range(MAX_REDRAWS):
        z = random.normal(size=(len(todo), len(columns)))
        out[np.ix_(todo, columns)] = theta[columns] + np.dot(z, chol.T)
        if log_prior is None:
            return out
        with np.errstate(all='ignore'):
            todo = todo[~np.isfinite(np.asarray(log_prior(out[todo]), dtype=np.float64))]
        if len(todo) == 0:
            return out
    raise ValueError('{} walkers drawn around the mode are still outside the priors after {} tries'.format(
        len(todo), MAX_REDRAWS))
