"""
Affine-invariant ensemble sampler (Goodman & Weare 2010 stretch move) with the
interface of emcee 2.2.1's `EnsembleSampler`, which the reference drives
(psfMC/fitting.py:56-86, psfMC/database.py:18-19, analysis/statistics.py:145).

emcee is not installable here (no network) and is not vendored by the
reference, so this is written from the published algorithm and emcee's
documented API; SURVEY.md Appendix A lists the behaviour it reproduces:
two half-ensemble proposals per iteration, `z ~ g(z) ∝ 1/sqrt(z)` on [1/a, a],
acceptance `ln q = (dim-1) ln z + lnp(new) - lnp(old) > ln U`, a
`numpy.random.RandomState` owned by the sampler, `(lnprob, blob)` results,
`ValueError` on NaN log-probabilities or non-finite parameters, the `pool.map`
hook, `chain [nwalkers, iterations, dim]`, `lnprobability`, `acceptance_fraction`,
`reset`, `clear_blobs`, `get_autocorr_time`.  PARITY UNPINNED against emcee
itself (no copy available); its statistical behaviour is tested on Gaussian
targets (tests/test_sampler.py).

What is new: every half-step evaluates its walkers in ONE call --
`batch_lnpostfn([n, dim]) -> [n]` (e.g. `model.log_posterior_batch`, one GPU
batch) or `pool.map` (e.g. `BatchLogPosterior.as_pool()`), instead of one Python
call per walker.
"""
import threading

import numpy as np

__all__ = ['EnsembleSampler', 'DeviceEnsembleSampler', 'FieldSetSampler', 'TemperedEnsembleSampler',
           'DeviceTemperedSampler', 'default_betas', 'AutocorrError', 'integrated_time',
           'StretchMove', 'DEMove', 'moves_label']


class AutocorrError(Exception):
    """The chain is too short to estimate the autocorrelation time."""


def autocorr_function(x, axis=0):
    """Normalised autocorrelation function along `axis` (FFT based)."""
    x = np.atleast_1d(x)
    n = x.shape[axis]
    idx = [slice(None)] * x.ndim
    f = np.fft.fft(x - np.mean(x, axis=axis, keepdims=True), n=2 * n, axis=axis)
    idx[axis] = slice(0, n)
    acf = np.fft.ifft(f * np.conjugate(f), axis=axis)[tuple(idx)].real
    idx[axis] = slice(0, 1)
    return acf / acf[tuple(idx)]


def integrated_time(x, low=10, high=None, step=1, c=10, axis=0):
    """Integrated autocorrelation time with the self-consistent window of
    emcee 2.x: the smallest window M in [low, high) with M > c * tau(M)."""
    size = 0.5 * x.shape[axis]
    if int(c * low) >= size:
        raise AutocorrError('The chain is too short')
    f = autocorr_function(x, axis=axis)
    if high is None:
        high = int(size / c)
    idx = [slice(None)] * f.ndim
    for m in np.arange(low, high, step).astype(int):
        idx[axis] = slice(1, m)
        tau = 1 + 2 * np.sum(f[tuple(idx)], axis=axis)
        if np.all(tau > 1.0) and m > c * tau.max():
            return tau
        if c * tau.max() >= size:           # emcee 2.2.1 gives up here (recalled; parity unpinned)
            break
    raise AutocorrError('The chain is too short to reliably estimate the '
                        'autocorrelation time')


class _Wrapped(object):
    """lnpostfn with its extra arguments bound (a fresh kwargs dict per call:
    the reference's log_posterior pops 'model' from it, models.py:205)."""

    def __init__(self, f, args, kwargs):
        self.f, self.args, self.kwargs = f, list(args or []), dict(kwargs or {})

    def __call__(self, x):
        return self.f(x, *self.args, **self.kwargs)


class StretchMove(object):
    """The Goodman & Weare stretch move, the proposal of `EnsembleSampler(moves=None)`: per half-step
    `z = ((a-1) rand(half) + 1)^2 / a`, `partner = randint(half, size=half)`, `ln u = log(rand(half))`;
    `q_i = c[partner_i] - z_i (c[partner_i] - s_i)`, accepted where `(P-1) ln z + lnp_new - lnp > ln u`."""

    kind, name = 0, 'stretch'               # (the library's PSFMC_MOVE_STRETCH)

    def __init__(self, a=2.0):
        self.a = float(a)

    def check(self, nwalkers):
        pass

    def draw(self, rs, half, dim):
        """One half-step's random numbers -> (scalar [half], Hastings term [half], a [half], b [half], ln u
        [half]); b is not used."""
        z = ((self.a - 1.0) * rs.rand(half) + 1) ** 2.0 / self.a
        a = rs.randint(half, size=(half,))
        log_u = np.log(rs.rand(half))
        return z, (dim - 1.0) * np.log(z), a, np.zeros(half, dtype=a.dtype), log_u

    @staticmethod
    def propose(s, c, z, a, b):
        return c[a] - z[:, np.newaxis] * (c[a] - s)


class DEMove(object):
    """Differential evolution (ter Braak 2006) on the split ensemble, as emcee 3's `DEMove`: walker i of the
    active half s takes two DISTINCT walkers a_i != b_i of the complementary half c and proposes
    `q_i = s_i + g_i (c[a_i] - c[b_i])`.  The proposal is symmetric: the Hastings term is 0 and it is accepted
    where `lnp_new - lnp > ln u`.  `g_i = gamma0 (1 + sigma (2 u1_i - 1))`, `gamma0` by default
    `2.38 / sqrt(2 P)`; with probability `jump` g_i is exactly 1.0 instead (ter Braak's mode-jumping step).

    The jitter of g is UNIFORM, not emcee's normal, on purpose: the draws then use `rand` and `randint` only,
    and `DeviceEnsembleSampler._state_snapshotter` relies on the generator's Gaussian cache never being touched.

    Draw order per half-step, whatever the options: `rand(half)` -> u1, `rand(half)` -> the jump selector (g_i = 1
    where it is < jump), `randint(half, size=half)` -> a, `randint(half - 1, size=half)` -> b then `b += (b >= a)`,
    `rand(half)` -> u.  The proposal is three roundings, never fused: `diff = c[a] - c[b]`, `step = g * diff`,
    `q = s + step`.  Needs two walkers to choose from in each half: nwalkers >= 4."""

    kind, name = 1, 'de'                    # (the library's PSFMC_MOVE_DE)

    def __init__(self, sigma=1e-5, gamma0=None, jump=0.0):
        self.sigma = float(sigma)
        self.gamma0 = None if gamma0 is None else float(gamma0)
        self.jump = float(jump)
        if not (np.isfinite(self.sigma) and 0.0 <= self.jump <= 1.0) or \
                (self.gamma0 is not None and not np.isfinite(self.gamma0)):
            raise ValueError('DEMove needs finite sigma and gamma0, and jump in [0, 1]')

    def check(self, nwalkers):
        if nwalkers < 4:
            raise ValueError('DEMove needs at least 4 walkers (two distinct partners in each half-ensemble); '
                             'got {}'.format(nwalkers))

    def draw(self, rs, half, dim):
        """One half-step's random numbers -> (g [half], Hastings term (0) [half], a [half], b [half], ln u [half])."""
        u1 = rs.rand(half)
        jump = rs.rand(half)
        a = rs.randint(half, size=(half,))
        b = rs.randint(half - 1, size=(half,))
        b += (b >= a)
        log_u = np.log(rs.rand(half))
        gamma0 = self.gamma0 if self.gamma0 is not None else 2.38 / np.sqrt(2.0 * dim)
        g = gamma0 * (1.0 + self.sigma * (2.0 * u1 - 1.0))
        g[jump < self.jump] = 1.0
        return g, np.zeros(half), a, b, log_u

    @staticmethod
    def propose(s, c, g, a, b):
        diff = c[a] - c[b]
        step = g[:, np.newaxis] * diff
        return s + step


def _parse_moves(moves, nwalkers):
    """`moves=` -> (list of moves, cumulative normalised weights): a single move, or a list of (move, weight)."""
    if hasattr(moves, 'draw'):
        pairs = [(moves, 1.0)]
    else:
        try:
            pairs = [(m, float(w)) for m, w in moves]
        except (TypeError, ValueError):
            raise ValueError('moves must be None, a move, or a list of (move, weight) pairs')
    if not pairs or not all(hasattr(m, 'draw') and hasattr(m, 'propose') for m, _ in pairs):
        raise ValueError('moves must be None, a move, or a list of (move, weight) pairs')
    weights = np.array([w for _, w in pairs], dtype=np.float64)
    if not np.all(np.isfinite(weights)) or np.any(weights < 0) or not weights.sum() > 0:
        raise ValueError('move weights must be finite, non-negative and not all zero')
    for m, _ in pairs:
        m.check(nwalkers)
    cum = np.cumsum(weights / weights.sum())
    cum[-1] = 1.0
    return [m for m, _ in pairs], cum


def moves_label(moves):
    """'stretch:0.5,de:0.5': the moves and their normalised weights, as the database header's MCMOVES records
    them; None for moves=None."""
    if moves is None:
        return None
    pairs = [(moves, 1.0)] if hasattr(moves, 'draw') else [(m, float(w)) for m, w in moves]
    total = sum(w for _, w in pairs)
    return ','.join('{}:{:g}'.format(getattr(m, 'name', type(m).__name__), w / total) for m, w in pairs)


def _kept(done, n, thin):
    """The kept iterations of a block of n that starts at iteration `done`: iteration done + i is kept iff
    (done + i) % thin == 0, at index (done + i) // thin -- an arithmetic progression.  -> (first, count, offset):
    the block's positions first::thin, `count` of them, stored from index i0 + offset on."""
    first = (-done) % thin
    count = (n - first + thin - 1) // thin if first < n else 0
    return first, count, (done + first) // thin


class _SamplerState(object):
    """What `EnsembleSampler` and `TemperedEnsembleSampler` have in common: the moves, the generator and the
    beta = 1 chain's storage and readers.  Reads `k` (walkers per ensemble), `dim`, `_random`, `_chain` [W, n, P], `_lnprob` [W, n]
    and, once `set_moves` has run, `_moves` / `_move_cum`."""

    def set_moves(self, moves):
        """The proposal moves of the coming iterations (named after the library's psfmc_stretch_set_moves): None
        (the stretch move with this sampler's `a`, the path of a sampler that never had moves), one move, or
        (move, weight) pairs, parsed by `_parse_moves` against this sampler's walkers per ensemble.  Every sampler
        of this module has it; call it before the first `sample()` or between two `sample()` calls."""
        self._moves, self._move_cum = (None, None) if moves is None else _parse_moves(moves, self.k)

    def _select_move(self):
        """The move of the coming iteration (`moves=`): one `rand()` when there is more than one to choose from."""
        if len(self._moves) == 1:
            return 0
        r = self._random.rand()
        return min(int(np.searchsorted(self._move_cum, r, side='right')), len(self._moves) - 1)

    def clear_blobs(self):
        pass

    def _grow_storage(self, iterations, thin, storechain):
        """Room for the kept iterations of a `sample()` call; -> the index of its first one."""
        i0 = self._chain.shape[1]
        if storechain:
            n_keep = int(iterations // thin)
            self._chain = np.concatenate((self._chain, np.zeros((self.k, n_keep, self.dim))), axis=1)
            self._lnprob = np.concatenate((self._lnprob, np.zeros((self.k, n_keep))), axis=1)
        return i0

    @property
    def random_state(self):
        return self._random.get_state()

    @random_state.setter
    def random_state(self, state):
        try:
            self._random.set_state(state)
        except (TypeError, ValueError):
            pass

    @property
    def chain(self):
        return self._chain

    @property
    def flatchain(self):
        s = self._chain.shape
        return self._chain.reshape(s[0] * s[1], s[2])

    @property
    def lnprobability(self):
        return self._lnprob

    @property
    def flatlnprobability(self):
        return self._lnprob.flatten()

    @property
    def acor(self):
        return self.get_autocorr_time()

    def get_autocorr_time(self, low=10, high=None, step=1, c=10):
        return integrated_time(np.mean(self._chain, axis=0), axis=0, low=low, high=high,
                               step=step, c=c)


class EnsembleSampler(_SamplerState):
    """moves: None (the stretch move with this sampler's `a`: emcee 2.2.1's sampler, draw for draw), a single
    move (`StretchMove`, `DEMove`), or a list of (move, weight) pairs.  With more than one move ONE extra `rand()`
    is drawn at the start of every iteration and selects, by cumulative normalised weight, the move of BOTH
    half-steps of that iteration; with exactly one move no selector is drawn.  Each half-step then draws in its
    move's own order (see the move classes) and accepts where `(hastings + lnp_new) - lnp > ln u`.
    `set_moves(moves)` is the keyword after construction: before the first `sample()` or between two."""

    def __init__(self, nwalkers, dim, lnpostfn=None, a=2.0, args=None, kwargs=None,
                 threads=1, pool=None, live_dangerously=False, batch_lnpostfn=None, moves=None):
        self.k = int(nwalkers)
        self.set_moves(moves)
        if nwalkers % 2:
            raise ValueError('The number of walkers must be even.')
        if nwalkers < 2 * dim and not live_dangerously:
            raise ValueError('The number of walkers needs to be more than twice the '
                             'dimension of your parameter space.')
        if lnpostfn is None and batch_lnpostfn is None:
            raise ValueError('need lnpostfn or batch_lnpostfn')
        self.k, self.dim, self.a = int(nwalkers), int(dim), float(a)
        self.lnprobfn = _Wrapped(lnpostfn, args, kwargs) if lnpostfn is not None else None
        self.batch_lnpostfn = batch_lnpostfn
        self.pool = pool
        self.threads = threads
        self._random = np.random.mtrand.RandomState()
        self._last_run_mcmc_result = None
        self.reset()

    # -- state ----------------------------------------------------------------
    def reset(self):
        self.iterations = 0
        self.naccepted = np.zeros(self.k)
        self._chain = np.empty((self.k, 0, self.dim))
        self._lnprob = np.empty((self.k, 0))
        self._blobs = []
        self._last_run_mcmc_result = None

    clear_chain = reset

    def clear_blobs(self):
        self._blobs = []

    @property
    def blobs(self):
        return self._blobs

    @property
    def acceptance_fraction(self):
        return self.naccepted / max(self.iterations, 1)

    # -- evaluation -------------------------------------------------------------
    def _get_lnprob(self, pos):
        p = np.asarray(pos, dtype=np.float64)
        if np.any(np.isinf(p)):
            raise ValueError('At least one parameter value was infinite.')
        if np.any(np.isnan(p)):
            raise ValueError('At least one parameter value was NaN.')
        if self.batch_lnpostfn is not None:
            lnprob, blob = np.asarray(self.batch_lnpostfn(p), dtype=np.float64), None
        else:
            mapper = self.pool.map if self.pool is not None else map
            results = list(mapper(self.lnprobfn, [p[i] for i in range(len(p))]))
            try:
                lnprob = np.array([float(r[0]) for r in results])
                blob = [r[1] for r in results]
            except (IndexError, TypeError):
                lnprob = np.array([float(r) for r in results])
                blob = None
        if np.any(np.isnan(lnprob)):
            raise ValueError('lnprob returned NaN.')
        return lnprob, blob

    def _propose_stretch(self, p0, p1, lnprob0):
        s, c = np.atleast_2d(p0), np.atleast_2d(p1)
        ns, nc = len(s), len(c)
        zz = ((self.a - 1.0) * self._random.rand(ns) + 1) ** 2.0 / self.a
        rint = self._random.randint(nc, size=(ns,))
        q = c[rint] - zz[:, np.newaxis] * (c[rint] - s)
        newlnprob, blob = self._get_lnprob(q)
        lnpdiff = (self.dim - 1.0) * np.log(zz) + newlnprob - lnprob0
        accept = lnpdiff > np.log(self._random.rand(len(lnpdiff)))
        return q, newlnprob, accept, blob

    def _propose_move(self, move, p0, p1, lnprob0):
        s, c = np.atleast_2d(p0), np.atleast_2d(p1)
        scal, hastings, a, b, log_u = move.draw(self._random, len(s), self.dim)
        q = move.propose(s, c, scal, a, b)
        newlnprob, blob = self._get_lnprob(q)
        with np.errstate(invalid='ignore'):
            accept = hastings + newlnprob - lnprob0 > log_u
        return q, newlnprob, accept, blob

    # -- sampling ----------------------------------------------------------------
    def sample(self, p0, lnprob0=None, rstate0=None, blobs0=None, iterations=1, thin=1,
               storechain=True):
        """Generator advancing the ensemble; yields (pos, lnprob, rstate[, blobs])
        after every iteration."""
        if rstate0 is not None:
            self.random_state = rstate0
        p = np.array(p0, dtype=np.float64)
        if p.shape != (self.k, self.dim):
            raise ValueError('p0 must have shape ({}, {})'.format(self.k, self.dim))
        halfk = self.k // 2
        lnprob, blobs = lnprob0, blobs0
        if lnprob is None:
            lnprob, blobs = self._get_lnprob(p)
        lnprob = np.array(lnprob, dtype=np.float64)
        if np.any(np.isnan(lnprob)):
            raise ValueError('The initial lnprob was NaN.')
        i0 = self._grow_storage(iterations, thin, storechain)
        first, second = slice(halfk), slice(halfk, self.k)
        for i in range(int(iterations)):
            self.iterations += 1
            move = None if self._moves is None else self._moves[self._select_move()]
            for s0, s1 in ((first, second), (second, first)):
                if move is None:
                    q, newlnp, acc, blob = self._propose_stretch(p[s0], p[s1], lnprob[s0])
                else:
                    q, newlnp, acc, blob = self._propose_move(move, p[s0], p[s1], lnprob[s0])
                if np.any(acc):
                    lnprob[s0][acc] = newlnp[acc]
                    p[s0][acc] = q[acc]
                    self.naccepted[s0][acc] += 1
                    if blob is not None and blobs is not None:
                        full = np.arange(self.k)[s0][acc]
                        for j, src in zip(full, np.arange(len(acc))[acc]):
                            blobs[j] = blob[src]
            if storechain and i % thin == 0:
                ind = i0 + int(i // thin)
                self._chain[:, ind, :] = p
                self._lnprob[:, ind] = lnprob
                if blobs is not None:
                    self._blobs.append(list(blobs))
            if blobs is not None:
                yield p, lnprob, self.random_state, blobs
            else:
                yield p, lnprob, self.random_state

    def run_mcmc(self, pos0, N, rstate0=None, lnprob0=None, **kwargs):
        if pos0 is None:
            if self._last_run_mcmc_result is None:
                raise ValueError('Cannot have pos0=None if run_mcmc has never been called.')
            pos0, lnprob0, rstate0 = self._last_run_mcmc_result[:3]
        results = None
        for results in self.sample(pos0, lnprob0, rstate0, iterations=N, **kwargs):
            pass
        self._last_run_mcmc_result = results[:3] if results is not None else None
        return results


def _run_async(fn, *args, **kwargs):
    """Start fn(*args, **kwargs) on a thread; the returned callable joins and gives its result
    (or raises what it raised)."""
    box = {}

    def work():
        try:
            box['value'] = fn(*args, **kwargs)
        except BaseException as exc:            # re-raised by the caller
            box['error'] = exc

    th = threading.Thread(target=work)
    th.start()

    def join():
        th.join()
        if 'error' in box:
            raise box['error']
        return box['value']
    return join


def _run_blocks(iterations, block, draw, launch, overlap=True):
    """The block loop of every device sampler: `iterations` in blocks of at most `block`; yields, per block,
    (done, n, result, states): the iterations before it, its size, what `launch(draws)` returned and the states of
    `draw(n) -> (draws, states)`.  `draw` is never called with 0.
    overlap: the next block's random numbers are drawn while the GPU works on the current one (`launch` runs on a
    thread; the library call releases the GIL) -- the draws stay in the host sampler's order because the stream
    is sequential: block k+1 is drawn right after block k, only earlier in time.  Without it `launch` runs on the
    calling thread and the next draw follows it (the sharded route: collectives are issued from the caller's
    thread, in the same order on every rank).  A launch that fails raises once the draw beside it has ended, and
    a draw that fails still joins the launch."""
    done = 0
    draws, states = draw(min(block, iterations)) if iterations > 0 else (None, None)
    while done < iterations:
        n = min(block, iterations - done)
        n_next = min(block, iterations - done - n)
        block_states = states
        if overlap:
            job = _run_async(launch, draws)
            try:
                draws, states = draw(n_next) if n_next > 0 else (None, None)
            finally:
                result = job()
        else:
            result = launch(draws)
            draws, states = draw(n_next) if n_next > 0 else (None, None)
        yield done, n, result, block_states
        done += n


_HALF_STEP = ('z', 'lz', 'partner', 'log_u', 'partner_b')


class _Draws(object):
    """The random numbers of a block of iterations, by name.  Per half-step, [n_iter, 2, (T,) W/2]: `z` (the move's
    scalar), `lz` (its Hastings term), `partner`, `log_u` and, with moves, `partner_b`; with moves `kind`
    [n_iter]; for a ladder the swaps' `swap_i`, `swap_j`, `swap_log_u` [n_iter, T-1, W].  What a draw does not have
    is None: `kind is None` is the run without moves.  Iterating gives the arrays that are there, in the order
    below -- the argument order of every entry point (`stretch_run`, `move_run`, `pt_run`, `pt_move_run` and their
    `_fields` forms), so a launch is `run(pos, lnp, *draws, ...)`."""

    __slots__ = ('z', 'lz', 'partner', 'log_u', 'kind', 'partner_b', 'swap_i', 'swap_j', 'swap_log_u')

    def __init__(self, **arrays):
        for name in self.__slots__:
            setattr(self, name, arrays.pop(name, None))
        if arrays:
            raise TypeError('not a draw: {}'.format(sorted(arrays)))

    def __iter__(self):
        return (a for a in (getattr(self, name) for name in self.__slots__) if a is not None)


def _stack_fields(per, one_rung=False):
    """The fields' draws as one, by name, in the shapes of the `_fields` entry points: the half-step arrays
    [n_iter, 2, F, T, W/2], the swaps' [n_iter, F, T-1, W], kind [n_iter, F].  one_rung: the fields' draws are an
    ensemble's, without a rung axis, and get T = 1."""
    out = {}
    for name in _Draws.__slots__:
        parts = [getattr(d, name) for d in per]
        if parts[0] is None:
            continue
        if one_rung and name in _HALF_STEP:
            parts = [a[:, :, np.newaxis, :] for a in parts]
        out[name] = np.ascontiguousarray(np.stack(parts, axis=2 if name in _HALF_STEP else 1))
    return _Draws(**out)


def _check_start(p, lnprob, shape, evaluate):
    """The start-state checks of the device samplers: p a float64 array of `shape`, finite; lnprob (from
    `evaluate(p)` when None) without NaN.  -> lnprob."""
    if p.shape != shape:
        raise ValueError('p0 must have shape ({})'.format(', '.join(str(s) for s in shape)))
    if np.any(~np.isfinite(p)):
        raise ValueError('At least one parameter value was infinite or NaN.')
    if lnprob is None:
        lnprob = evaluate(p)
    if np.any(np.isnan(lnprob)):
        raise ValueError('The initial lnprob was NaN.')
    return lnprob


class _DeviceMember(object):
    """The host side of one device-resident ensemble or ladder: the cheap state snapshot, the accumulate counters,
    and (subclasses) the draws in the host sampler's order and the store of a block's kept iterations.  Mixed into
    a host sampler, of which it reads `_random`, `k`, `dim`, `a`, `_moves`, `_select_move()`, `_chain`, `_lnprob`
    and, for ladders, `ntemps` and `_lnlike`; `model` is the member's model."""

    def _state_snapshotter(self):
        """A cheap `get_state()` for the per-iteration snapshots: `RandomState.get_state` costs
        ~50 us (it would double the host time per iteration); the MT19937 key and position are
        copied straight from the bit generator's state block (1 us), the Gaussian cache -- which
        `rand` / `randint` never touch -- is taken from one full call.  Falls back to `get_state`
        if the bit generator does not expose its state the expected way."""
        rs = self._random
        full = rs.get_state()
        try:
            import ctypes
            bg = rs._bit_generator
            if type(bg).__name__ != 'MT19937':
                return rs.get_state
            block = (ctypes.c_uint32 * 625).from_address(bg.ctypes.state_address)
            view = np.frombuffer(block, dtype=np.uint32)
            if not (np.array_equal(view[:624], full[1]) and int(view[624]) == full[2]):
                return rs.get_state
        except Exception:
            return rs.get_state
        tail = tuple(full[3:])

        def snap():
            a = view.copy()
            return ('MT19937', a[:624], int(a[624])) + tail
        return snap

    def _count_accumulated(self, samples):
        self.model._device_samples += samples
        self.model.accumulated_samples += samples


class _EnsembleMember(_DeviceMember):
    """A device-resident ensemble: `DeviceEnsembleSampler`, and a field's share of a `FieldSetSampler`."""

    def _draw(self, n_iter):
        """Random numbers of n_iter iterations in emcee's order (per half-step: rand(Ns) -> z, randint(Nc, Ns) ->
        partner, rand(Ns) -> ln u) or, with moves, in the order of `EnsembleSampler(moves=...)`: per iteration
        the selector `rand()` (more than one move only), then each half-step's draws in its move's order.
        -> (`_Draws`, the generator state after each iteration's draws)."""
        half = self.k // 2
        z = np.empty((n_iter, 2, half))
        partner = np.empty((n_iter, 2, half), dtype=np.int32)
        log_u = np.empty((n_iter, 2, half))
        moves = self._moves is not None
        if moves:
            lz = np.empty((n_iter, 2, half))
            partner_b = np.zeros((n_iter, 2, half), dtype=np.int32)
            kind = np.empty(n_iter, dtype=np.int32)
        rs = self._random
        states = []
        snap = self._state_snapshotter()
        for it in range(n_iter):
            if moves:
                move = self._moves[self._select_move()]
                kind[it] = move.kind
            for h in range(2):
                if moves:
                    z[it, h], lz[it, h], partner[it, h], partner_b[it, h], log_u[it, h] = \
                        move.draw(rs, half, self.dim)
                    continue
                z[it, h] = ((self.a - 1.0) * rs.rand(half) + 1) ** 2.0 / self.a
                partner[it, h] = rs.randint(half, size=(half,))
                log_u[it, h] = np.log(rs.rand(half))
            states.append(snap())
        if moves:
            return _Draws(z=z, lz=lz, partner=partner, log_u=log_u, kind=kind, partner_b=partner_b), states
        return _Draws(z=z, lz=(self.dim - 1.0) * np.log(z), partner=partner, log_u=log_u), states

    def _store_block(self, i0, done, n, thin, chain, lnchain):
        """The kept iterations of a block (chain [W, n, P], lnchain [W, n]) into the storage grown from i0 on:
        an arithmetic progression, copied with slices (index arrays made this 1.6 ms per block)."""
        first, count, offset = _kept(done, n, thin)
        if count:
            dst = i0 + offset
            self._chain[:, dst:dst + count, :] = chain[:, first::thin, :]
            self._lnprob[:, dst:dst + count] = lnchain[:, first::thin]


class _LadderMember(_DeviceMember):
    """A device-resident ladder: `DeviceTemperedSampler`, and a field's share of a `FieldSetTemperedSampler`."""

    def _draw(self, n_iter):
        """Random numbers of n_iter iterations in the host sampler's order: the arrays of `Context.pt_run` or,
        with moves set, of `Context.pt_move_run` -- the selector `rand()` of every iteration drawn here too (more
        than one move only), z the moves' scalar, lz their Hastings term, kind [n_iter] and partner_b added.
        -> (`_Draws`, the generator state after each iteration's draws)."""
        n_t, n_w, half = self.ntemps, self.k, self.k // 2
        n_s = max(n_t - 1, 0)
        z = np.empty((n_iter, 2, n_t, half))
        partner = np.empty((n_iter, 2, n_t, half), dtype=np.int32)
        log_u = np.empty((n_iter, 2, n_t, half))
        si = np.empty((n_iter, n_s, n_w), dtype=np.int32)
        sj = np.empty((n_iter, n_s, n_w), dtype=np.int32)
        slu = np.empty((n_iter, n_s, n_w))
        moves = self._moves is not None
        if moves:
            lz = np.empty((n_iter, 2, n_t, half))
            partner_b = np.zeros((n_iter, 2, n_t, half), dtype=np.int32)
            kind = np.empty(n_iter, dtype=np.int32)
        rs = self._random
        states = []
        snap = self._state_snapshotter()
        for it in range(n_iter):
            if moves:
                move = self._moves[self._select_move()]
                kind[it] = move.kind
            for h in range(2):
                for t in range(n_t):
                    if moves:
                        z[it, h, t], lz[it, h, t], partner[it, h, t], partner_b[it, h, t], log_u[it, h, t] = \
                            move.draw(rs, half, self.dim)
                        continue
                    z[it, h, t] = ((self.a - 1.0) * rs.rand(half) + 1) ** 2.0 / self.a
                    partner[it, h, t] = rs.randint(half, size=(half,))
                    log_u[it, h, t] = np.log(rs.rand(half))
            for t in range(n_t - 1, 0, -1):
                si[it, t - 1] = rs.permutation(n_w)
                sj[it, t - 1] = rs.permutation(n_w)
                slu[it, t - 1] = np.log(rs.rand(n_w))
            states.append(snap())
        swaps = dict(swap_i=si, swap_j=sj, swap_log_u=slu)
        if moves:
            return _Draws(z=z, lz=lz, partner=partner, log_u=log_u, kind=kind, partner_b=partner_b, **swaps), states
        return _Draws(z=z, lz=(self.dim - 1.0) * np.log(z), partner=partner, log_u=log_u, **swaps), states

    def _store_block(self, i0, done, n, thin, chain, lnchain, llchain):
        """The kept iterations of a block into the storage grown from i0 on: the beta = 1 rung of chain
        [T, W, n, P], its lnchain [W, n], and every rung's llchain [T, W, n]."""
        first, count, offset = _kept(done, n, thin)
        if count:
            dst = i0 + offset
            self._chain[:, dst:dst + count, :] = chain[0, :, first::thin, :]
            self._lnprob[:, dst:dst + count] = lnchain[:, first::thin]
            self._lnlike[:, :, dst:dst + count] = llchain[:, :, first::thin]


class _FieldMembers(object):
    """What the two field-set samplers do to every member of `fields`."""

    def set_moves(self, moves):
        """`set_moves` for every field's ensemble or ladder."""
        for f in self.fields:
            f.set_moves(moves)

    def reset(self):
        for f in self.fields:
            f.reset()

    def clear_blobs(self):
        pass

    def _draw(self, n_iter, one_rung=False):
        """Every field's draws from its own generator, stacked by name (`_stack_fields`), and its states."""
        per = [f._draw(n_iter) for f in self.fields]
        return _stack_fields([d for d, _ in per], one_rung=one_rung), [s for _, s in per]


class DeviceEnsembleSampler(_EnsembleMember, EnsembleSampler):
    """The same sampler with the walkers resident on the GPU: proposal, log-posterior
    (priors included), acceptance and chain storage all run on the device
    (`psfmc_stretch_run`); the host only draws the random numbers, from the same
    `RandomState` in the same order as the host loop, so both samplers produce the
    same chain.  `block` iterations are enqueued per library call (nothing is copied
    back in between); `sample()` still yields once per iteration, each time with the
    generator state that follows that iteration's draws, while `iterations`, `naccepted`
    and the stored chain advance a whole block at a time.

    group: a torch.distributed process group (True = the default group) or a
    `parallel.RankGroup`: the walkers of every half-step's proposals are then sharded over the
    ranks (one process per GPU) -- each rank evaluates its contiguous block, the blocks'
    log-posteriors are all-gathered (the one collective of the path) and every rank applies the
    same accept / move, so all ranks hold the same chain, equal to the single-GPU chain bit for
    bit.  Every rank must construct the sampler with the same `random_state` and call `sample`
    with the same arguments.

    Needs a `MultiComponentModel` whose priors all belong to the families the library
    evaluates (uniform, normal, weibull_min, discrete uniform); otherwise use
    `EnsembleSampler(batch_lnpostfn=model.log_posterior_batch)`.

    moves: as `EnsembleSampler`'s (None, a move, or (move, weight) pairs).  With moves given the run goes
    through `psfmc_move_run` (`psfmc_move_run_joint` for a `JointModel`, `psfmc_stretch_set_moves` with
    `group`): a proposal kernel per half-step, plain half-steps, never whole-iteration launches.  The chain,
    `naccepted` and the yielded generator states equal those of `EnsembleSampler(...,
    batch_lnpostfn=model.log_posterior_batch, moves=moves)` bit for bit.  moves=None launches exactly what it
    always did.
    """

    def __init__(self, nwalkers, model, a=2.0, live_dangerously=False, block=64, accumulate=False,
                 group=None, moves=None):
        from .parallel import RankGroup, ShardedLogPosterior
        ranks = group if isinstance(group, RankGroup) else None
        if ranks is None and group is not None:
            ranks = RankGroup(None if group is True else group, 'cuda:%d' % model._device)
        self.ranks = ranks if ranks is not None and not ranks.single else None
        evaluate = (ShardedLogPosterior(model, group=self.ranks) if self.ranks is not None
                    else model.log_posterior_batch)
        super(DeviceEnsembleSampler, self).__init__(nwalkers, model.num_params, a=a,
                                                    batch_lnpostfn=evaluate,
                                                    live_dangerously=live_dangerously, moves=moves)
        self.model = model
        self.block = int(block)
        self.accumulate = bool(accumulate)
        if nwalkers > model._max_walkers:
            raise ValueError('model was built for at most {} walkers'.format(model._max_walkers))
        eng = model.engine                # context + layout
        self.set_moves(moves)             # (again, now that the engine is known)
        if not hasattr(type(eng), 'stretch_run'):
            # (a model of a FieldSet: its context is shared by the set's fields)
            eng.stretch_run()             # raises NotImplementedError naming the FieldSet
        if model._host_priors:
            raise ValueError('priors {} are evaluated on the host: the device sampler cannot be '
                             'used'.format([p.name for p, _ in model._host_priors]))

    def set_moves(self, moves):
        eng = getattr(getattr(self, 'model', None), 'engine', None)
        if moves is not None and eng is not None and not hasattr(type(eng), 'move_run'):
            raise NotImplementedError('moves= is not available on a {}: the proposal moves serve one-field models and '
                                      'joint fits (DESIGN.md section 21)'.format(type(eng).__name__))
        super(DeviceEnsembleSampler, self).set_moves(moves)

    def _run_block_sharded(self, pos, lnprob, draws, nacc, store=True, accumulate=False):
        """One block of iterations with every half-step's proposals sharded over the ranks
        (include/psfmc_hip.h psfmc_stretch_open / _half_eval / _half_accept / _close).  With `moves` the draws
        carry kind and partner_b: the open run then proposes by kind (psfmc_stretch_set_moves)."""
        rg, eng = self.ranks, self.model.engine
        torch = rg.torch
        n_iter, half = int(np.shape(draws.z)[0]), self.k // 2
        lo, hi = rg.block(half)
        a_lo, a_hi = rg.block(self.k)
        with torch.cuda.device(rg.device), rg.on_stream():
            stream = rg.stream_ptr()
            send = torch.zeros(rg.slot(half), dtype=torch.float64, device=rg.device)
            eng.stretch_open(pos, lnprob, draws.z, draws.lz, draws.partner, draws.log_u, nacc, store=store)
            if draws.kind is not None:
                eng.stretch_set_moves(draws.kind, draws.partner_b)
            for it in range(n_iter):
                for h in range(2):
                    eng.stretch_half_eval(it, h, lo, hi - lo, send.data_ptr(), stream)
                    full = rg.all_gather_blocks(send, half).contiguous()
                    eng.stretch_half_accept(it, h, full.data_ptr(), stream)
                if accumulate:
                    eng.stretch_accumulate(a_lo, a_hi - a_lo, stream)
            torch.cuda.current_stream(rg.device).synchronize()
            return eng.stretch_close(nacc, stream)

    def sample(self, p0, lnprob0=None, rstate0=None, blobs0=None, iterations=1, thin=1,
               storechain=True):
        if rstate0 is not None:
            self.random_state = rstate0
        p = np.array(p0, dtype=np.float64)
        lnprob = _check_start(p, None if lnprob0 is None else np.array(lnprob0, dtype=np.float64),
                              (self.k, self.dim), lambda q: self._get_lnprob(q)[0])
        i0 = self._grow_storage(iterations, thin, storechain)
        nacc = self.naccepted.astype(np.int64)
        eng = self.model.engine

        def launch(draws):
            if self.ranks is not None:
                return self._run_block_sharded(p, lnprob, draws, nacc, store=True, accumulate=self.accumulate)
            run = eng.stretch_run if draws.kind is None else eng.move_run
            return run(p, lnprob, *draws, nacc, store=True, accumulate=self.accumulate)

        # sharded: collectives are issued from this thread, and this rank sums its block of the walkers
        lo, hi = (0, self.k) if self.ranks is None else self.ranks.block(self.k)
        for done, n, result, states in _run_blocks(iterations, self.block, self._draw, launch,
                                                   overlap=self.ranks is None):
            p, lnprob, chain, lnchain = result
            if self.accumulate:
                self._count_accumulated(n * (hi - lo))
            # per-block bookkeeping in whole-array operations: at a few hundred microseconds
            # per iteration on the GPU, per-iteration numpy calls here were 10 % of the run
            if storechain:
                self._store_block(i0, done, n, thin, chain, lnchain)
            # counters advance with the block (the device reports acceptances per block), so
            # `acceptance_fraction` is consistent whenever the consumer looks; the yielded
            # generator state is the one right after iteration j's draws, so that
            # (pos, lnprob, rstate) of any yield resumes the same chain
            self.naccepted = nacc.astype(np.float64)
            self.iterations += n
            for j in range(n):
                yield chain[:, j, :].copy(), lnchain[:, j].copy(), states[j]


class _FieldChain(_EnsembleMember, EnsembleSampler):
    """One field's share of a `FieldSetSampler`: the emcee-style state (chain, lnprobability,
    acceptance counters, random state) of that field's ensemble -- what `save_database`,
    `check_convergence_autocorr` and the reference's own post-processing read."""

    def __init__(self, nwalkers, model, a=2.0):
        super(_FieldChain, self).__init__(nwalkers, model.num_params, a=a,
                                          batch_lnpostfn=model.log_posterior_batch)
        self.model = model


class FieldSetSampler(_FieldMembers):
    """The device-resident stretch-move sampler for every field of a `models.FieldSet` at once
    (`psfmc_stretch_run_fields`): each field is its own ensemble of `nwalkers` walkers with its own
    `RandomState` -- exactly the `DeviceEnsembleSampler` of that field alone -- but the half-step
    proposals of all fields are evaluated as ONE batch, so many small ensembles sample at the rate of one
    large one (BASELINE config 5 as a fit).  `fields[f]` is field f's emcee-style sampler object (`.chain`,
    `.lnprobability`, `.acceptance_fraction`, `.random_state`, ...).  A field's chain equals the chain its
    own one-field `DeviceEnsembleSampler` produces from the same start and random state, bit for bit.
    The reference fits one field per process (psfMC/fitting.py:13-113).
    Proposal moves are given with `set_moves(moves)`, not by keyword: every field then
    draws its own selector from its own generator -- in one iteration different fields may run different moves --
    and its chain equals its own `DeviceEnsembleSampler(moves=moves)` run.  The run goes through
    `psfmc_pt_move_run_fields` with one rung, beta = 1."""

    def __init__(self, nwalkers, fieldset, a=2.0, block=64, accumulate=False):
        if nwalkers % 2:
            raise ValueError('The number of walkers must be even.')
        if nwalkers * len(fieldset.models) > fieldset.max_walkers:
            raise ValueError('the FieldSet was built for at most {} walkers in all'.format(fieldset.max_walkers))
        self.fieldset = fieldset
        self.k, self.dim = int(nwalkers), fieldset.num_params
        self.block = int(block)
        self.accumulate = bool(accumulate)
        self.fields = [_FieldChain(nwalkers, m, a=a) for m in fieldset.models]

    def _draw(self, n_iter):
        """Every field's draws from its own generator, stacked by name: z, lz, partner, log_u [F, n_iter, 2, W/2]
        for `stretch_run`; with moves the shapes of `pt_move_run_fields` with one rung."""
        if self.fields[0]._moves is not None:
            return super(FieldSetSampler, self)._draw(n_iter, one_rung=True)
        per = [f._draw(n_iter) for f in self.fields]
        return (_Draws(**{name: np.ascontiguousarray([getattr(d, name) for d, _ in per])
                          for name in ('z', 'lz', 'partner', 'log_u')}), [s for _, s in per])

    def _run_one_rung(self, pos, lnp, draws, counters):
        """A block with moves: every field one rung at beta = 1, where lnp = 1 lnL + lnpi is the walker's
        log-posterior bit for bit; a walker enters as (lnL, lnpi) = (lnp, 0), the same sum."""
        n_f = len(self.fields)
        none = np.empty((len(draws.kind), n_f, 0, self.k))
        t_acc = np.ascontiguousarray(counters[:, np.newaxis, :])
        out = self.fieldset.context.pt_move_run_fields(
            np.ones(1), pos[:, np.newaxis], lnp[:, np.newaxis], np.zeros((n_f, 1, self.k)), *draws, none, none, none,
            naccepted=t_acc, nswap=np.zeros((n_f, 0), dtype=np.int64), store=True, accumulate=self.accumulate)
        counters[...] = t_acc[:, 0]
        return out[0][:, 0], out[4][:, :, -1].copy(), out[3][:, 0], out[4]

    def sample(self, p0, lnprob0=None, iterations=1, thin=1, storechain=True):
        """p0: [F, W, P] (or a list of [W, P]) start positions; lnprob0 likewise or None.  Yields, once per
        iteration, the list over fields of (pos, lnprob, rstate)."""
        n_f = len(self.fields)
        p = np.array([np.asarray(q, dtype=np.float64) for q in p0])
        lnprob = None if lnprob0 is None else np.array([np.asarray(q, dtype=np.float64) for q in lnprob0])
        lnprob = _check_start(p, lnprob, (n_f, self.k, self.dim),
                              lambda q: np.array(self.fieldset.log_posterior_batch(list(q))))
        i0 = [f._grow_storage(iterations, thin, storechain) for f in self.fields]
        nacc = np.ascontiguousarray([f.naccepted.astype(np.int64) for f in self.fields])

        def launch(draws):
            if draws.kind is not None:
                return self._run_one_rung(p, lnprob, draws, nacc)
            return self.fieldset.context.stretch_run(p, lnprob, *draws, nacc, store=True, accumulate=self.accumulate)

        for done, n, result, states in _run_blocks(iterations, self.block, self._draw, launch):
            p, lnprob, chain, lnchain = result
            for i, f in enumerate(self.fields):
                if self.accumulate:
                    f._count_accumulated(n * self.k)
                if storechain:
                    f._store_block(i0[i], done, n, thin, chain[i], lnchain[i])
                f.naccepted = nacc[i].astype(np.float64)
                f.iterations += n
            for j in range(n):
                yield [(chain[i][:, j, :].copy(), lnchain[i][:, j].copy(), states[i][j]) for i in range(n_f)]


# ---------------------------------------------------------------------------------------------------------------------
# Parallel tempering
# ---------------------------------------------------------------------------------------------------------------------
def default_betas(ntemps, tmax):
    """The default inverse-temperature ladder of `ntemps` rungs: ntemps - 1 geometric rungs from 1 down to
    1 / tmax, then beta = 0 (the prior, which the evidence needs).  ntemps = 1: (1,), plain sampling."""
    ntemps = int(ntemps)
    if ntemps < 1:
        raise ValueError('ntemps must be at least 1')
    if ntemps == 1:
        return np.ones(1)
    tmax = float(tmax)
    if not (np.isfinite(tmax) and tmax > 1.0):
        raise ValueError('tmax must be finite and greater than 1')
    betas = np.concatenate([np.geomspace(1.0, 1.0 / tmax, ntemps - 1), [0.0]])
    betas[0] = 1.0
    return betas


def check_betas(betas):
    """A user ladder as float64 [T], or ValueError: finite, beta_0 = 1, strictly decreasing, and (T > 1) the last
    rung 0 -- every device prior family is proper, so beta = 0 samples a proper prior."""
    b = np.array(betas, dtype=np.float64).ravel()
    if b.size < 1 or not np.all(np.isfinite(b)):
        raise ValueError('the temperature ladder must be a non-empty list of finite betas')
    if b[0] != 1.0:
        raise ValueError('the first rung of the ladder must be beta = 1')
    if np.any(np.diff(b) >= 0):
        raise ValueError('the ladder must be strictly decreasing')
    if b.size > 1 and b[-1] != 0.0:
        raise ValueError('the last rung of the ladder must be beta = 0 (the evidence needs the prior rung)')
    return b


def _tempered(beta, lnlike, lnprior):
    """beta lnL + lnpi -- that product, then that sum -- and -inf where lnL or lnpi is not finite."""
    with np.errstate(invalid='ignore', over='ignore'):
        v = beta * lnlike + lnprior
    return np.where(np.isfinite(lnlike) & np.isfinite(lnprior), v, -np.inf)


def _logsumexp(x):
    m = np.max(x)
    if not np.isfinite(m):
        return m
    return m + np.log(np.sum(np.exp(x - m)))


def _stepping_stone(betas, lnlike):
    """ln Z = sum_k [logsumexp((beta_k - beta_{k+1}) lnL^(k+1)) - ln N], lnlike [T, N] the samples of each rung."""
    total = 0.0
    for k in range(len(betas) - 1):
        x = (betas[k] - betas[k + 1]) * lnlike[k + 1]
        total += _logsumexp(x) - np.log(x.size)
    return total


class TemperedEnsembleSampler(_SamplerState):
    """Parallel-tempered stretch-move sampler: T copies of an ensemble of `nwalkers` walkers sample the tempered
    posteriors beta_t lnL + lnpi on the ladder `betas` (1 = beta_0 > ... > beta_{T-1} = 0), and neighbouring
    rungs swap walkers.  The stored lnL samples of every rung give the Bayesian evidence (`log_evidence`).

    This numpy implementation is the contract: `DeviceTemperedSampler` reproduces it bit for bit.  It is NOT a
    port of emcee 2's PTSampler (another z distribution and another split of the ensemble; emcee is not
    available here to pin anything against).  Per iteration:
      * the two half-steps of `EnsembleSampler.sample` (contiguous halves, h = 0 then 1); in each, for every rung
        t = 0 ... T-1 in turn: z = ((a-1) rand(half) + 1)^2 / a, partner = randint(half, size=half) (the same
        rung's other half), log_u = log(rand(half)); then ONE `like_prior_fn` call evaluates the T half proposals;
        accept where ((P-1) ln z + lnp_new) - lnp > log_u, lnp = beta_t lnL + lnpi;
        with `set_moves`: at the start of the iteration, when there is more than one move, ONE `rand()` selects
        (`EnsembleSampler._select_move`) the move of both half-steps of EVERY rung; in each half-step rung t then
        calls `move.draw(rs, half, P)` -> (scalar, Hastings term, a, b, ln u) in its move's own draw order and
        proposes `move.propose(s, c, scalar, a, b)`, partners from the same rung's other half; accept where
        (Hastings + lnp_new) - lnp > ln u.  No moves is `StretchMove(a)`, draw for draw;
      * swaps: for t = T-1 down to 1: i = permutation(W), j = permutation(W), log_u = log(rand(W)); pair k swaps
        walker i[k] of rung t with walker j[k] of rung t-1 when log_u[k] < (beta_{t-1} - beta_t) (lnL[t, i[k]] -
        lnL[t-1, j[k]]): positions, lnL and lnpi are exchanged, lnp recomputed at the new beta;
      * then storage.
    A walker whose lnpi or lnL is not finite has lnL = lnp = -inf at every beta.  With T = 1 (betas = (1,)) the
    chain is `EnsembleSampler`'s, bit for bit.

    like_prior_fn(theta [N, P]) -> (lnL [N], lnpi [N]), e.g. `model.log_likelihood_and_prior_batch`.
    Stored: `chain` [W, n, P] and `lnprobability` [W, n] of the beta = 1 rung (what `save_database` and
    `check_convergence_autocorr` read), `lnlikelihood` [T, W, n] of every rung; counters `naccepted_t` [T, W],
    `nswap` [T-1].  Proposal moves are given with `set_moves(moves)`, not by keyword;
    with T = 1 the chain is then `EnsembleSampler(moves=moves)`'s, bit for bit."""

    def __init__(self, nwalkers, dim, betas, like_prior_fn, a=2.0):
        if nwalkers % 2 or nwalkers < 2:
            raise ValueError('The number of walkers must be even.')
        self.k, self.dim, self.a = int(nwalkers), int(dim), float(a)
        self.betas = check_betas(betas)
        self.ntemps = len(self.betas)
        self.like_prior_fn = like_prior_fn
        self._random = np.random.mtrand.RandomState()
        self._moves = self._move_cum = None
        self.reset()

    def reset(self):
        self.iterations = 0
        self.naccepted_t = np.zeros((self.ntemps, self.k))
        self.nswap = np.zeros(max(self.ntemps - 1, 0))
        self._chain = np.empty((self.k, 0, self.dim))
        self._lnprob = np.empty((self.k, 0))
        self._lnlike = np.empty((self.ntemps, self.k, 0))

    clear_chain = reset

    @property
    def naccepted(self):
        return self.naccepted_t[0]

    @property
    def lnlikelihood(self):
        return self._lnlike

    @property
    def acceptance_fraction(self):
        return self.naccepted_t[0] / max(self.iterations, 1)

    @property
    def temperature_acceptance_fraction(self):
        return self.naccepted_t / max(self.iterations, 1)

    @property
    def tswap_acceptance_fraction(self):
        return self.nswap / (max(self.iterations, 1) * self.k)

    def log_evidence(self, fburnin=0.1):
        """(ln Z, err): the stepping-stone estimate from the stored lnL samples of every rung after the first
        `fburnin` of the stored iterations, ln Z = sum_k [logsumexp((beta_k - beta_{k+1}) lnL^(k+1)) - ln N];
        err = |ln Z - the same estimate on every other rung| (rungs 0, 2, 4, ... and always the beta = 0 one).
        Z is relative to the prior's normalisation over its support, the walkers' beta = 0 distribution."""
        if self.ntemps < 2:
            raise ValueError('the evidence needs a ladder of at least two rungs (beta = 1 ... beta = 0)')
        n = self._lnlike.shape[2]
        first = int(fburnin * n)
        if n - first < 1:
            raise ValueError('no stored samples after the burn-in')
        samples = self._lnlike[:, :, first:].reshape(self.ntemps, -1)
        lnz = _stepping_stone(self.betas, samples)
        coarse = list(range(0, self.ntemps, 2))
        if coarse[-1] != self.ntemps - 1:
            coarse.append(self.ntemps - 1)
        err = abs(lnz - _stepping_stone(self.betas[coarse], samples[coarse]))
        return lnz, err

    # -- state ----------------------------------------------------------------------------------------------------
    def _start(self, p0):
        p = np.array(p0, dtype=np.float64)
        if p.shape != (self.ntemps, self.k, self.dim):
            raise ValueError('p0 must have shape ({}, {}, {})'.format(self.ntemps, self.k, self.dim))
        if np.any(~np.isfinite(p)):
            raise ValueError('At least one parameter value was infinite or NaN.')
        return p

    def _like_prior(self, theta):
        ll, lp = self.like_prior_fn(theta)
        ll, lp = np.array(ll, dtype=np.float64), np.array(lp, dtype=np.float64)
        ll[~(np.isfinite(ll) & np.isfinite(lp))] = -np.inf
        return ll, lp

    def _grow_storage(self, iterations, thin, storechain):
        i0 = super(TemperedEnsembleSampler, self)._grow_storage(iterations, thin, storechain)
        if storechain:
            n_keep = int(iterations // thin)
            self._lnlike = np.concatenate((self._lnlike, np.zeros((self.ntemps, self.k, n_keep))), axis=2)
        return i0

    def sample(self, p0, lnlike0=None, lnprior0=None, rstate0=None, iterations=1, thin=1, storechain=True):
        """Generator: p0 [T, W, P] start positions (lnlike0 / lnprior0 [T, W] or None: evaluated); yields
        (pos [T, W, P], lnL [T, W], lnpi [T, W], rstate) after every iteration -- a state to resume from."""
        if rstate0 is not None:
            self.random_state = rstate0
        n_t, n_w, n_p = self.ntemps, self.k, self.dim
        p = self._start(p0)
        if lnlike0 is None or lnprior0 is None:
            ll, lp = self._like_prior(p.reshape(n_t * n_w, n_p))
            ll, lp = ll.reshape(n_t, n_w), lp.reshape(n_t, n_w)
        else:
            ll = np.array(lnlike0, dtype=np.float64).reshape(n_t, n_w)
            lp = np.array(lnprior0, dtype=np.float64).reshape(n_t, n_w)
            ll[~(np.isfinite(ll) & np.isfinite(lp))] = -np.inf
        beta = self.betas[:, None]
        lnp = _tempered(beta, ll, lp)
        i0 = self._grow_storage(iterations, thin, storechain)
        half = n_w // 2
        rs = self._random
        stretch = StretchMove(self.a)                   # no moves: the stretch move, draw for draw
        for i in range(int(iterations)):
            self.iterations += 1
            move = stretch if self._moves is None else self._moves[self._select_move()]
            for s0, s1 in ((slice(0, half), slice(half, n_w)), (slice(half, n_w), slice(0, half))):
                hastings = np.empty((n_t, half))
                lu = np.empty((n_t, half))
                q = np.empty((n_t, half, n_p))
                for t in range(n_t):
                    scal, hastings[t], a, b, lu[t] = move.draw(rs, half, n_p)
                    q[t] = move.propose(p[t, s0], p[t, s1], scal, a, b)
                nl, npri = self._like_prior(q.reshape(n_t * half, n_p))
                nl, npri = nl.reshape(n_t, half), npri.reshape(n_t, half)
                newlnp = _tempered(beta, nl, npri)
                with np.errstate(invalid='ignore'):
                    acc = hastings + newlnp - lnp[:, s0] > lu
                if np.any(acc):
                    p[:, s0][acc] = q[acc]
                    ll[:, s0][acc] = nl[acc]
                    lp[:, s0][acc] = npri[acc]
                    lnp[:, s0][acc] = newlnp[acc]
                    self.naccepted_t[:, s0][acc] += 1
            for t in range(n_t - 1, 0, -1):
                ii = rs.permutation(n_w)
                jj = rs.permutation(n_w)
                lu = np.log(rs.rand(n_w))
                with np.errstate(invalid='ignore'):
                    acc = lu < (self.betas[t - 1] - self.betas[t]) * (ll[t, ii] - ll[t - 1, jj])
                if np.any(acc):
                    a, b = ii[acc], jj[acc]
                    for arr in (p, ll, lp):
                        arr[t, a], arr[t - 1, b] = arr[t - 1, b].copy(), arr[t, a].copy()
                    lnp[t, a] = _tempered(self.betas[t], ll[t, a], lp[t, a])
                    lnp[t - 1, b] = _tempered(self.betas[t - 1], ll[t - 1, b], lp[t - 1, b])
                    self.nswap[t - 1] += int(np.count_nonzero(acc))
            if storechain and i % thin == 0:
                ind = i0 + int(i // thin)
                self._chain[:, ind, :] = p[0]
                self._lnprob[:, ind] = lnp[0]
                self._lnlike[:, :, ind] = ll
            yield p.copy(), ll.copy(), lp.copy(), self.random_state

    def run_mcmc(self, pos0, N, lnlike0=None, lnprior0=None, rstate0=None, **kwargs):
        results = None
        for results in self.sample(pos0, lnlike0, lnprior0, rstate0, iterations=N, **kwargs):
            pass
        return results


class DeviceTemperedSampler(_LadderMember, TemperedEnsembleSampler):
    """`TemperedEnsembleSampler` with every rung resident on the GPU (`psfmc_pt_run`): proposals of all T rungs
    in one launch per half-step, one pipeline pass over T W/2 records, the tempered accept, the swaps and the
    chain entries on the device.  The host draws the random numbers from the same `RandomState` in the same
    order (the next block while the GPU runs the current one), so both samplers produce the same chain bit for
    bit given lnL / lnpi as the device computes them (`model.log_likelihood_and_prior_batch`).  `block`
    iterations per library call; `sample()` yields once per iteration with a resumable state, while the counters
    and the stored chain advance a block at a time.

    The ladder is `betas`, or `default_betas(ntemps, tmax)`.  The defaults (ntemps=16, tmax=1e6) are argued in
    DESIGN.md section 13.  A one-field `MultiComponentModel` with every prior on the device, whose `max_walkers`
    must hold ntemps x nwalkers; or a `JointModel` of F fields (`psfmc_pt_run_joint`, DESIGN.md section 22: a
    walker is F field records, the likelihood the fields' sum), whose `max_walkers` must hold ntemps x nwalkers
    x F.  `accumulate`: posterior images of the beta = 1 rung after every iteration (every field's, for a joint
    fit).  Proposal moves are given with `set_moves(moves)`, not by keyword: the run then
    goes through `psfmc_pt_move_run` (`psfmc_pt_move_run_joint`), a proposal kernel by kind per half-step, and
    equals `TemperedEnsembleSampler` + `set_moves` bit for bit; `set_moves(None)` launches what it always did."""

    def __init__(self, nwalkers, model, ntemps=16, tmax=1e6, betas=None, a=2.0, block=64, accumulate=False):
        from .models import JointModel, MultiComponentModel
        from .engine import Context, JointView
        joint = isinstance(model, JointModel)
        if not joint and not isinstance(model, MultiComponentModel):
            raise ValueError('the tempered device sampler serves one-field MultiComponentModel fits and JointModel '
                             'fits; FieldSets and device groups are not supported')
        if betas is None:
            betas = default_betas(ntemps, tmax)
        super(DeviceTemperedSampler, self).__init__(nwalkers, model.num_params, betas,
                                                    model.log_likelihood_and_prior_batch, a=a)
        self.model = model
        self.block = int(block)
        self.accumulate = bool(accumulate)
        n_f = len(model.field_models) if joint else 1
        if joint and self.ntemps * self.k * n_f > model._max_walkers:
            raise ValueError('model was built for at most {} field records; {} temperatures x {} walkers x F={} fields '
                             'need more'.format(model._max_walkers, self.ntemps, self.k, n_f))
        if self.ntemps * self.k > model._max_walkers:
            raise ValueError('model was built for at most {} walkers; {} temperatures x {} walkers need more'
                             .format(model._max_walkers, self.ntemps, self.k))
        eng = model.engine
        if type(eng) is not (JointView if joint else Context):
            raise ValueError('the tempered device sampler serves one-field models and joint fits only')
        if model._host_priors:
            raise ValueError('priors {} are evaluated on the host: the tempered device sampler cannot be '
                             'used'.format([p.name for p, _ in model._host_priors]))

    def sample(self, p0, lnlike0=None, lnprior0=None, rstate0=None, iterations=1, thin=1, storechain=True):
        if rstate0 is not None:
            self.random_state = rstate0
        p = self._start(p0)
        ll = lp = None
        if lnlike0 is not None and lnprior0 is not None:
            ll, lp = np.array(lnlike0, dtype=np.float64), np.array(lnprior0, dtype=np.float64)
        i0 = self._grow_storage(iterations, thin, storechain)
        nacc = self.naccepted_t.astype(np.int64)
        nsw = self.nswap.astype(np.int64)
        eng = self.model.engine

        def launch(draws):
            run = eng.pt_run if draws.kind is None else eng.pt_move_run
            return run(self.betas, p, ll, lp, *draws, naccepted=nacc, nswap=nsw, store=True,
                       accumulate=self.accumulate)

        for done, n, result, states in _run_blocks(iterations, self.block, self._draw, launch):
            p, ll, lp, chain, lnchain, llchain, lpchain = result
            if self.accumulate:
                self._count_accumulated(n * self.k)
            if storechain:
                self._store_block(i0, done, n, thin, chain, lnchain, llchain)
            self.naccepted_t = nacc.astype(np.float64)
            self.nswap = nsw.astype(np.float64)
            self.iterations += n
            for j in range(n):
                yield chain[:, :, j, :].copy(), llchain[:, :, j].copy(), lpchain[:, :, j].copy(), states[j]


class _FieldLadder(_LadderMember, TemperedEnsembleSampler):
    """One field's share of a `FieldSetTemperedSampler`: the `TemperedEnsembleSampler` state of that field's
    ladder (chain, lnprobability, lnlikelihood, counters, random state, `log_evidence`) -- what `save_database`
    and `check_convergence_autocorr` read -- and its draws, `DeviceTemperedSampler`'s from its own generator."""

    def __init__(self, nwalkers, model, betas, a=2.0):
        super(_FieldLadder, self).__init__(nwalkers, model.num_params, betas,
                                           model.log_likelihood_and_prior_batch, a=a)
        self.model = model


class FieldSetTemperedSampler(_FieldMembers):
    """The parallel-tempered device sampler for every field of a `models.FieldSet` at once
    (`psfmc_pt_run_fields`): each field is its own ladder of T ensembles of `nwalkers` walkers with its own
    `RandomState` -- exactly the `DeviceTemperedSampler` of that field alone on its own context -- but the
    half-step proposals of all F T rungs are ONE batch of F T W/2 records, and the launches per iteration do not
    depend on F or T.  One ladder, `betas` or `default_betas(ntemps, tmax)`, serves every
    field.  `fields[f]` is field f's `TemperedEnsembleSampler`-style object (`.chain`, `.lnprobability`,
    `.lnlikelihood`, `.naccepted_t`, `.nswap`, `.random_state`, `.log_evidence()`, ...): its contents equal the
    field's own run from the same start, random state, ladder and block size bit for bit, so each field gets its
    own Bayesian evidence.  The set's `max_walkers` must hold F x ntemps x nwalkers.  `accumulate`: every
    field's posterior images of its beta = 1 rung after every iteration.
    Proposal moves are given with `set_moves(moves)`, not by keyword: every field then
    draws its own selector from its own generator, the run goes through `psfmc_pt_move_run_fields`, and a field's
    contents equal its own `DeviceTemperedSampler` + `set_moves` run."""

    def __init__(self, nwalkers, fieldset, ntemps=16, tmax=1e6, betas=None, a=2.0, block=64, accumulate=False):
        if nwalkers % 2 or nwalkers < 2:
            raise ValueError('The number of walkers must be even.')
        self.betas = check_betas(default_betas(ntemps, tmax) if betas is None else betas)
        self.ntemps = len(self.betas)
        n_f = len(fieldset.models)
        if n_f * self.ntemps * nwalkers > fieldset.max_walkers:
            raise ValueError('the FieldSet was built for at most {} walkers in all; {} fields x {} temperatures x {} '
                             'walkers need more'.format(fieldset.max_walkers, n_f, self.ntemps, nwalkers))
        self.fieldset = fieldset
        self.k, self.dim = int(nwalkers), fieldset.num_params
        self.block = int(block)
        self.accumulate = bool(accumulate)
        self.fields = [_FieldLadder(nwalkers, m, self.betas, a=a) for m in fieldset.models]

    def sample(self, p0, lnlike0=None, lnprior0=None, iterations=1, thin=1, storechain=True):
        """p0: [F, T, W, P] (or a list of [T, W, P]) start positions; lnlike0 / lnprior0 [F, T, W] or None
        (evaluated).  Yields, once per iteration, the list over fields of (pos [T, W, P], lnL [T, W],
        lnpi [T, W], rstate) -- field f's entry a state its ladder resumes from."""
        ctx = self.fieldset.context
        n_f = len(self.fields)
        p = np.array([f._start(q) for f, q in zip(self.fields, p0)]) if len(p0) == n_f else None
        if p is None:
            raise ValueError('p0 must have shape ({}, {}, {}, {})'.format(n_f, self.ntemps, self.k, self.dim))
        ll = lp = None
        if lnlike0 is not None and lnprior0 is not None:
            ll = np.array([np.asarray(q, dtype=np.float64) for q in lnlike0])
            lp = np.array([np.asarray(q, dtype=np.float64) for q in lnprior0])
        i0 = [f._grow_storage(iterations, thin, storechain) for f in self.fields]
        nacc = np.ascontiguousarray([f.naccepted_t.astype(np.int64) for f in self.fields])
        nsw = np.ascontiguousarray([f.nswap.astype(np.int64) for f in self.fields])

        def launch(draws):
            run = ctx.pt_run_fields if draws.kind is None else ctx.pt_move_run_fields
            return run(self.betas, p, ll, lp, *draws, naccepted=nacc, nswap=nsw, store=True,
                       accumulate=self.accumulate)

        for done, n, result, states in _run_blocks(iterations, self.block, self._draw, launch):
            p, ll, lp, chain, lnchain, llchain, lpchain = result
            for i, f in enumerate(self.fields):
                if self.accumulate:
                    f._count_accumulated(n * self.k)
                if storechain:
                    f._store_block(i0[i], done, n, thin, chain[i], lnchain[i], llchain[i])
                f.naccepted_t = nacc[i].astype(np.float64)
                f.nswap = nsw[i].astype(np.float64)
                f.iterations += n
            for j in range(n):
                yield [(chain[i, :, :, j, :].copy(), llchain[i, :, :, j].copy(), lpchain[i, :, :, j].copy(),
                        states[i][j]) for i in range(n_f)]

