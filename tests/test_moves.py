"""The host contract of the proposal moves (psfmc_amd/sampler.py `StretchMove`, `DEMove`, `EnsembleSampler(moves=)`):
the stretch move through the new keyword is today's sampler draw for draw, the DE proposal is the documented
expression in the documented draw order, both leave a Gaussian target stationary, and the selector costs one draw per
iteration of a mixture.  No GPU."""
import numpy as np
import pytest

from psfmc_amd.sampler import DEMove, EnsembleSampler, StretchMove, integrated_time, moves_label


def gauss(x):
    return -0.5 * np.sum(np.asarray(x) ** 2, axis=-1)


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def run(moves, n_w=12, dim=3, seed=5, n_iter=30, fn=gauss, **kw):
    s = EnsembleSampler(n_w, dim, batch_lnpostfn=fn, moves=moves, **kw)
    s.random_state = np.random.RandomState(seed).get_state()
    p0 = np.random.RandomState(seed + 1).normal(size=(n_w, dim))
    s.run_mcmc(p0, n_iter)
    return s


def todays_chain(n_w, dim, seed, n_iter, a=2.0):
    """emcee 2.2.1's loop written out (the sampler's own description: psfmc_amd/sampler.py's module docstring):
    (chain, naccepted, generator state)."""
    rs = np.random.RandomState(seed)
    p = np.random.RandomState(seed + 1).normal(size=(n_w, dim))
    lnp = gauss(p)
    half = n_w // 2
    chain, nacc = np.empty((n_w, n_iter, dim)), np.zeros(n_w)
    for i in range(n_iter):
        for s0, s1 in ((slice(half), slice(half, n_w)), (slice(half, n_w), slice(half))):
            s, c = p[s0], p[s1]
            zz = ((a - 1.0) * rs.rand(half) + 1) ** 2.0 / a
            rint = rs.randint(half, size=(half,))
            q = c[rint] - zz[:, np.newaxis] * (c[rint] - s)
            new = gauss(q)
            acc = (dim - 1.0) * np.log(zz) + new - lnp[s0] > np.log(rs.rand(half))
            lnp[s0][acc] = new[acc]
            p[s0][acc] = q[acc]
            nacc[s0][acc] += 1
        chain[:, i] = p
    return chain, nacc, rs.get_state()


def test_stretch_parity():
    """moves=None and moves=StretchMove() are today's sampler: chain, naccepted and the final generator state."""
    chain, nacc, state = todays_chain(12, 3, 5, 30)
    for moves in (None, StretchMove(), [(StretchMove(a=2.0), 3.0)]):
        s = run(moves)
        assert np.array_equal(s.chain, chain), moves
        assert np.array_equal(s.naccepted, nacc), moves
        assert same_state(s.random_state, state), moves
    assert nacc.sum() > 0
    # another `a`: the move's own, not the sampler's
    chain15, _, _ = todays_chain(12, 3, 5, 30, a=1.5)
    assert np.array_equal(run(StretchMove(a=1.5)).chain, chain15)
    assert np.array_equal(run(None, a=1.5).chain, chain15)
    assert not np.array_equal(chain15, chain)


@pytest.mark.parametrize('jump,sigma,gamma0', [(0.0, 1e-5, None), (0.3, 0.1, None), (1.0, 1e-5, None), (0.0, 0.2, 0.7)])
def test_de_proposal_formula(jump, sigma, gamma0):
    """One half-step of `DEMove` recomputed by hand from a second generator: the proposals agree bit for bit, a != b
    everywhere, and jump = 1 makes every g exactly 1."""
    n_w, dim, seed = 14, 4, 9
    half = n_w // 2
    seen = []

    def spy(x):
        seen.append(np.array(x))
        return gauss(x)

    s = EnsembleSampler(n_w, dim, batch_lnpostfn=spy, moves=DEMove(sigma=sigma, gamma0=gamma0, jump=jump),
                        live_dangerously=True)
    s.random_state = np.random.RandomState(seed).get_state()
    p0 = np.random.RandomState(seed + 1).normal(size=(n_w, dim))
    lnp0 = gauss(p0)
    pos, lnp, state = next(s.sample(p0, lnprob0=lnp0.copy(), iterations=1))[:3]
    assert len(seen) == 2
    rs = np.random.RandomState(seed)                       # no selector draw: one move
    p = p0.copy()
    cur = lnp0.copy()
    for h, q_seen in enumerate(seen):
        mine = slice(0, half) if h == 0 else slice(half, n_w)
        other = slice(half, n_w) if h == 0 else slice(0, half)
        u1 = rs.rand(half)
        sel = rs.rand(half)
        a = rs.randint(half, size=half)
        b = rs.randint(half - 1, size=half)
        b += (b >= a)
        log_u = np.log(rs.rand(half))
        assert np.all(a != b) and b.min() >= 0 and b.max() < half
        g0 = 2.38 / np.sqrt(2 * dim) if gamma0 is None else gamma0
        g = g0 * (1 + sigma * (2 * u1 - 1))
        g = np.where(sel < jump, 1.0, g)
        if jump == 1.0:
            assert np.all(g == 1.0)
        if jump == 0.0:
            assert np.all(g != 1.0) and np.all(np.abs(g / g0 - 1) <= sigma * (1 + 1e-12))
        s_, c_ = p[mine], p[other]
        q = np.empty((half, dim))
        for i in range(half):
            for d in range(dim):
                diff = c_[a[i], d] - c_[b[i], d]
                step = g[i] * diff
                q[i, d] = s_[i, d] + step
        assert np.array_equal(q, q_seen), h
        new = gauss(q)
        acc = new - cur[mine] > log_u
        p[mine] = np.where(acc[:, None], q, p[mine])
        cur[mine] = np.where(acc, new, cur[mine])
    assert np.array_equal(pos, p) and np.array_equal(lnp, cur)
    assert same_state(state, rs.get_state())


COV = np.array([[1.0, 0.6, 0.3, 0.0, -0.2],
                [0.6, 2.0, 0.5, 0.1, 0.0],
                [0.3, 0.5, 0.5, -0.1, 0.1],
                [0.0, 0.1, -0.1, 1.5, 0.4],
                [-0.2, 0.0, 0.1, 0.4, 0.8]])
ICOV = np.linalg.inv(COV)


def corr_gauss(x):
    x = np.asarray(x)
    return -0.5 * np.einsum('ni,ij,nj->n', x, ICOV, x)


@pytest.mark.parametrize('label', ['de_jump', 'mixture'])
def test_stationarity_on_a_correlated_gaussian(label):
    """5-dimensional correlated Gaussian, 32 walkers, 500 burn-in + 4000 kept iterations, a fixed seed: every mean
    within 5 standard errors of 0 and every variance within 5 relative standard errors of the truth, the standard
    errors from the chain's own integrated autocorrelation time (sqrt(var tau / n) and sqrt(2 tau / n), n the
    number of kept samples of all walkers): sampling theory, not tuned to the code."""
    moves = DEMove(jump=0.1) if label == 'de_jump' else [(StretchMove(), 1.0), (DEMove(), 1.0)]
    n_w, dim, burn, keep = 32, 5, 500, 4000
    assert np.all(np.linalg.eigvalsh(COV) > 0)
    s = EnsembleSampler(n_w, dim, batch_lnpostfn=corr_gauss, moves=moves)
    s.random_state = np.random.RandomState(123).get_state()
    p0 = np.random.RandomState(124).multivariate_normal(np.zeros(dim), COV, size=n_w)
    pos, lnp, _ = s.run_mcmc(p0, burn)
    s.reset()
    s.run_mcmc(pos, keep, lnprob0=lnp)
    chain = s.chain                                                    # [W, keep, dim]
    # of the ensemble mean, per parameter.  Window c = 5 (Sokal's lower bound, emcee 3's default): with 4000 kept
    # iterations the default c = 10 only reaches tau < 20, and the mixture's stretch half has a longer one
    tau = integrated_time(np.mean(chain, axis=0), axis=0, c=5)
    n = n_w * keep
    var_true = np.diag(COV)
    flat = chain.reshape(-1, dim)
    mean, var = flat.mean(axis=0), flat.var(axis=0)
    se_mean = np.sqrt(var_true * tau / n)
    se_var = np.sqrt(2.0 * tau / n)
    z_mean = np.abs(mean) / se_mean
    z_var = np.abs(var / var_true - 1.0) / se_var
    print('%s: tau %s, mean in standard errors %s, variance in relative standard errors %s, acceptance %.2f'
          % (label, np.round(tau, 1), np.round(z_mean, 2), np.round(z_var, 2), s.acceptance_fraction.mean()))
    assert np.all(tau >= 1.0) and np.all(tau < 200)
    assert np.all(z_mean <= 5.0), z_mean
    assert np.all(z_var <= 5.0), z_var
    assert 0.1 < s.acceptance_fraction.mean() < 0.9


def n_draws_between(state0, state1):
    """32-bit words the generator produced between two states of the same MT19937 stream (no reseed; fewer than
    one reload of 624 words, or whole reloads counted by replaying)."""
    rs = np.random.RandomState()
    rs.set_state(state0)
    for n in range(0, 200000):
        if same_state(rs.get_state(), state1):
            return n
        rs.randint(0, 2 ** 32, dtype=np.uint32)
    raise AssertionError('state not reached')


@pytest.mark.parametrize('first', [StretchMove(), DEMove(jump=0.2)])
def test_selector_draw(first):
    """Weights (1, 0): the mixture is the pure first move with ONE more `rand()` at the start of every iteration
    (a double: two 32-bit words), counted through the generator state; with one move no selector is drawn."""
    n_w, dim, seed, n_iter = 12, 3, 21, 8
    other = DEMove() if isinstance(first, StretchMove) else StretchMove()
    mix = run([(first, 1.0), (other, 0.0)], n_w, dim, seed, n_iter)
    # the pure move fed the same stream with one double skipped before every iteration
    pure = EnsembleSampler(n_w, dim, batch_lnpostfn=gauss, moves=first)
    rs = np.random.RandomState(seed)
    p = np.random.RandomState(seed + 1).normal(size=(n_w, dim))
    lnp, words = None, 0
    for it in range(n_iter):
        before = rs.get_state()
        rs.rand()
        after_selector = rs.get_state()
        assert n_draws_between(before, after_selector) == 2
        p, lnp, state = pure.run_mcmc(p, 1, rstate0=after_selector, lnprob0=lnp)
        p, lnp = p.copy(), lnp.copy()
        words += 2 + n_draws_between(after_selector, state)
        rs.set_state(state)
    assert np.array_equal(mix.chain, pure.chain)
    assert np.array_equal(mix.naccepted, pure.naccepted)
    assert same_state(mix.random_state, rs.get_state())
    # the whole run drew what the pure iterations drew plus two words (one double) per iteration
    start = np.random.RandomState(seed).get_state()
    assert n_draws_between(start, mix.random_state) == words
    # a single move draws no selector (test_stretch_parity and test_de_proposal_formula hold its generator state to
    # a replay without one): from the same seed its chain is another one
    assert not np.array_equal(run(first, n_w, dim, seed, n_iter).chain, mix.chain)
    # ... and the weights do select: (0, 1) is the pure second move behind the same selector draws
    swapped = run([(first, 0.0), (other, 1.0)], n_w, dim, seed, n_iter)
    assert not np.array_equal(swapped.chain, mix.chain)


def test_both_moves_of_a_mixture_occur():
    """Half and half over 40 iterations: the per-iteration choice follows the selector draw (r < 0.5: the first)."""
    n_w, dim, seed, n_iter = 12, 3, 33, 40
    calls = []

    class Tell(StretchMove):
        def draw(self, rs, half, dim):
            calls.append('s')
            return StretchMove.draw(self, rs, half, dim)

    class TellDE(DEMove):
        def draw(self, rs, half, dim):
            calls.append('d')
            return DEMove.draw(self, rs, half, dim)

    run([(Tell(), 1.0), (TellDE(), 1.0)], n_w, dim, seed, n_iter)
    assert len(calls) == 2 * n_iter and calls[0::2] == calls[1::2]        # one move per iteration, both half-steps
    assert 5 < calls.count('s') // 2 < 35


def test_errors():
    with pytest.raises(ValueError, match='4 walkers'):
        EnsembleSampler(2, 1, batch_lnpostfn=gauss, moves=DEMove())
    with pytest.raises(ValueError, match='4 walkers'):
        EnsembleSampler(2, 1, batch_lnpostfn=gauss, moves=[(StretchMove(), 1.0), (DEMove(), 1.0)])
    EnsembleSampler(2, 1, batch_lnpostfn=gauss, moves=StretchMove())           # the stretch move needs no more
    for weights in ((1.0, -1.0), (0.0, 0.0), (np.nan, 1.0), (np.inf, 1.0)):
        with pytest.raises(ValueError, match='weights'):
            EnsembleSampler(8, 2, batch_lnpostfn=gauss, moves=[(StretchMove(), weights[0]), (DEMove(), weights[1])])
    with pytest.raises(ValueError):
        EnsembleSampler(8, 2, batch_lnpostfn=gauss, moves=[])
    with pytest.raises(ValueError):
        EnsembleSampler(8, 2, batch_lnpostfn=gauss, moves='de')
    with pytest.raises(ValueError):
        DEMove(jump=1.5)


def test_samplers_without_the_keyword():
    """`FieldSetSampler`, `DeviceTemperedSampler` and `TemperedEnsembleSampler` do not take `moves` (their docstrings
    say so): the keyword is refused before anything else is looked at."""
    from psfmc_amd.sampler import DeviceTemperedSampler, FieldSetSampler, TemperedEnsembleSampler
    with pytest.raises(TypeError, match='moves'):
        FieldSetSampler(8, None, moves=DEMove())
    with pytest.raises(TypeError, match='moves'):
        DeviceTemperedSampler(8, None, moves=DEMove())
    with pytest.raises(TypeError, match='moves'):
        TemperedEnsembleSampler(8, 2, (1.0,), None, moves=DEMove())
    for cls in (FieldSetSampler, DeviceTemperedSampler, TemperedEnsembleSampler):
        assert 'moves' in cls.__doc__


def test_fitting_refuses_a_sampler_class_without_the_keyword():
    """`model_galaxy_mcmc(moves=..., sampler_class=<no such keyword>)` is a ValueError, raised before the class is
    constructed or a context is made."""
    from psfmc_amd import fitting

    class Plain(object):
        def __init__(self, nwalkers, dim, lnpostfn, kwargs=None, pool=None):
            raise AssertionError('constructed')

    class Model(fitting.MultiComponentModel):
        def __init__(self):
            self._device, self._max_walkers, self._num_params, self._engine = 0, 64, 3, None

    with pytest.raises(ValueError, match='moves'):
        fitting.model_galaxy_mcmc(Model(), output_name='unused', chains=8, sampler_class=Plain, moves=DEMove(),
                                  group=None, quiet=True)
    assert fitting._takes_moves(EnsembleSampler) and not fitting._takes_moves(Plain)


def test_moves_label():
    assert moves_label(None) is None
    assert moves_label(DEMove()) == 'de:1'
    assert moves_label([(StretchMove(), 0.5), (DEMove(), 0.5)]) == 'stretch:0.5,de:0.5'
    assert moves_label([(StretchMove(), 3), (DEMove(), 1)]) == 'stretch:0.75,de:0.25'
