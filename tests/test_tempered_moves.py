"""The host contract of the proposal moves on tempered ladders and field sets (psfmc_amd/sampler.py `set_moves`):
the stretch move through `set_moves` is the untouched sampler draw for draw, one rung with moves is
`EnsembleSampler(moves=)`, a DE half-step over three rungs is the documented expression in the documented rung and
draw order, the selector costs one draw per iteration for the whole ladder, a yielded state resumes, every sampler
class parses its moves alike, and the evidence of a Gaussian in a box survives the mixture.  No GPU."""
import numpy as np
import pytest

from psfmc_amd.sampler import (DEMove, DeviceEnsembleSampler, DeviceTemperedSampler, EnsembleSampler,
                               FieldSetSampler, FieldSetTemperedSampler, StretchMove, TemperedEnsembleSampler,
                               default_betas)
from test_moves import n_draws_between, same_state
from test_tempered import gaussian_in_box


def mixture(jump=0.1):
    return [(StretchMove(), .5), (DEMove(jump=jump), .5)]


def ladder(moves, n_t=4, n_w=8, dim=2, seed=9, n_iter=20, set_it=True, **kw):
    fn, _ = gaussian_in_box(dim)
    s = TemperedEnsembleSampler(n_w, dim, default_betas(n_t, 50.0), fn, **kw)
    if set_it:
        s.set_moves(moves)
    s.random_state = np.random.RandomState(seed).get_state()
    p0 = np.random.RandomState(seed + 1).uniform(-5, 5, (n_t, n_w, dim))
    return s, list(s.sample(p0, iterations=n_iter))


def same_run(a, b):
    return (np.array_equal(a.chain, b.chain) and np.array_equal(a.lnprobability, b.lnprobability) and
            np.array_equal(a.lnlikelihood, b.lnlikelihood) and np.array_equal(a.naccepted_t, b.naccepted_t) and
            np.array_equal(a.nswap, b.nswap) and same_state(a.random_state, b.random_state))


def test_stretch_through_set_moves_is_the_untouched_sampler():
    plain, _ = ladder(None, set_it=False)
    assert plain.naccepted_t.sum() > 0 and plain.nswap.sum() > 0
    for moves in (StretchMove(), [(StretchMove(a=2.0), 3.0)], None):
        s, _ = ladder(moves)
        assert same_run(s, plain), moves
    # another `a`: the move's own, not the sampler's; and set_moves(None) after moves restores the sampler's
    other, _ = ladder(None, set_it=False, a=1.5)
    assert not np.array_equal(other.chain, plain.chain)
    assert same_run(ladder(StretchMove(a=1.5))[0], other)
    back = TemperedEnsembleSampler(8, 2, default_betas(4, 50.0), gaussian_in_box(2)[0])
    back.set_moves(DEMove())
    back.set_moves(None)
    back.random_state = np.random.RandomState(9).get_state()
    list(back.sample(np.random.RandomState(10).uniform(-5, 5, (4, 8, 2)), iterations=20))
    assert same_run(back, plain)


def test_one_rung_with_a_mixture_is_the_ensemble_sampler():
    fn, _ = gaussian_in_box(3)
    p0 = np.random.RandomState(5).uniform(-2, 2, (10, 3))
    host = EnsembleSampler(10, 3, batch_lnpostfn=lambda x: np.add(*fn(x)), moves=mixture(0.2))
    temp = TemperedEnsembleSampler(10, 3, [1.0], fn)
    temp.set_moves(mixture(0.2))
    for s in (host, temp):
        s.random_state = np.random.RandomState(17).get_state()
    list(host.sample(p0, iterations=30))
    list(temp.sample(p0[None], iterations=30))
    assert np.array_equal(temp.chain, host.chain)
    assert np.array_equal(temp.lnprobability, host.lnprobability)
    assert np.array_equal(temp.naccepted, host.naccepted) and host.naccepted.sum() > 0
    assert same_state(temp.random_state, host.random_state)
    # ... and EnsembleSampler.set_moves is its keyword
    late = EnsembleSampler(10, 3, batch_lnpostfn=lambda x: np.add(*fn(x)))
    late.set_moves(mixture(0.2))
    late.random_state = np.random.RandomState(17).get_state()
    list(late.sample(p0, iterations=30))
    assert np.array_equal(late.chain, host.chain) and same_state(late.random_state, host.random_state)


def test_a_de_half_step_over_three_rungs_by_hand():
    """T = 3, 8 walkers, P = 2, pure DEMove(jump = 0.3, sigma = 0.1): the first half-step's proposals of the three
    rungs recomputed from a second generator -- no selector draw, then rung 0, 1, 2 in turn, each in DEMove's draw
    order, partners from the same rung's other half, three roundings -- and their acceptance."""
    n_t, n_w, dim, seed = 3, 8, 2, 13
    half = n_w // 2
    betas = default_betas(n_t, 20.0)
    fn, _ = gaussian_in_box(dim)
    seen = []

    def spy(x):
        seen.append(np.array(x))
        return fn(x)

    s = TemperedEnsembleSampler(n_w, dim, betas, spy)
    s.set_moves(DEMove(sigma=0.1, jump=0.3))
    s.random_state = np.random.RandomState(seed).get_state()
    p0 = np.random.RandomState(seed + 1).uniform(-3, 3, (n_t, n_w, dim))
    ll0, lp0 = (v.reshape(n_t, n_w) for v in fn(p0.reshape(-1, dim)))
    next(s.sample(p0, lnlike0=ll0, lnprior0=lp0, iterations=1))
    assert [len(q) for q in seen] == [n_t * half, n_t * half]        # ONE call per half-step
    rs = np.random.RandomState(seed)
    p, ll, lp = p0.copy(), ll0.copy(), lp0.copy()
    nacc = np.zeros((n_t, n_w))
    for h, (mine, oth) in enumerate(((slice(0, half), slice(half, n_w)), (slice(half, n_w), slice(0, half)))):
        q = np.empty((n_t, half, dim))
        lu = np.empty((n_t, half))
        for t in range(n_t):
            u1, sel = rs.rand(half), rs.rand(half)
            a = rs.randint(half, size=half)
            b = rs.randint(half - 1, size=half)
            b += (b >= a)
            lu[t] = np.log(rs.rand(half))
            assert np.all(a != b)
            g = 2.38 / np.sqrt(2 * dim) * (1 + 0.1 * (2 * u1 - 1))
            g = np.where(sel < 0.3, 1.0, g)
            own, other = p[t, mine], p[t, oth]
            for i in range(half):
                for d in range(dim):
                    diff = other[a[i], d] - other[b[i], d]
                    step = g[i] * diff
                    q[t, i, d] = own[i, d] + step
        assert np.array_equal(seen[h], q.reshape(-1, dim)), h
        nl, npri = (v.reshape(n_t, half) for v in fn(q.reshape(-1, dim)))
        ok = np.isfinite(nl) & np.isfinite(npri)
        with np.errstate(invalid='ignore'):
            new = np.where(ok, betas[:, None] * nl + npri, -np.inf)
            old = betas[:, None] * ll[:, mine] + lp[:, mine]
            acc = new - old > lu                                      # no Hastings term
        assert 0 < acc.sum() < acc.size
        p[:, mine] = np.where(acc[:, :, None], q, p[:, mine])         # the second half-step proposes from this
        ll[:, mine] = np.where(acc, nl, ll[:, mine])
        lp[:, mine] = np.where(acc, npri, lp[:, mine])
        nacc[:, mine] += acc
    assert np.array_equal(s.naccepted_t, nacc)


def test_one_selector_draw_per_iteration_for_the_whole_ladder():
    """Weights (1, 0): the mixture is the pure first move with ONE more `rand()` (two 32-bit words) at the start of
    every iteration, whatever the number of rungs; with one move no selector is drawn."""
    n_iter = 6
    mix, out = ladder([(DEMove(jump=0.2), 1.0), (StretchMove(), 0.0)], n_iter=n_iter)
    fn, _ = gaussian_in_box(2)
    pure = TemperedEnsembleSampler(8, 2, default_betas(4, 50.0), fn)
    pure.set_moves(DEMove(jump=0.2))
    rs = np.random.RandomState(9)
    state = (np.random.RandomState(10).uniform(-5, 5, (4, 8, 2)), None, None)
    words = 0
    for it in range(n_iter):
        before = rs.get_state()
        rs.rand()
        after = rs.get_state()
        assert n_draws_between(before, after) == 2
        pos, ll, lp, rstate = pure.run_mcmc(state[0], 1, state[1], state[2], rstate0=after)
        state = (pos, ll, lp)
        words += 2 + n_draws_between(after, rstate)
        rs.set_state(rstate)
        assert same_state(out[it][3], rstate), it
    assert np.array_equal(mix.chain, pure.chain) and np.array_equal(mix.nswap, pure.nswap)
    assert n_draws_between(np.random.RandomState(9).get_state(), mix.random_state) == words
    assert not np.array_equal(ladder(DEMove(jump=0.2), n_iter=n_iter)[0].chain, mix.chain)


def test_both_moves_of_a_mixture_occur_on_every_rung_alike():
    calls = []

    class Tell(StretchMove):
        def draw(self, rs, half, dim):
            calls.append('s')
            return StretchMove.draw(self, rs, half, dim)

    class TellDE(DEMove):
        def draw(self, rs, half, dim):
            calls.append('d')
            return DEMove.draw(self, rs, half, dim)

    ladder([(Tell(), 1.0), (TellDE(), 1.0)], n_t=3, n_iter=40)
    per_iter = [calls[i:i + 6] for i in range(0, len(calls), 6)]      # 2 half-steps x 3 rungs
    assert len(per_iter) == 40 and all(len(set(c)) == 1 for c in per_iter)
    assert 5 < sum(c[0] == 's' for c in per_iter) < 35


def test_resume_from_a_yielded_state_with_moves():
    full, out = ladder(mixture(), n_iter=20)
    pos, ll, lp, rstate = out[6]
    fn, _ = gaussian_in_box(2)
    again = TemperedEnsembleSampler(8, 2, default_betas(4, 50.0), fn)
    again.set_moves(mixture())
    list(again.sample(pos, lnlike0=ll, lnprior0=lp, rstate0=rstate, iterations=13))
    assert np.array_equal(again.chain, full.chain[:, 7:])
    assert np.array_equal(again.lnlikelihood, full.lnlikelihood[:, :, 7:])
    assert same_state(again.random_state, full.random_state)
    # moves set between two sample() calls take effect from the next iteration on
    two = TemperedEnsembleSampler(8, 2, default_betas(4, 50.0), fn)
    two.random_state = np.random.RandomState(9).get_state()
    first = list(two.sample(np.random.RandomState(10).uniform(-5, 5, (4, 8, 2)), iterations=5))[-1]
    plain, _ = ladder(None, n_iter=5, set_it=False)
    assert np.array_equal(two.chain, plain.chain)
    two.set_moves(DEMove())
    list(two.sample(*first[:3], iterations=5))
    assert two.chain.shape[1] == 10 and two.naccepted_t.sum() > plain.naccepted_t.sum()


class _Field(object):
    """What `_FieldChain` / `_FieldLadder` read of a model, without a GPU."""

    def __init__(self, dim):
        self.num_params = dim

    def log_posterior_batch(self, x):
        return np.add(*gaussian_in_box(self.num_params)[0](x))

    def log_likelihood_and_prior_batch(self, x):
        return gaussian_in_box(self.num_params)[0](x)


class _Set(object):
    def __init__(self, dim):
        self.models, self.max_walkers, self.num_params = [_Field(dim), _Field(dim)], 1024, dim


def _samplers(n_w, dim):
    fn, _ = gaussian_in_box(dim)
    return [EnsembleSampler(n_w, dim, batch_lnpostfn=lambda x: np.add(*fn(x))),
            TemperedEnsembleSampler(n_w, dim, [1.0, 0.0], fn),
            FieldSetSampler(n_w, _Set(dim)),
            FieldSetTemperedSampler(n_w, _Set(dim), betas=[1.0, 0.0])]


def test_set_moves_on_every_sampler_class():
    for s in _samplers(8, 2):
        for weights in ((1.0, -1.0), (0.0, 0.0), (np.nan, 1.0), (np.inf, 1.0)):
            with pytest.raises(ValueError, match='weights'):
                s.set_moves([(StretchMove(), weights[0]), (DEMove(), weights[1])])
        for bad in ([], 'de'):
            with pytest.raises(ValueError):
                s.set_moves(bad)
        s.set_moves(mixture())
        members = getattr(s, 'fields', [s])
        assert all(len(m._moves) == 2 and m._move_cum[-1] == 1.0 for m in members)
        s.set_moves(None)
        assert all(m._moves is None for m in members)
    for s in _samplers(2, 1):                # DE needs two distinct partners in each half: 4 walkers per ensemble
        with pytest.raises(ValueError, match='4 walkers'):
            s.set_moves(DEMove())
        with pytest.raises(ValueError, match='4 walkers'):
            s.set_moves(mixture())
        s.set_moves(StretchMove())
    # the device samplers have the method of their host classes (exercised in tests/test_gpu_tempered_moves.py)
    assert DeviceTemperedSampler.set_moves is TemperedEnsembleSampler.set_moves
    assert callable(DeviceEnsembleSampler.set_moves)


# Calibrated on this host as tests/test_tempered.py's floors were (4 seeds each -- d, d + 100, d + 200, d + 300 --
# 25 % burn-in, the half-and-half mixture): the largest |lnZ - exact| was 0.061 at d = 2 (0.061, 0.038, 0.047,
# 0.007) and 0.063 at d = 11 (0.006, 0.036, 0.001, 0.063), while `err` was 0.002 ... 0.034; the floors are about
# 2.5 x the largest deviation seen.
@pytest.mark.parametrize('d, walkers, ntemps, tmax, iterations, floor', [
    (2, 16, 8, 100.0, 400, 0.15),
    (11, 32, 12, 300.0, 600, 0.16),
])
def test_evidence_of_a_gaussian_in_a_box_with_the_mixture(d, walkers, ntemps, tmax, iterations, floor):
    fn, exact = gaussian_in_box(d)
    rs = np.random.RandomState(d)
    s = TemperedEnsembleSampler(walkers, d, default_betas(ntemps, tmax), fn)
    s.set_moves([(StretchMove(), .5), (DEMove(jump=0.1), .5)])
    s.random_state = rs.get_state()
    for _ in s.sample(rs.uniform(-5, 5, (ntemps, walkers, d)), iterations=iterations):
        pass
    lnz, err = s.log_evidence(0.25)
    print('d = %d: lnZ %.4f exact %.4f err %.4f' % (d, lnz, exact, err))
    assert abs(lnz - exact) <= max(3 * err, floor), (lnz, exact, err)
    assert np.all(s.tswap_acceptance_fraction > 0.2)
