"""The block edges of the four device samplers: a `thin` that does not divide `block` and a `block` that does not
divide `iterations` (18 iterations in blocks of 7, 7 and 4, every third kept: the kept positions of the three blocks
start at 0, 2 and 1), with `accumulate=True`, with and without `set_moves`.  Every run is held with `array_equal`
to the host contract -- `EnsembleSampler` / `TemperedEnsembleSampler` fed the device's own evaluation -- in the
stored arrays, the counters, every yield and every yielded generator state, and resumes from the yield of
iteration 9, inside the second block.  W = 22 (a half of 11), T = 3; one 64^2 field, and 64^2 beside 96^2 for
the sets (point source + one Sersic, as tests/test_gpu_mixed_fields.py builds them).

18 iterations, not 20: the contract, like emcee 2, makes room for `iterations // thin` kept iterations and stores
iteration i where `i % thin == 0`, so a `thin` that does not divide `iterations` ends in an IndexError on the host
and in a shape error on the device, before and after this file.  18 = 2 x 7 + 4 crosses the same edges, and the
resumed 9 iterations divide by 3 as well.  The other files of the suite cover blocks that do not divide the
iterations (without `thin`) on every sampler; `thin` ran on a device sampler only in tests/test_gpu_fitting.py,
inside one block."""
import numpy as np
import pytest

import test_gpu_mixed_fields as mixed
from test_gpu_fields_tempered import _same_state
from psfmc_amd.sampler import (DEMove, DeviceEnsembleSampler, DeviceTemperedSampler, EnsembleSampler, StretchMove,
                               TemperedEnsembleSampler, default_betas)

pytestmark = pytest.mark.gpu

N_W, N_T, N_ITER, BLOCK, THIN, STOP = 22, 3, 18, 7, 3, 9
SHAPES = [(64, 64, 11), (96, 96, 13)]
BETAS = default_betas(N_T, 50.0)
MOVES = [None, 'mixture']


def _moves(which):
    return None if which is None else [(StretchMove(), .5), (DEMove(jump=0.2), .5)]


def _start(fld, n_t, seed):
    p = fld['truth'] + np.random.RandomState(seed).normal(size=(n_t, N_W, len(fld['truth']))) * 1e-3
    p[:, :, 10] = np.arange(N_W) % 2
    return p


@pytest.fixture(scope='module')
def fields():
    return [mixed._field(ny, nx, pk, seed=30 + f) for f, (ny, nx, pk) in enumerate(SHAPES)]


@pytest.fixture(scope='module')
def one(fields):
    model = mixed._model(fields[0], N_T * N_W)
    yield model
    model.close()


@pytest.fixture(scope='module')
def both(fields):
    from psfmc_amd import FieldSet
    fs = FieldSet([mixed._model(fld, 1) for fld in fields], max_walkers=len(fields) * N_T * N_W)
    yield fs
    fs.close()


def _copies(yields):
    """The yields of a `sample()` as they were when yielded (the host samplers yield their live arrays)."""
    return [tuple(np.copy(v) if isinstance(v, np.ndarray) else v for v in y) for y in yields]


def _host(ladder, dim, evaluate, which, seed):
    if ladder:
        host = TemperedEnsembleSampler(N_W, dim, BETAS, evaluate)
        host.set_moves(_moves(which))
    else:
        host = EnsembleSampler(N_W, dim, batch_lnpostfn=evaluate, moves=_moves(which))
    host.random_state = np.random.RandomState(seed).get_state()
    return host


def _assert_member(dev, host, got, want, ladder, f):
    """One device ensemble or ladder (a sampler, or a set's member) and its yields against the contract's."""
    n_arrays = 3 if ladder else 2
    assert dev.chain.shape == (N_W, N_ITER // THIN, dev.dim)         # iterations 0, 3, ..., 15
    assert np.array_equal(dev.chain, host.chain), f
    assert np.array_equal(dev.lnprobability, host.lnprobability), f
    assert dev.iterations == host.iterations == N_ITER, f
    if ladder:
        assert np.array_equal(dev.lnlikelihood, host.lnlikelihood), f
        assert np.array_equal(dev.naccepted_t, host.naccepted_t) and np.array_equal(dev.nswap, host.nswap), f
        assert host.nswap.sum() > 0, f
    else:
        assert np.array_equal(dev.naccepted, host.naccepted), f
    assert 0 < host.naccepted.sum() < N_W * N_ITER, f
    assert len(got) == len(want) == N_ITER, f
    for j, (a, b) in enumerate(zip(got, want)):
        for k in range(n_arrays):
            assert np.array_equal(a[k], b[k]), (f, j, k)
        assert _same_state(a[n_arrays], b[n_arrays]), (f, j)


def _assert_same_end(rest, full, ladder, f):
    n_arrays = 3 if ladder else 2
    assert len(rest) == N_ITER - STOP
    for k in range(n_arrays):
        assert np.array_equal(rest[-1][k], full[-1][k]), (f, k)
    assert _same_state(rest[-1][n_arrays], full[-1][n_arrays]), f


@pytest.mark.parametrize('which', MOVES)
@pytest.mark.parametrize('ladder', [False, True])
def test_one_field(one, fields, ladder, which):
    dim = one.num_params
    p0 = _start(fields[0], N_T if ladder else 1, seed=70)
    p0 = p0 if ladder else p0[0]

    def device():
        if ladder:
            dev = DeviceTemperedSampler(N_W, one, betas=BETAS, block=BLOCK, accumulate=True)
            dev.set_moves(_moves(which))
            return dev
        return DeviceEnsembleSampler(N_W, one, block=BLOCK, accumulate=True, moves=_moves(which))

    host = _host(ladder, dim, one.log_likelihood_and_prior_batch if ladder else one.log_posterior_batch, which, 600)
    want = _copies(host.sample(p0, iterations=N_ITER, thin=THIN))
    one.reset_images()
    dev = device()
    dev.random_state = np.random.RandomState(600).get_state()
    got = _copies(dev.sample(p0, iterations=N_ITER, thin=THIN))
    assert one.accumulated_samples == N_ITER * N_W
    _assert_member(dev, host, got, want, ladder, 0)
    at = got[STOP - 1]
    again = device()
    rest = _copies(again.sample(*at[:-1], rstate0=at[-1], iterations=N_ITER - STOP, thin=THIN))
    _assert_same_end(rest, got, ladder, 0)
    assert again.chain.shape[1] == (N_ITER - STOP) // THIN and again.iterations == N_ITER - STOP
    one.reset_images()


@pytest.mark.parametrize('which', MOVES)
@pytest.mark.parametrize('ladder', [False, True])
def test_two_fields_of_different_size(both, fields, ladder, which):
    from psfmc_amd import FieldSetSampler, FieldSetTemperedSampler
    n_f = len(fields)
    p0 = [_start(fld, N_T if ladder else 1, seed=70 + f) for f, fld in enumerate(fields)]
    p0 = p0 if ladder else [p[0] for p in p0]

    def device(states):
        if ladder:
            dev = FieldSetTemperedSampler(N_W, both, betas=BETAS, block=BLOCK, accumulate=True)
        else:
            dev = FieldSetSampler(N_W, both, block=BLOCK, accumulate=True)
        dev.set_moves(_moves(which))
        for sub, state in zip(dev.fields, states):
            sub.random_state = state
        return dev

    for m in both.models:
        m.reset_images()
    dev = device([np.random.RandomState(600 + f).get_state() for f in range(n_f)])
    got = [_copies(y) for y in dev.sample(p0, iterations=N_ITER, thin=THIN)]
    for f in range(n_f):
        member = both.models[f]
        assert member.accumulated_samples == N_ITER * N_W, f
        host = _host(ladder, both.num_params,
                     member.log_likelihood_and_prior_batch if ladder else member.log_posterior_batch, which, 600 + f)
        want = _copies(host.sample(p0[f], iterations=N_ITER, thin=THIN))
        _assert_member(dev.fields[f], host, [y[f] for y in got], want, ladder, f)
    at = got[STOP - 1]
    again = device([y[-1] for y in at])
    start = [[y[k] for y in at] for k in range(3 if ladder else 2)]
    rest = [_copies(y) for y in again.sample(*start, iterations=N_ITER - STOP, thin=THIN)]
    for f in range(n_f):
        _assert_same_end([y[f] for y in rest], [y[f] for y in got], ladder, f)
        assert again.fields[f].iterations == N_ITER - STOP
    for m in both.models:
        m.reset_images()
