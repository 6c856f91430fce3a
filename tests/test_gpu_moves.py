"""The proposal moves on the device (psfmc_move_run, psfmc_stretch_set_moves, psfmc_move_run_joint; k_move_propose)
against the host contract `EnsembleSampler(batch_lnpostfn=model.log_posterior_batch, moves=...)`: the same
`RandomState`, the same draw order, the same chain bit for bit."""
import os
import shutil

import numpy as np
import pytest

import helpers
from psfmc_amd.engine import NativeError, _move_run
from psfmc_amd.sampler import DEMove, DeviceEnsembleSampler, EnsembleSampler, StretchMove

pytestmark = pytest.mark.gpu

EINVAL = -1                 # include/psfmc_hip.h PSFMC_EINVAL


def mixture():
    return [(StretchMove(), 1), (DEMove(), 1)]


def telling(moves):
    """The same moves for the host sampler, telling which one every iteration drew from: (moves, kinds)."""
    kinds = []

    def wrap(move):
        class Tell(type(move)):
            def draw(self, rs, half, dim):
                kinds.append(self.kind)
                return type(move).draw(self, rs, half, dim)
        tell = Tell.__new__(Tell)
        tell.__dict__.update(move.__dict__)
        return tell
    pairs = [(moves, 1.0)] if hasattr(moves, 'draw') else moves
    return [(wrap(m), w) for m, w in pairs], kinds


def pair(n_w, model, moves, seed, fn=None, **dev_kw):
    """(host, device) samplers on the same generator state; the host's evaluations are the device's own."""
    host_moves, kinds = telling(moves)
    host = EnsembleSampler(n_w, model.num_params, batch_lnpostfn=fn or model.log_posterior_batch, moves=host_moves,
                           live_dangerously=True)
    dev = DeviceEnsembleSampler(n_w, model, moves=moves, live_dangerously=True, **dev_kw)
    for s in (host, dev):
        s.random_state = np.random.RandomState(seed).get_state()
    return host, dev, kinds


def same_chain(dev, host, exact_lnp=True):
    assert np.array_equal(dev.chain, host.chain)
    assert np.array_equal(dev.naccepted, host.naccepted)
    if exact_lnp:
        assert np.array_equal(dev.lnprobability, host.lnprobability)
    else:
        assert helpers.rel_err(dev.lnprobability, host.lnprobability) <= 1e-13


def tight_start(model, case, n_w, seed):
    """n_w walkers in a small ball round the fixture's best walker: proposals of either move stay reasonable."""
    ok = np.isfinite(case['lnprob'])
    best = case['params'][ok][np.argmax(case['lnprob'][ok])]
    p0 = best * (1.0 + 1e-4 * np.random.RandomState(seed).normal(size=(n_w, len(best))))
    assert np.all(np.isfinite(model.log_posterior_batch(p0)))
    return p0


@pytest.fixture(scope='module')
def synth(tmp_path_factory):
    case = helpers.load_case('synth128x2')
    model = helpers.build_model('synth128x2', case, tmp_path_factory.mktemp('moves'), max_walkers=160)
    assert model.num_params == 17
    yield case, model
    model.close()


def test_device_equals_host_small_odd_half(synth):
    """22 walkers (a half of 11), DEMove(jump=0.2), blocks of 4 over 10 iterations; never a whole-iteration launch."""
    case, model = synth
    p0 = tight_start(model, case, 22, 1)
    before = model.engine.get_option('speculated_runs')
    host, dev, _ = pair(22, model, DEMove(jump=0.2), 11, block=4)
    out_h = list(host.sample(p0, iterations=10))
    out_d = list(dev.sample(p0, iterations=10))
    same_chain(dev, host, exact_lnp=False)
    assert len(out_d) == 10 and np.array_equal(out_d[-1][0], out_h[-1][0])
    assert model.engine.get_option('speculated_runs') == before
    assert 0 < dev.naccepted.sum() < 22 * 10
    for (_, _, sd), (_, _, sh) in zip(out_d, out_h):                  # the yielded generator states
        assert all(np.array_equal(a, b) for a, b in zip(sd, sh))


def test_more_than_one_workgroup_of_proposals(synth):
    """140 walkers: a half of 70 is 70 x 17 = 1190 elements (five workgroups of k_move_propose) and crosses the
    64-walker tile of the record kernel; the half-and-half mixture over 6 iterations, both moves drawn."""
    case, model = synth
    p0 = tight_start(model, case, 140, 2)
    host, dev, kinds = pair(140, model, mixture(), 3, block=4)
    list(host.sample(p0, iterations=6))
    list(dev.sample(p0, iterations=6))
    assert len(kinds) == 12 and kinds[0::2] == kinds[1::2] and set(kinds) == {0, 1}, kinds
    same_chain(dev, host)
    assert dev.naccepted.sum() > 0


def test_resume_from_a_yielded_state(synth):
    """(pos, lnprob, rstate) of a yield inside a block and at a block edge continues the host's chain."""
    case, model = synth
    p0 = tight_start(model, case, 22, 3)
    host, dev, _ = pair(22, model, mixture(), 5, block=4)
    list(host.sample(p0, iterations=10))
    out_d = list(dev.sample(p0, iterations=10))
    same_chain(dev, host)
    for stop in (2, 4):
        pos, lnp, rstate = out_d[stop - 1]
        again = DeviceEnsembleSampler(22, model, moves=mixture(), live_dangerously=True, block=4)
        list(again.sample(pos, lnprob0=lnp, rstate0=rstate, iterations=10 - stop))
        assert np.array_equal(again.chain, host.chain[:, stop:]), stop
        assert np.array_equal(again.lnprobability, host.lnprobability[:, stop:]), stop


def test_accumulation(synth):
    """accumulate=True: the images equal those accumulated from the host chain's positions (the bound of
    tests/test_gpu_fitting.py's stretch sampler)."""
    case, model = synth
    p0 = tight_start(model, case, 22, 4)
    host, dev, _ = pair(22, model, mixture(), 3, block=4, accumulate=True)
    model.reset_images()
    list(dev.sample(p0, iterations=5))
    got = {k: v.copy() for k, v in model.collect_posterior_images().items()}
    assert model.accumulated_samples == 22 * 5
    list(host.sample(p0, iterations=5))
    same_chain(dev, host)
    model.reset_images()
    for it in range(5):
        model.accumulate_samples(host.chain[:, it])
    want = model.collect_posterior_images()
    for k in want:
        assert np.allclose(got[k], want[k], rtol=1e-11, atol=1e-12 * np.abs(want[k]).max()), k
    model.reset_images()


def test_sharded_half_steps_in_one_process(synth):
    """open, set_moves, then every half-step evaluated in the two unequal blocks [0, 4) and [4, 11), gathered by
    hand, accepted; close.  The chain is psfmc_move_run's, bit for bit."""
    import torch
    case, model = synth
    eng = model.engine
    n_w, n_iter, half = 22, 5, 11
    p0 = tight_start(model, case, n_w, 5)
    lnp0 = model.log_posterior_batch(p0)
    samp = DeviceEnsembleSampler(n_w, model, moves=DEMove(jump=0.2), live_dangerously=True)
    samp.random_state = np.random.RandomState(17).get_state()
    (scal, lz, a, log_u, kind, b), _ = samp._draw(n_iter)
    assert np.all(kind == 1) and np.all(a != b) and not lz.any()
    nacc_run = np.zeros(n_w, dtype=np.int64)
    pos_r, lnp_r, chain_r, lnchain_r = eng.move_run(p0, lnp0, scal, lz, a, log_u, kind, b, nacc_run)
    assert 0 < nacc_run.sum() < n_w * n_iter
    nacc = np.zeros(n_w, dtype=np.int64)
    dev = torch.device('cuda:%d' % model._device)
    # every call and the gather on ONE torch stream of the test's own (the context's stream does not wait for
    # torch's default stream)
    side = torch.cuda.Stream(device=dev)
    stream = side.cuda_stream
    assert stream
    with torch.cuda.device(dev), torch.cuda.stream(side):
        first = torch.zeros(4, dtype=torch.float64, device=dev)
        second = torch.zeros(7, dtype=torch.float64, device=dev)
        eng.stretch_open(p0, lnp0, scal, lz, a, log_u, nacc, store=True)
        eng.stretch_set_moves(kind, b)
        kept = []
        for it in range(n_iter):
            for h in range(2):
                eng.stretch_half_eval(it, h, 0, 4, first.data_ptr(), stream)
                eng.stretch_half_eval(it, h, 4, 7, second.data_ptr(), stream)
                full = torch.cat([first, second]).contiguous()
                kept.append(full)
                eng.stretch_half_accept(it, h, full.data_ptr(), stream)
        side.synchronize()
        pos, lnp, chain, lnchain = eng.stretch_close(nacc, stream)
    assert np.array_equal(chain, chain_r) and np.array_equal(lnchain, lnchain_r)
    assert np.array_equal(pos, pos_r) and np.array_equal(lnp, lnp_r) and np.array_equal(nacc, nacc_run)
    # without set_moves the same open run is the stretch sampler's: nothing changed for it
    z = ((2.0 - 1.0) * np.random.RandomState(1).rand(n_iter, 2, half) + 1) ** 2.0 / 2.0
    lzs = (model.num_params - 1.0) * np.log(z)
    nacc_s, nacc_o = np.zeros(n_w, dtype=np.int64), np.zeros(n_w, dtype=np.int64)
    eng.set_option('speculate', 0)
    want = eng.stretch_run(p0, lnp0, z, lzs, a, log_u, nacc_s)
    eng.set_option('speculate', -1)
    with torch.cuda.device(dev), torch.cuda.stream(side):
        whole = torch.zeros(half, dtype=torch.float64, device=dev)
        eng.stretch_open(p0, lnp0, z, lzs, a, log_u, nacc_o, store=True)
        for it in range(n_iter):
            for h in range(2):
                eng.stretch_half_eval(it, h, 0, half, whole.data_ptr(), stream)
                eng.stretch_half_accept(it, h, whole.data_ptr(), stream)
        side.synchronize()
        got = eng.stretch_close(nacc_o, stream)
    assert np.array_equal(got[2], want[2]) and np.array_equal(nacc_o, nacc_s)
    # ... and psfmc_move_run with stretch kinds is psfmc_stretch_run's chain
    nacc_k = np.zeros(n_w, dtype=np.int64)
    as_moves = eng.move_run(p0, lnp0, z, lzs, a, log_u, np.zeros(n_iter, dtype=np.int32), np.zeros_like(b), nacc_k)
    assert np.array_equal(as_moves[2], want[2]) and np.array_equal(as_moves[3], want[3])
    assert np.array_equal(nacc_k, nacc_s)


def test_out_of_support_proposals_stay_put():
    """A Sersic magnitude with a prior 0.1 mag wide and walkers spread over it: with jump = 0.5 (g = 1) a good share
    of the DE proposals leave the support; their log-posterior is -inf, the walker stays, and the chain is the
    host's."""
    from psfmc_amd.distributions import Uniform
    from test_joint_link import make_field, make_model
    fld = make_field(64, 64, 11, seed=41)
    model = make_model(fld, max_walkers=32, sersic_mag=Uniform(loc=20.45, scale=0.1))
    n_w, rng = 22, np.random.RandomState(6)
    assert model.num_params == 11
    p0 = fld['truth'] + rng.normal(size=(n_w, 11)) * 1e-3
    names = sum(([n] * w for n, w in zip(model.param_names, model.param_lens)), [])
    p0[:, names.index('1_Sersic_mag')] = 20.45 + 0.1 * rng.uniform(0.02, 0.98, n_w)
    p0[:, -1] = np.arange(n_w) % 2                                  # the PSF index
    assert np.all(np.isfinite(model.log_posterior_batch(p0)))
    outside = []

    def spy(theta):
        lnp = model.log_posterior_batch(theta)
        outside.append((np.array(theta), lnp == -np.inf))
        return lnp

    host, dev, _ = pair(n_w, model, DEMove(jump=0.5), 9, fn=spy, block=4)
    list(host.sample(p0, iterations=8))
    list(dev.sample(p0, iterations=8))
    same_chain(dev, host)
    n_out = sum(int(flag.sum()) for _, flag in outside)
    assert n_out >= 8 and dev.naccepted.sum() > 0, n_out
    flat = dev.chain.reshape(-1, 11)
    for q, flag in outside:                                         # no such proposal was ever taken
        for row in q[flag]:
            assert not np.any(np.all(flat == row, axis=1))
    assert np.all(np.isfinite(dev.lnprobability))
    model.close()


def test_joint_fit():
    """Two 64^2 exposures with one per-field parameter, 24 joint walkers, the mixture, 6 iterations."""
    from psfmc_amd import JointModel
    from test_joint_link import make_field, make_model
    flds = [make_field(64, 64, 11, seed=50 + f) for f in range(2)]
    joint = JointModel([make_model(fld) for fld in flds], per_field=['0_PointSource_mag'], max_walkers=2 * 24)
    n_w, dim = 24, joint.num_params
    truth = np.zeros(dim)
    for f, fld in enumerate(flds):
        truth[joint.field_columns(f)] = fld['truth']
    p0 = truth + np.random.RandomState(8).normal(size=(n_w, dim)) * 1e-3
    for f in range(2):
        col = sum(joint.param_lens[:joint.param_names.index('PSF_Index_f%d' % f)])
        p0[:, col] = np.arange(n_w) % 2
    host, dev, kinds = pair(n_w, joint, mixture(), 3, block=4, accumulate=True)
    for m in joint.field_models:
        m.reset_images()
    list(host.sample(p0, iterations=6))
    list(dev.sample(p0, iterations=6))
    assert set(kinds) == {0, 1}, kinds
    same_chain(dev, host)
    assert dev.naccepted.sum() > 0 and np.all(np.isfinite(dev.lnprobability))
    assert all(m.accumulated_samples == 6 * n_w for m in joint.field_models)
    joint.close()


def test_one_general_component():
    """A Sersic with fixed Fourier modes and a free spiral: the auxiliary table on the "theta is given" route of the
    record kernel.  22 walkers, DE, 5 iterations."""
    import test_gpu_spiral_arms as tsa
    fld = tsa.make_field(64, 64, seed=7)
    model = tsa.make_model(fld, tsa.LEAN_SPIRAL, fourier={2: (0.08, 25.0), 3: (0.05, -40.0)}, max_walkers=22,
                           lean=True)
    assert model.num_params == 10
    p0 = tsa._lean_start(fld, 22, 2)
    host, dev, _ = pair(22, model, DEMove(jump=0.2), 8, block=4)
    list(host.sample(p0, iterations=5))
    list(dev.sample(p0, iterations=5))
    same_chain(dev, host)
    assert dev.naccepted.sum() > 0 and np.all(np.isfinite(dev.lnprobability))
    model.close()


def refused(text, call, *args):
    with pytest.raises(NativeError) as err:
        call(*args)
    assert err.value.code == EINVAL and text in str(err.value), err.value


def test_library_refusals(synth):
    """PSFMC_EINVAL with its text for a == b, a partner out of range, W = 2 with a DE kind and a FieldSet context;
    the context still samples afterwards."""
    from psfmc_amd.models import FieldSet
    from test_joint_link import make_field, make_model
    case, model = synth
    eng = model.engine
    n_w, n_iter, half = 22, 3, 11
    p0 = tight_start(model, case, n_w, 6)
    lnp0 = model.log_posterior_batch(p0)
    samp = DeviceEnsembleSampler(n_w, model, moves=DEMove(), live_dangerously=True)
    samp.random_state = np.random.RandomState(2).get_state()
    (scal, lz, a, log_u, kind, b), _ = samp._draw(n_iter)
    nacc = np.zeros(n_w, dtype=np.int64)
    good = (p0, lnp0, scal, lz, a, log_u, kind, b, nacc)

    def with_(**kw):
        names = ('pos', 'lnprob', 'scal', 'lz', 'a', 'log_u', 'kind', 'b', 'nacc')
        return tuple(kw.get(n, v) for n, v in zip(names, good))
    same = b.copy()
    same[1, 1, 4] = a[1, 1, 4]
    refused('must differ', eng.move_run, *with_(b=same))
    for bad in (half, -1):
        far = b.copy()
        far[2, 0, 10] = bad
        refused('out of range', eng.move_run, *with_(b=far))
        far = a.copy()
        far[0, 1, 0] = bad
        refused('out of range', eng.move_run, *with_(a=far))
        stretch_far = a.copy()
        stretch_far[0, 0, 3] = bad                                   # a is checked for a stretch kind too
        refused('out of range', eng.move_run, *with_(a=stretch_far, kind=np.zeros(n_iter, dtype=np.int32)))
    refused('not a move', eng.move_run, *with_(kind=np.array([1, 2, 1], dtype=np.int32)))
    two = (p0[:2], lnp0[:2], scal[:, :, :1], lz[:, :, :1], np.zeros((n_iter, 2, 1), dtype=np.int32), log_u[:, :, :1],
           kind, np.zeros((n_iter, 2, 1), dtype=np.int32), np.zeros(2, dtype=np.int64))
    refused('W >= 4', eng.move_run, *two)
    # the half-step form: set_moves before open, and bad partners after it
    refused('psfmc_stretch_open', lambda: eng._check(eng._lib.psfmc_stretch_set_moves(eng._ctx, None, None)))
    eng.stretch_open(p0, lnp0, scal, lz, a, log_u, nacc, store=True)
    refused('must differ', eng.stretch_set_moves, kind, same)
    eng.stretch_set_moves(kind, b)
    eng.stretch_close(nacc)
    assert not nacc.any()
    # a context of several fields
    flds = [make_field(64, 64, 11, seed=60 + f) for f in range(2)]
    fieldset = FieldSet([make_model(fld) for fld in flds], max_walkers=2 * n_w)
    ctx = fieldset.context
    dim = fieldset.num_params
    args = (np.zeros((n_w, dim)), np.zeros(n_w), scal, lz, a, log_u, kind, b, np.zeros(n_w, dtype=np.int64))
    rc, _ = _move_run(ctx._lib.psfmc_move_run, ctx._ctx, *args, True, False)
    assert rc == EINVAL and 'one field' in ctx._lib.psfmc_last_error().decode()
    with pytest.raises(NotImplementedError, match='move_run'):
        fieldset.models[0].engine.move_run(*args)
    with pytest.raises(NotImplementedError, match='moves='):
        DeviceEnsembleSampler(n_w, fieldset.models[0], moves=DEMove(), live_dangerously=True)
    fieldset.close()
    # the run goes through afterwards
    out = eng.move_run(*good)
    assert np.all(np.isfinite(out[3])) and nacc.sum() > 0


def _example(tmp_path):
    src = os.path.join(helpers.GOLDEN, 'example')
    for name in os.listdir(src):
        if os.path.isfile(os.path.join(src, name)):
            shutil.copy(os.path.join(src, name), tmp_path)
    return str(tmp_path / 'model_example.py')


def test_model_galaxy_mcmc_with_moves(tmp_path):
    """`model_galaxy_mcmc` on the example field with the half-and-half mixture, 20 + 20 iterations: MCMOVES in the
    header, a second run from the same `random_state` identical; with moves=None no MCMOVES and the chain of a
    `DeviceEnsembleSampler` driven directly as before.  38 chains: the example model has 18 free parameters and the
    samplers refuse fewer than 2 P = 36 walkers (emcee's rule; `model_galaxy_mcmc` has no way round it), so 38 =
    2 P + 2, the entry point's own default, stands in for 22."""
    from psfmc_amd import MultiComponentModel, load_database, model_galaxy_mcmc
    model_file = _example(tmp_path)
    moves = [(StretchMove(), 0.5), (DEMove(), 0.5)]
    dbs = []
    for tag in ('a', 'b'):
        np.random.seed(42)                                          # prior draws use the global numpy RNG
        model, db = model_galaxy_mcmc(model_file, output_name=str(tmp_path / ('out_' + tag)), iterations=20, burn=20,
                                      chains=38, random_state=7, quiet=True, moves=moves)
        on_disk = load_database(str(tmp_path / ('out_' + tag)) + '_db.fits')
        assert on_disk.meta['MCMOVES'] == 'stretch:0.5,de:0.5' and on_disk.meta['MCITER'] == 20
        assert len(on_disk) == 38 * 20 and 0.0 < on_disk.meta['MCACCEPT'] < 1.0
        theta = on_disk.param_matrix(model.param_names)
        assert helpers.rel_err(model.log_posterior_batch(theta[::29]), on_disk['lnprobability'][::29]) <= 1e-12
        dbs.append((theta, on_disk['lnprobability'].copy()))
        model.close()
    assert np.array_equal(dbs[0][0], dbs[1][0]) and np.array_equal(dbs[0][1], dbs[1][1])
    # moves=None: today's run
    np.random.seed(42)
    model, db = model_galaxy_mcmc(model_file, output_name=str(tmp_path / 'out_none'), iterations=20, burn=20,
                                  chains=38, random_state=7, quiet=True, moves=None)
    plain = load_database(str(tmp_path / 'out_none') + '_db.fits')
    assert 'MCMOVES' not in plain.meta
    theta_none = plain.param_matrix(model.param_names)
    assert not np.array_equal(theta_none, dbs[0][0])
    model.close()
    np.random.seed(42)
    model = MultiComponentModel(model_file, max_walkers=1024)
    p0 = model.init_params_from_priors(38)
    direct = DeviceEnsembleSampler(38, model)
    direct.random_state = np.random.RandomState(7).get_state()
    pos = lnp = None
    for pos, lnp, _ in direct.sample(p0, iterations=20):
        pass
    direct.reset()
    list(direct.sample(pos, lnprob0=lnp, iterations=20))
    assert np.array_equal(theta_none, direct.chain.reshape(-1, model.num_params))       # (rows: walker-major)
    assert np.array_equal(plain['lnprobability'], direct.lnprobability.ravel())
    assert plain.meta['MCACCEPT'] == pytest.approx(float(direct.acceptance_fraction.mean()), rel=1e-12)   # (header text)
    model.close()
