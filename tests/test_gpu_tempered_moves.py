"""Proposal moves on the tempered and field-set device samplers (psfmc_pt_move_run, psfmc_pt_move_run_joint,
psfmc_pt_move_run_fields, k_pt_move_propose; `set_moves` on DeviceTemperedSampler, FieldSetTemperedSampler and
FieldSetSampler).  Every run is held, with `array_equal`, to the host contract -- `TemperedEnsembleSampler` +
`set_moves`, or `EnsembleSampler(moves=)` -- fed the device's own evaluation, and the fields of a set to their own
one-field device runs as well.  64^2 fields, at most 16 iterations per run."""
import os
import shutil

import numpy as np
import pytest

import helpers
import test_gpu_mixed_fields as mixed
import test_gpu_spiral_arms as tgs
from test_gpu_fields_tempered import _assert_same_run, _assert_same_yields, _square_start
from test_gpu_fullsize import make_model as square_model
from test_gpu_joint_tempered import _fields as joint_fields, _ladder_start
from test_gpu_moves import telling
from test_joint_link import POS, make_model as link_model
from psfmc_amd.engine import NativeError
from psfmc_amd.sampler import (DEMove, DeviceEnsembleSampler, DeviceTemperedSampler, EnsembleSampler, StretchMove,
                               TemperedEnsembleSampler, default_betas)

pytestmark = pytest.mark.gpu

EINVAL = -1                 # include/psfmc_hip.h PSFMC_EINVAL
N_F, N_T, N_W, N_ITER, BLOCK = 3, 4, 22, 16, 7


def mixture(jump=0.2):
    return [(StretchMove(), .5), (DEMove(jump=jump), .5)]


def contract(n_w, dim, betas, fn, moves, seed):
    """The host contract with `moves` set, on the generator state of `seed`: (sampler, the kind every draw call
    drew from -- per iteration 2 T entries, all alike)."""
    host_moves, kinds = telling(moves)
    host = TemperedEnsembleSampler(n_w, dim, betas, fn)
    host.set_moves(host_moves)
    host.random_state = np.random.RandomState(seed).get_state()
    return host, kinds


def device(n_w, model, betas, moves, seed, **kw):
    dev = DeviceTemperedSampler(n_w, model, betas=betas, **kw)
    dev.set_moves(moves)
    dev.random_state = np.random.RandomState(seed).get_state()
    return dev


def per_iteration(kinds, n_t):
    """One kind per iteration from `telling`'s list; every rung and both half-steps of an iteration drew alike."""
    rows = [kinds[i:i + 2 * n_t] for i in range(0, len(kinds), 2 * n_t)]
    assert all(len(set(r)) == 1 for r in rows)
    return [r[0] for r in rows]


@pytest.fixture(scope='module')
def own3():
    """Three 64^2 fields, each a model with a context of its own that holds one ladder."""
    pairs = [square_model(64, 1, 'fused', max_walkers=N_T * 24, seed=s) for s in range(N_F)]
    yield pairs
    for m, _ in pairs:
        m.close()


@pytest.fixture(scope='module')
def set3():
    from psfmc_amd import FieldSet
    fs = FieldSet([square_model(64, 1, 'fused', max_walkers=1, seed=s)[0] for s in range(N_F)],
                  max_walkers=N_F * N_T * N_W)
    yield fs
    fs.close()


@pytest.fixture(scope='module')
def one_field(own3):
    """Case 1, computed once: field 0's ladder of T = 4 rungs of W = 22 walkers (a half of 11: odd, below a wave;
    4 x 11 x 10 = 440 proposal elements: rung boundaries inside a workgroup, two workgroups) in blocks of 7 with the
    half-and-half mixture, on the device and by the contract fed the device's own split evaluation."""
    model, fld = own3[0]
    betas = default_betas(N_T, 50.0)
    p0 = _square_start(fld, N_T, N_W, seed=3)
    host, kinds = contract(N_W, model.num_params, betas, model.log_likelihood_and_prior_batch, mixture(), 11)
    dev = device(N_W, model, betas, mixture(), 11, block=BLOCK)
    out_h = list(host.sample(p0, iterations=N_ITER))
    out_d = list(dev.sample(p0, iterations=N_ITER))
    return dict(model=model, betas=betas, p0=p0, host=host, dev=dev, out_h=out_h, out_d=out_d,
                kinds=per_iteration(kinds, N_T))


def test_one_field_ladder_equals_the_contract(one_field):
    r = one_field
    assert r['model'].num_params == 10
    assert set(r['kinds'][:BLOCK]) == {0, 1}, r['kinds']             # both kinds within the first block
    _assert_same_run(r['dev'], r['host'], 0)
    _assert_same_yields(r['out_d'], r['out_h'], 0)
    assert r['dev'].nswap.sum() > 0 and np.all(r['dev'].naccepted_t.sum(axis=1) > 0)
    assert np.all(r['dev'].naccepted_t <= N_ITER)


def test_the_smallest_de_ensemble(own3):
    """W = 4: a half of 2, so b is forced to the walker a is not; T = 3, pure DEMove()."""
    model, fld = own3[1]
    betas = default_betas(3, 20.0)
    p0 = _square_start(fld, 3, 4, seed=5)
    host, kinds = contract(4, model.num_params, betas, model.log_likelihood_and_prior_batch, DEMove(), 21)
    dev = device(4, model, betas, DEMove(), 21, block=5)
    out_h = list(host.sample(p0, iterations=12))
    out_d = list(dev.sample(p0, iterations=12))
    assert set(kinds) == {1} and len(kinds) == 12 * 2 * 3
    _assert_same_run(dev, host, 1)
    _assert_same_yields(out_d, out_h, 1)
    assert dev.naccepted_t.sum() > 0


@pytest.mark.parametrize('stop', [3, 7])
def test_resuming_inside_a_block_and_at_a_block_edge(one_field, stop):
    r = one_field
    pos, ll, lp, rstate = r['out_d'][stop - 1]
    again = DeviceTemperedSampler(N_W, r['model'], betas=r['betas'], block=BLOCK)
    again.set_moves(mixture())
    rest = list(again.sample(pos, ll, lp, rstate0=rstate, iterations=N_ITER - stop))
    assert np.array_equal(again.chain, r['host'].chain[:, stop:])
    assert np.array_equal(again.lnlikelihood, r['host'].lnlikelihood[:, :, stop:])
    assert np.array_equal(again.lnprobability, r['host'].lnprobability[:, stop:])
    _assert_same_yields(rest, r['out_h'][stop:], 0)


def test_joint_fit_of_two_exposures():
    """64 x 64 beside 64 x 96 with the positions per field, T = 3, W = 22: the joint prior and F field records of
    given vectors per half-step, against the contract fed the joint model's split evaluation."""
    from psfmc_amd import JointModel
    flds = joint_fields()
    joint = JointModel([link_model(fld) for fld in flds], per_field=POS, max_walkers=3 * N_W * 2)
    try:
        betas = default_betas(3, 50.0)
        p0 = _ladder_start(joint, flds, 3, N_W, seed=22)
        host, kinds = contract(N_W, joint.num_params, betas, joint.log_likelihood_and_prior_batch, mixture(), 11)
        dev = device(N_W, joint, betas, mixture(), 11, block=5)
        out_h = list(host.sample(p0, iterations=12))
        out_d = list(dev.sample(p0, iterations=12))
        assert set(per_iteration(kinds, 3)) == {0, 1}
        _assert_same_run(dev, host, 'joint')
        _assert_same_yields(out_d, out_h, 'joint')
        assert dev.nswap.sum() > 0 and np.all(dev.naccepted_t.sum(axis=1) > 0)
    finally:
        joint.close()


def test_three_fields_each_its_own_ladder_and_its_own_moves(own3, set3, one_field):
    """F = 3, T = 4, W = 22: 1 320 proposal elements, six workgroups, ladder boundaries inside a workgroup.  Every
    field equals its own `DeviceTemperedSampler` + `set_moves` run and the contract fed the member model's split
    evaluation; the fields draw their own selectors, and in some iteration two of them run different moves."""
    from psfmc_amd import FieldSetTemperedSampler
    betas = one_field['betas']
    p0 = np.array([_square_start(fld, N_T, N_W, seed=3 + f) for f, (_, fld) in enumerate(own3)])
    together = FieldSetTemperedSampler(N_W, set3, betas=betas, block=BLOCK)
    together.set_moves(mixture())
    for f, sub in enumerate(together.fields):
        sub.random_state = np.random.RandomState(700 + f).get_state()
    yields = list(together.sample(p0, iterations=N_ITER))
    kinds = []
    for f, (model, _) in enumerate(own3):
        solo = device(N_W, model, betas, mixture(), 700 + f, block=BLOCK)
        want = list(solo.sample(p0[f], iterations=N_ITER))
        _assert_same_run(together.fields[f], solo, f)
        _assert_same_yields([y[f] for y in yields], want, f)
        host, told = contract(N_W, set3.num_params, betas, set3.models[f].log_likelihood_and_prior_batch,
                              mixture(), 700 + f)
        out = list(host.sample(p0[f], iterations=N_ITER))
        _assert_same_run(together.fields[f], host, f)
        for k in range(3):
            assert np.array_equal(yields[-1][f][k], out[-1][k]), (f, k)
        kinds.append(per_iteration(told, N_T))
        assert together.fields[f].nswap.sum() > 0 and np.all(together.fields[f].naccepted_t.sum(axis=1) > 0), f
    assert any(len(set(at)) == 2 for at in zip(*kinds)), kinds       # (seeds 700 ...: iteration 1 is 0, 1, 0)
    # ... and set_moves(None) on the set is the set that never had moves
    for s in (together, FieldSetTemperedSampler(N_W, set3, betas=betas, block=BLOCK)):
        s.set_moves(None)
        s.reset()
        for f, sub in enumerate(s.fields):
            sub.random_state = np.random.RandomState(40 + f).get_state()
        list(s.sample(p0, iterations=5))
        chains = [sub.chain.copy() for sub in s.fields]
    for f in range(N_F):
        assert np.array_equal(together.fields[f].chain, chains[f]), f


def test_field_set_sampler_on_fields_of_different_size():
    """64^2 beside 96^2 (as tests/test_gpu_mixed_fields.py builds them), W = 24, blocks of 3 over 8 iterations:
    every field's chain is `EnsembleSampler(moves=)`'s fed the member model's log-posterior -- what its own
    `DeviceEnsembleSampler(moves=)` reproduces bit for bit -- and that device run's itself wherever the field's own
    context has the set's transform (the fields of a mixed set share one; tests/test_gpu_mixed_fields.py)."""
    from psfmc_amd import FieldSet, FieldSetSampler
    shapes = [(64, 64, 11), (96, 96, 13)]
    n_w, n_iter = 24, 8
    flds = [mixed._field(ny, nx, pk, seed=30 + f) for f, (ny, nx, pk) in enumerate(shapes)]
    fs = FieldSet([mixed._model(fld, 1) for fld in flds], max_walkers=2 * n_w)
    try:
        p0 = [fld['truth'] + np.random.RandomState(70 + f).normal(size=(n_w, 11)) * 1e-3 for f, fld in enumerate(flds)]
        for p in p0:
            p[:, 10] = np.arange(n_w) % 2
        both = FieldSetSampler(n_w, fs, block=3)
        both.set_moves(mixture())
        for f, sub in enumerate(both.fields):
            sub.random_state = np.random.RandomState(600 + f).get_state()
        yields = list(both.sample(p0, iterations=n_iter))
        transform = (fs.context.get_option('transform_ny'), fs.context.get_option('transform_nx'))
        same_transform, kinds = [], []
        for f in range(2):
            host_moves, told = telling(mixture())
            host = EnsembleSampler(n_w, fs.num_params, batch_lnpostfn=fs.models[f].log_posterior_batch,
                                   moves=host_moves)
            host.random_state = np.random.RandomState(600 + f).get_state()
            out = list(host.sample(p0[f], iterations=n_iter))
            sub = both.fields[f]
            assert np.array_equal(sub.chain, host.chain), f
            assert np.array_equal(sub.lnprobability, host.lnprobability), f
            assert np.array_equal(sub.naccepted, host.naccepted) and host.naccepted.sum() > 0, f
            for j in range(n_iter):                              # (the host yields its live arrays: its chain instead)
                assert np.array_equal(yields[j][f][0], host.chain[:, j]), (f, j)
                assert np.array_equal(yields[j][f][1], host.lnprobability[:, j]), (f, j)
                assert all(np.array_equal(a, b) for a, b in zip(yields[j][f][2], out[j][2])), (f, j)
            kinds.append(told[0::2])
            own = mixed._model(flds[f], n_w)
            if (own.engine.get_option('transform_ny'), own.engine.get_option('transform_nx')) == transform:
                same_transform.append(f)
                solo = DeviceEnsembleSampler(n_w, own, block=3, moves=mixture())
                solo.random_state = np.random.RandomState(600 + f).get_state()
                list(solo.sample(p0[f], iterations=n_iter))
                assert np.array_equal(sub.chain, solo.chain), f
                assert np.array_equal(sub.lnprobability, solo.lnprobability), f
                assert np.array_equal(sub.naccepted, solo.naccepted), f
            own.close()
        assert 1 in same_transform
        assert all(set(k) == {0, 1} for k in kinds) and kinds[0] != kinds[1], kinds
        # a yielded state resumes (the start's lnprob is given), and set_moves(None) is the set without moves
        stop = 4
        again = FieldSetSampler(n_w, fs, block=3)
        again.set_moves(mixture())
        for f, sub in enumerate(again.fields):
            sub.random_state = yields[stop - 1][f][2]
        list(again.sample([y[0] for y in yields[stop - 1]], [y[1] for y in yields[stop - 1]],
                          iterations=n_iter - stop))
        for f in range(2):
            assert np.array_equal(again.fields[f].chain, both.fields[f].chain[:, stop:]), f
            assert np.array_equal(again.fields[f].lnprobability, both.fields[f].lnprobability[:, stop:]), f
        plain = FieldSetSampler(n_w, fs, block=3)
        for s in (again, plain):
            s.set_moves(None)
            s.reset()
            for f, sub in enumerate(s.fields):
                sub.random_state = np.random.RandomState(9 + f).get_state()
            list(s.sample(p0, iterations=4))
        for f in range(2):
            assert np.array_equal(again.fields[f].chain, plain.fields[f].chain), f
    finally:
        fs.close()


def test_fourier_modes_and_a_spiral_on_the_given_vector_route():
    """A Sersic with a free Fourier mode and spiral arms (the auxiliary table), T = 2, W = 26."""
    fld = tgs.make_field(64, 64, seed=8)
    model = tgs.make_model(fld, tgs.LEAN_SPIRAL, fourier={1: (tgs.FREE, tgs.FREE)}, max_walkers=2 * 26, lean=True)
    try:
        assert model.num_params == 12
        s = dict(four=[0.1, 20.0], spi=dict(r_out=9.0, winding=120.0), index=1.5, mag=18.0, reff=6.0, reff_b=3.0,
                 x=32.3, y=30.8)
        base = tgs.theta_of(fld, s, lean=True)
        p0 = base + np.random.RandomState(3).normal(size=(2 * 26, len(base))) * 1e-2
        ir, ib = tgs.column(model, '2_Sersic_reff'), tgs.column(model, '2_Sersic_reff_b')
        p0[:, ib] = np.minimum(p0[:, ib], p0[:, ir] - 1e-3)
        p0 = p0.reshape(2, 26, -1)
        betas = np.array([1.0, 0.0])
        host, kinds = contract(26, 12, betas, model.log_likelihood_and_prior_batch, mixture(), 11)
        dev = device(26, model, betas, mixture(), 11, block=3)
        out_h = list(host.sample(p0, iterations=8))
        out_d = list(dev.sample(p0, iterations=8))
        assert set(per_iteration(kinds, 2)) == {0, 1}
        _assert_same_run(dev, host, 'spiral')
        _assert_same_yields(out_d, out_h, 'spiral')
        assert np.all(np.isfinite(dev.lnlikelihood[0])) and dev.naccepted_t.sum() > 0
    finally:
        model.close()


def test_accumulation_of_the_beta_one_rung(own3):
    """accumulate=True: the beta = 1 image sums are those of the stored chain (tests/test_gpu_tempered.py's bound)."""
    model, fld = own3[2]
    p0 = _square_start(fld, 3, 24, seed=9)
    model.reset_images()
    acc = device(24, model, default_betas(3, 20.0), mixture(), 3, block=4, accumulate=True)
    steps = list(acc.sample(p0, iterations=6))
    got = {k: v.copy() for k, v in model.collect_posterior_images().items()}
    assert model.accumulated_samples == 6 * 24
    model.reset_images()
    for pos, _, _, _ in steps:
        model.accumulate_samples(pos[0])
    want = model.collect_posterior_images()
    for k in want:
        assert np.allclose(got[k], want[k], rtol=1e-11, atol=1e-12 * np.abs(want[k]).max()), k
    model.reset_images()


def _draws(n_iter, n_t, n_w, kind, seed=0):
    """Valid arrays of Context.pt_move_run: (scal, lz, partner, log_u, kind, partner_b, swap_i, swap_j, swap_log_u)."""
    rs = np.random.RandomState(seed)
    half = n_w // 2
    z = 0.5 + rs.rand(n_iter, 2, n_t, half)
    a = rs.randint(half, size=(n_iter, 2, n_t, half)).astype(np.int32)
    b = ((a + 1 + rs.randint(max(half - 1, 1), size=a.shape)) % half).astype(np.int32)
    log_u = np.log(rs.rand(n_iter, 2, n_t, half))
    perms = lambda: np.array([[rs.permutation(n_w) for _ in range(n_t - 1)]
                              for _ in range(n_iter)]).astype(np.int32).reshape(n_iter, n_t - 1, n_w)
    si, sj = perms(), perms()
    slu = np.log(rs.rand(n_iter, n_t - 1, n_w))
    kind = np.array(kind, dtype=np.int32)
    lz = np.where(kind[:, None, None, None] == 1, 0.0, 9.0 * np.log(z))
    return [z, lz, a, log_u, kind, b, si, sj, slu]


def test_library_refusals(own3):
    """Each refusal of psfmc_pt_move_run by its psfmc_last_error text, before anything is uploaded, and a good run
    straight after them."""
    model, fld = own3[0]
    eng = model.engine
    betas = default_betas(3, 20.0)

    def run(n_w, kind, change=None):
        p0 = _square_start(fld, 3, n_w, seed=1)
        args = _draws(len(kind), 3, n_w, kind)
        if change:
            change(args)
        nacc, nsw = np.zeros((3, n_w), dtype=np.int64), np.zeros(2, dtype=np.int64)
        return eng.pt_move_run(betas, p0, None, None, *args, naccepted=nacc, nswap=nsw), nacc, nsw

    def refused(text, *args):
        with pytest.raises(NativeError, match=text) as err:
            run(*args)
        assert err.value.code == EINVAL

    refused('kind.*is not a move', 22, [0, 2, 1])
    refused('needs W >= 4', 2, [0, 1])

    def b_out_of_range(args):
        args[5][1, 1, 2, 3] = 11                                 # half = 11: one past the end, a DE iteration

    refused(r'partner index 11 out of range \[0, 11\) at iteration 1', 22, [0, 1], b_out_of_range)

    def b_negative(args):
        args[5][0, 0, 0, 0] = -1

    refused('partner index -1 out of range', 22, [1, 0], b_negative)

    def a_equals_b(args):
        args[5][2, 0, 1, 4] = args[2][2, 0, 1, 4]

    refused('must differ', 22, [0, 0, 1], a_equals_b)

    def a_out_of_range(args):                                    # what psfmc_pt_run refuses is still refused
        args[2][0, 1, 1, 2] = 11

    refused('partner index 11 outside', 22, [0, 1], a_out_of_range)

    def bad_swap(args):
        args[6][1, 0, 0] = args[6][1, 0, 1]

    refused('permutations', 22, [0, 1], bad_swap)
    with pytest.raises(NativeError, match='last rung') as err:
        p0 = _square_start(fld, 3, 22, seed=1)
        eng.pt_move_run(np.array([1.0, 0.5, 0.1]), p0, None, None, *_draws(2, 3, 22, [0, 1]),
                        naccepted=np.zeros((3, 22), dtype=np.int64), nswap=np.zeros(2, dtype=np.int64))
    assert err.value.code == EINVAL

    # partner_b is not read in a stretch iteration: nonsense there is no refusal, and the context runs correctly
    def nonsense_in_stretch_iterations(args):
        args[5][[0, 2]] = -7

    kind = [0, 1, 0, 1]
    (pos, ll, lp, chain, lnchain, llchain, lpchain), nacc, nsw = run(22, kind, nonsense_in_stretch_iterations)
    assert nacc.sum() > 0 and np.isfinite(ll[0]).all()
    again = model.log_likelihood_and_prior_batch(pos.reshape(-1, model.num_params))
    assert np.array_equal(again[0].reshape(ll.shape), ll) and np.array_equal(again[1].reshape(lp.shape), lp)
    assert np.array_equal(chain[:, :, -1], pos) and np.array_equal(llchain[:, :, -1], ll)
    # with W = 2 the stretch move still runs (no second partner needed)
    (pos2, ll2, _, _, _, _, _), nacc2, _ = run(2, [0, 0, 0])
    assert pos2.shape == (3, 2, model.num_params) and np.isfinite(ll2[0]).all()


def test_set_moves_none_after_moves_is_the_sampler_that_never_had_them(one_field):
    model, betas, p0 = one_field['model'], one_field['betas'], one_field['p0']
    never = DeviceTemperedSampler(N_W, model, betas=betas, block=BLOCK)
    back = DeviceTemperedSampler(N_W, model, betas=betas, block=BLOCK)
    back.set_moves(mixture())
    back.random_state = np.random.RandomState(5).get_state()
    first = list(back.sample(p0, iterations=3))[-1]              # three iterations with moves, then none
    back.set_moves(None)
    back.reset()
    out = []
    for s in (never, back):
        s.random_state = np.random.RandomState(6).get_state()
        out.append(list(s.sample(*first[:3], iterations=9)))
    _assert_same_run(back, never, 0)
    _assert_same_yields(out[1], out[0], 0)
    # the device samplers parse their moves as the host ones do
    for bad in ([(StretchMove(), 1.0), (DEMove(), -1.0)], [], 'de'):
        with pytest.raises(ValueError):
            back.set_moves(bad)
    small = DeviceTemperedSampler(2, model, betas=betas)
    with pytest.raises(ValueError, match='4 walkers'):
        small.set_moves(DEMove())
    plain = DeviceEnsembleSampler(22, model)
    plain.set_moves(mixture())
    assert len(plain._moves) == 2
    with pytest.raises(ValueError, match='weights'):
        plain.set_moves([(StretchMove(), 0.0), (DEMove(), 0.0)])


def test_model_galaxy_ptmcmc_with_moves(tmp_path):
    from psfmc_amd import load_database, model_galaxy_ptmcmc
    src = os.path.join(helpers.GOLDEN, 'example')
    for name in os.listdir(src):
        if os.path.isfile(os.path.join(src, name)):
            shutil.copy(os.path.join(src, name), tmp_path)
    metas = {}
    for label, moves in (('moves', mixture(0.1)), ('plain', None)):
        out = str(tmp_path / ('out_' + label))
        np.random.seed(42)
        model, db, (lnz, err) = model_galaxy_ptmcmc(str(tmp_path / 'model_example.py'), output_name=out,
                                                    iterations=12, burn=6, chains=40, ntemps=4, tmax=100.0,
                                                    random_state=7, quiet=True, moves=moves,
                                                    write_fits=('convolved_model',))
        stored = load_database(out + '_db.fits')
        assert len(stored) == 40 * 12 and stored.meta['MCNTEMPS'] == 4 and np.isfinite(stored.meta['MCLNZ'])
        theta = stored.param_matrix(model.param_names)
        again = model.log_posterior_batch(theta[::37])
        assert helpers.rel_err(again, stored['lnprobability'][::37]) <= 1e-12
        assert os.path.exists(out + '_convolved_model.fits') and model.accumulated_samples == 40 * 12
        metas[label] = dict(stored.meta)
        model.close()
    assert metas['moves']['MCMOVES'] == 'stretch:0.5,de:0.5'
    assert 'MCMOVES' not in metas['plain']
    assert set(metas['moves']) - {'MCMOVES'} == set(metas['plain'])


def test_model_fields_entry_points_with_moves(tmp_path):
    from psfmc_amd import load_database, model_fields_mcmc, model_fields_ptmcmc
    n_f, chains, n_t = 2, 22, 3
    kinds = ('convolved_model',)
    flds = [square_model(64, 1, 'fused', max_walkers=1, seed=s)[1] for s in range(n_f)]
    p0 = [_square_start(fld, n_t, chains, seed=5 + f) for f, fld in enumerate(flds)]
    for label, moves in (('moves', mixture(0.1)), ('plain', None)):
        names = [str(tmp_path / ('t_%s%d' % (label, f))) for f in range(n_f)]
        models = [square_model(64, 1, 'fused', max_walkers=1, seed=s)[0] for s in range(n_f)]
        results = model_fields_ptmcmc(models, output_names=names, write_fits=kinds, iterations=8, burn=4,
                                      chains=chains, ntemps=n_t, tmax=50.0, random_states=[7, 8],
                                      start_positions=p0, quiet=True, moves=moves)
        for f, (m, db, (lnz, err)) in enumerate(results):
            meta = load_database(names[f] + '_db.fits').meta
            assert (meta.get('MCMOVES') == 'stretch:0.5,de:0.5') if moves else ('MCMOVES' not in meta), (label, f)
            assert len(db) == 8 * chains and np.isfinite(lnz) and meta['MCNTEMPS'] == n_t
            m.close()
        names = [str(tmp_path / ('s_%s%d' % (label, f))) for f in range(n_f)]
        models = [square_model(64, 1, 'fused', max_walkers=1, seed=s)[0] for s in range(n_f)]
        results = model_fields_mcmc(models, output_names=names, write_fits=kinds, iterations=8, burn=4,
                                    chains=chains, random_states=[7, 8], start_positions=[p[0] for p in p0],
                                    convergence_check=lambda sampler: True, quiet=True, moves=moves)
        for f, (m, db) in enumerate(results):
            meta = load_database(names[f] + '_db.fits').meta
            assert (meta.get('MCMOVES') == 'stretch:0.5,de:0.5') if moves else ('MCMOVES' not in meta), (label, f)
            assert len(db) == 8 * chains and os.path.exists(names[f] + '_convolved_model.fits')
            m.close()
