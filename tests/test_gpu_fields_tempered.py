"""Every field of a FieldSet tempered together (psfmc_eval_theta_split_fields, psfmc_pt_run_fields,
FieldSetTemperedSampler, model_fields_ptmcmc).  The contract: field f's tempered run inside the set IS its own
`DeviceTemperedSampler` run on a context of its own -- chain, every rung's lnL, lnprobability, the counters and
every yielded state are `array_equal` given the same start, random state, ladder and block size.  The split
evaluation against each field's own context; the contract at a half-ensemble below a wave and over unequal fields
in several passes; resuming from yields; one rung against `FieldSetSampler`; the beta = 1 posterior images; the
refusals; and the entry point against `model_galaxy_ptmcmc`."""
import os

import numpy as np
import pytest

import synth_field
from test_gpu_fullsize import make_model as square_model
from test_joint_link import make_field, make_model

pytestmark = pytest.mark.gpu

EINVAL = -1                 # include/psfmc_hip.h PSFMC_EINVAL
N_F, N_T, N_W, N_ITER, BLOCK = 3, 4, 22, 16, 7
MAX_WALKERS = N_F * N_T * N_W


def _ladder():
    from psfmc_amd.sampler import default_betas
    return default_betas(N_T, 50.0)


def _square_start(fld, n_t, n_w, seed):
    """[T, W, P] of a 64^2 field: rung 0 near the truth, the hotter rungs drawn from the priors."""
    p0 = np.empty((n_t, n_w, len(fld['truth'])))
    p0[0] = synth_field.draw_walkers(64, 1, n_w, seed=seed, near_truth=fld['truth'], jitter=1e-3)
    for t in range(1, n_t):
        p0[t] = synth_field.draw_walkers(64, 1, n_w, seed=100 * seed + t)
    return p0


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _assert_same_run(sub, solo, f):
    assert np.array_equal(sub.chain, solo.chain), f
    assert np.array_equal(sub.lnlikelihood, solo.lnlikelihood), f
    assert np.array_equal(sub.lnprobability, solo.lnprobability), f
    assert np.array_equal(sub.naccepted_t, solo.naccepted_t), f
    assert np.array_equal(sub.nswap, solo.nswap), f
    assert sub.iterations == solo.iterations


def _assert_same_yields(got, want, f):
    assert len(got) == len(want)
    for j, (a, b) in enumerate(zip(got, want)):
        for k in range(3):
            assert np.array_equal(a[k], b[k]), (f, j, k)
        assert _same_state(a[3], b[3]), (f, j)


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
                  max_walkers=MAX_WALKERS)
    yield fs
    fs.close()


@pytest.fixture(scope='module')
def runs(own3, set3):
    """The reference runs, computed once: the set's 16 iterations (its sampler, every yield) and each field's own
    `DeviceTemperedSampler` run from the same start and random state."""
    from psfmc_amd import FieldSetTemperedSampler
    from psfmc_amd.sampler import DeviceTemperedSampler
    betas = _ladder()
    p0 = np.array([_square_start(fld, N_T, N_W, seed=3 + f) for f, (_, fld) in enumerate(own3)])
    together = FieldSetTemperedSampler(N_W, set3, betas=betas, block=BLOCK)
    for f, sub in enumerate(together.fields):
        sub.random_state = np.random.RandomState(700 + f).get_state()
    yields = list(together.sample(p0, iterations=N_ITER))
    solos, solo_yields = [], []
    for f, (model, _) in enumerate(own3):
        solo = DeviceTemperedSampler(N_W, model, betas=betas, block=BLOCK)
        solo.random_state = np.random.RandomState(700 + f).get_state()
        solo_yields.append(list(solo.sample(p0[f], iterations=N_ITER)))
        solos.append(solo)
    return dict(p0=p0, betas=betas, together=together, yields=yields, solos=solos, solo_yields=solo_yields)


def test_split_evaluation(own3, set3):
    thetas = []
    for f, (_, fld) in enumerate(own3):
        th = np.vstack([synth_field.draw_walkers(64, 1, 12, seed=20 + f, near_truth=fld['truth']),
                        synth_field.draw_walkers(64, 1, 12, seed=40 + f)])
        th[20, 5] = 30.0                                         # the Sersic magnitude outside its prior
        th[21, 0] = 10.0                                         # the point source's outside its prior
        th[22, 7] = th[22, 6] + 0.5                              # reff_b > reff
        th[23, 8:10] = (32.0, 32.0)                              # the Sersic centre on a pixel centre
        thetas.append(th)
    want = [m.log_likelihood_and_prior_batch(th) for (m, _), th in zip(own3, thetas)]
    post = [m.log_posterior_batch(th) for (m, _), th in zip(own3, thetas)]

    def check(got, rows=slice(None)):
        for f in range(N_F):
            ll, lp = got[f]
            assert np.array_equal(ll, want[f][0][rows]), f
            assert np.array_equal(lp, want[f][1][rows]), f
            fin = np.isfinite(post[f][rows])
            assert np.array_equal(ll[fin] + lp[fin], post[f][rows][fin]), f
            assert np.all(ll[~fin] == -np.inf), f

    for f in range(N_F):
        assert np.isfinite(post[f][:12]).all() and not np.isfinite(post[f][20:23]).any()
        assert np.all(want[f][1][20:23] == -np.inf)
    check(set3.log_likelihood_and_prior_batch(thetas))
    assert [np.array_equal(a, b) for a, b in zip(set3.log_posterior_batch(thetas), post)] == [True] * N_F
    # a member model's call goes through the shared context
    check([set3.models[f].log_likelihood_and_prior_batch(thetas[f]) for f in range(N_F)])
    only = set3.log_likelihood_and_prior_batch([None, thetas[1][5:9], None])
    assert only[0][0].size == 0 and np.array_equal(only[1][0], want[1][0][5:9])
    # the values do not depend on the batch: 72 records in several passes, and in another order
    ctx = set3.context
    chunk = ctx.get_option('chunk_walkers')
    ctx.set_option('chunk_walkers', 20)
    try:
        assert ctx._lib.psfmc_pass_size(ctx._ctx, N_F * 24) < N_F * 24
        check(set3.log_likelihood_and_prior_batch(thetas))
        perm = np.random.RandomState(1).permutation(24)
        check(set3.log_likelihood_and_prior_batch([th[perm] for th in thetas]), perm)
    finally:
        ctx.set_option('chunk_walkers', chunk)


def test_every_field_is_its_own_tempered_run(runs, set3):
    """F = 3, T = 4, W = 22 (a half of 11: odd, below a wave), blocks of 7."""
    from psfmc_amd.sampler import TemperedEnsembleSampler
    together = runs['together']
    for f, solo in enumerate(runs['solos']):
        sub = together.fields[f]
        _assert_same_run(sub, solo, f)
        _assert_same_yields([y[f] for y in runs['yields']], runs['solo_yields'][f], f)
        assert sub.nswap.sum() > 0 and np.all(sub.naccepted_t.sum(axis=1) > 0), f
        assert np.array_equal(sub.log_evidence(), solo.log_evidence(), equal_nan=True)
    # ... and the host contract itself, fed the member model's split evaluation
    host = TemperedEnsembleSampler(N_W, set3.num_params, runs['betas'], set3.models[1].log_likelihood_and_prior_batch)
    host.random_state = np.random.RandomState(701).get_state()
    out = list(host.sample(runs['p0'][1], iterations=N_ITER))
    _assert_same_run(together.fields[1], host, 1)
    for k in range(3):
        assert np.array_equal(runs['yields'][-1][1][k], out[-1][k])


def test_unequal_fields_in_several_passes():
    """64 x 64 with an 11-pixel PSF and 64 x 96 with a 13-pixel one, W = 40, T = 4: 160 records per half-step,
    ensemble and field boundaries inside one workgroup of the proposal kernel; four passes of at most 48.

    The fields of a mixed set share one transform shape, so a field whose own context would choose another one
    has log-likelihoods that differ from its own context's in the last digits (tests/test_gpu_mixed_fields.py
    holds them to 1e-12): every field is therefore held bit for bit to the definition, the host
    `TemperedEnsembleSampler` fed the member model's split evaluation, and to its own `DeviceTemperedSampler`
    wherever its own context has the set's transform -- the 64 x 96 field at least."""
    from psfmc_amd import FieldSet, FieldSetTemperedSampler
    from psfmc_amd.sampler import DeviceTemperedSampler, TemperedEnsembleSampler
    shapes = [(64, 64, 11), (64, 96, 13)]
    n_t, n_w, n_iter = 4, 40, 8
    flds = [make_field(ny, nx, pk, seed=60 + f) for f, (ny, nx, pk) in enumerate(shapes)]
    own = [make_model(fld, max_walkers=n_t * n_w) for fld in flds]
    fs = FieldSet([make_model(fld) for fld in flds], max_walkers=2 * n_t * n_w)
    betas = _ladder()
    p0 = np.empty((2, n_t, n_w, fs.num_params))
    np.random.seed(17)
    for f, fld in enumerate(flds):
        p0[f, 0] = fld['truth'] + np.random.RandomState(f).normal(size=(n_w, fs.num_params)) * 1e-3
        p0[f, 0, :, -1] = np.arange(n_w) % 2                     # the PSF index
        for t in range(1, n_t):
            p0[f, t] = own[f].init_params_from_priors(n_w)
    ctx = fs.context
    ctx.set_option('chunk_walkers', 48)
    assert ctx._lib.psfmc_pass_size(ctx._ctx, 2 * n_t * (n_w // 2)) < 160
    together = FieldSetTemperedSampler(n_w, fs, betas=betas, block=5)
    for f, sub in enumerate(together.fields):
        sub.random_state = np.random.RandomState(50 + f).get_state()
    yields = list(together.sample(p0, iterations=n_iter))
    transform = (ctx.get_option('transform_ny'), ctx.get_option('transform_nx'))
    same_transform = []
    for f, model in enumerate(own):
        host = TemperedEnsembleSampler(n_w, fs.num_params, betas, fs.models[f].log_likelihood_and_prior_batch)
        host.random_state = np.random.RandomState(50 + f).get_state()
        want = list(host.sample(p0[f], iterations=n_iter))
        _assert_same_run(together.fields[f], host, f)
        for j, (a, b) in enumerate(zip([y[f] for y in yields], want)):
            for k in range(3):
                assert np.array_equal(a[k], b[k]), (f, j, k)
        assert host.nswap.sum() > 0 and np.all(host.naccepted_t.sum(axis=1) > 0), f
        eng = model.engine
        if (eng.get_option('transform_ny'), eng.get_option('transform_nx')) == transform:
            same_transform.append(f)
            solo = DeviceTemperedSampler(n_w, model, betas=betas, block=5)
            solo.random_state = np.random.RandomState(50 + f).get_state()
            want = list(solo.sample(p0[f], iterations=n_iter))
            _assert_same_run(together.fields[f], solo, f)
            _assert_same_yields([y[f] for y in yields], want, f)
        model.close()
    assert 1 in same_transform
    fs.close()


@pytest.mark.parametrize('stop', [3, 7, 10])
def test_resuming_from_a_yield(runs, set3, stop):
    """Inside a block, at a block edge and in the next block: the rest of the same chains."""
    from psfmc_amd import FieldSetTemperedSampler
    state = runs['yields'][stop - 1]
    again = FieldSetTemperedSampler(N_W, set3, betas=runs['betas'], block=BLOCK)
    for f, sub in enumerate(again.fields):
        sub.random_state = state[f][3]
    rest = list(again.sample([s[0] for s in state], [s[1] for s in state], [s[2] for s in state],
                             iterations=N_ITER - stop))
    for f, solo in enumerate(runs['solos']):
        assert np.array_equal(again.fields[f].chain, solo.chain[:, stop:]), f
        assert np.array_equal(again.fields[f].lnlikelihood, solo.lnlikelihood[:, :, stop:]), f
        assert np.array_equal(again.fields[f].lnprobability, solo.lnprobability[:, stop:]), f
        _assert_same_yields([y[f] for y in rest], runs['solo_yields'][f][stop:], f)


def test_one_rung_is_the_field_set_sampler(runs, set3):
    from psfmc_amd import FieldSetSampler, FieldSetTemperedSampler
    p0 = runs['p0'][:, :1]
    ref = FieldSetSampler(N_W, set3, block=6)
    one = FieldSetTemperedSampler(N_W, set3, betas=[1.0], block=5)
    for s in (ref, one):
        for f, sub in enumerate(s.fields):
            sub.random_state = np.random.RandomState(8 + f).get_state()
    list(ref.sample(p0[:, 0], iterations=14))
    list(one.sample(p0, iterations=14))
    for f in range(N_F):
        assert np.array_equal(one.fields[f].chain, ref.fields[f].chain), f
        assert np.array_equal(one.fields[f].lnprobability, ref.fields[f].lnprobability), f
        assert np.array_equal(one.fields[f].naccepted, ref.fields[f].naccepted), f
        assert ref.fields[f].naccepted.sum() > 0


def test_accumulation_of_every_fields_beta_one_rung(own3, set3):
    from psfmc_amd import FieldSetTemperedSampler
    from psfmc_amd.sampler import DeviceTemperedSampler
    n_t, n_w, n_iter = 3, 24, 6
    p0 = np.array([_square_start(fld, n_t, n_w, seed=9 + f) for f, (_, fld) in enumerate(own3)])
    for m in set3.models:
        m.reset_images()
    acc = FieldSetTemperedSampler(n_w, set3, ntemps=n_t, tmax=20.0, block=4, accumulate=True)
    for f, sub in enumerate(acc.fields):
        sub.random_state = np.random.RandomState(30 + f).get_state()
    list(acc.sample(p0, iterations=n_iter))
    for f, (model, _) in enumerate(own3):
        model.reset_images()
        solo = DeviceTemperedSampler(n_w, model, ntemps=n_t, tmax=20.0, block=4, accumulate=True)
        solo.random_state = np.random.RandomState(30 + f).get_state()
        list(solo.sample(p0[f], iterations=n_iter))
        assert np.array_equal(acc.fields[f].chain, solo.chain), f
        assert set3.models[f].accumulated_samples == model.accumulated_samples == n_w * n_iter
        want = model.collect_posterior_images()
        got = set3.models[f].collect_posterior_images()
        for kind, img in want.items():
            fin = np.isfinite(img)
            assert np.array_equal(np.isfinite(got[kind]), fin), (f, kind)
            assert np.abs(got[kind][fin] - img[fin]).max() <= 1e-12 * np.abs(img[fin]).max(), (f, kind)
        model.reset_images()
        set3.models[f].reset_images()


def _draws(n_iter, n_f, n_t, n_w, seed=0):
    """Valid random numbers of psfmc_pt_run_fields."""
    rs = np.random.RandomState(seed)
    half = n_w // 2
    z = 0.5 + rs.rand(n_iter, 2, n_f, n_t, half)
    partner = rs.randint(half, size=(n_iter, 2, n_f, n_t, half)).astype(np.int32)
    log_u = np.log(rs.rand(n_iter, 2, n_f, n_t, half))
    perms = lambda: np.array([[[rs.permutation(n_w) for _ in range(n_t - 1)] for _ in range(n_f)]
                              for _ in range(n_iter)]).astype(np.int32).reshape(n_iter, n_f, n_t - 1, n_w)
    si, sj = perms(), perms()
    slu = np.log(rs.rand(n_iter, n_f, n_t - 1, n_w))
    return [z, 9.0 * np.log(z), partner, log_u, si, sj, slu]


def test_refusals(own3, set3):
    from psfmc_amd import FieldSetTemperedSampler, JointModel
    from psfmc_amd.engine import NativeError
    betas = _ladder()
    with pytest.raises(ValueError, match='3 fields'):            # 3 x 4 x 24 = 288 > 264
        FieldSetTemperedSampler(24, set3, betas=betas)
    with pytest.raises(ValueError, match='even'):
        FieldSetTemperedSampler(21, set3, betas=betas)
    with pytest.raises(ValueError, match='last rung'):
        FieldSetTemperedSampler(22, set3, betas=[1.0, 0.5, 0.1])

    def run(ctx, betas, n_w, change=None, n_iter=2, n_f=N_F):
        n_t = len(betas)
        p0 = np.array([_square_start(own3[f][1], n_t, n_w, seed=1 + f) for f in range(n_f)])
        args = _draws(n_iter, n_f, n_t, n_w)
        if change:
            change(args)
        nacc = np.zeros((n_f, n_t, n_w), dtype=np.int64)
        nsw = np.zeros((n_f, n_t - 1), dtype=np.int64)
        return ctx.pt_run_fields(betas, p0, None, None, *args, naccepted=nacc, nswap=nsw), nacc, nsw

    ctx = set3.context
    with pytest.raises(NativeError, match=r'3 fields.*max_walkers=264') as err:
        run(ctx, betas, 24)
    assert err.value.code == EINVAL
    with pytest.raises(NativeError, match='even') as err:
        run(ctx, betas, 21)
    assert err.value.code == EINVAL
    with pytest.raises(NativeError, match='last rung') as err:   # a ladder not ending at 0
        run(ctx, np.array([1.0, 0.5, 0.25, 0.1]), 22)
    assert err.value.code == EINVAL

    def bad_partner(args):
        args[2][1, 1, 1, 3, 5] = 11                              # half = 11: one past the end, in field 1

    with pytest.raises(NativeError, match=r'partner index 11 .*field 1') as err:
        run(ctx, betas, 22, bad_partner)
    assert err.value.code == EINVAL

    def bad_swap(args):
        args[4][1, 2, 2, 0] = args[4][1, 2, 2, 1]                # the last field: not a permutation

    with pytest.raises(NativeError, match='permutations') as err:
        run(ctx, betas, 22, bad_swap)
    assert err.value.code == EINVAL
    # a context whose fields are one joint fit
    joint = JointModel([square_model(64, 1, 'fused', max_walkers=1, seed=s)[0] for s in range(2)],
                       max_walkers=2 * N_T * N_W)
    try:
        assert joint.num_params == set3.num_params
        with pytest.raises(NativeError, match='joint priors') as err:
            run(joint.context, betas, 22, n_f=2)
        assert err.value.code == EINVAL
    finally:
        joint.close()
    # the context evaluates and samples correctly afterwards
    (pos, ll, lp, chain, lnchain, llchain, lpchain), nacc, nsw = run(ctx, betas, 22, n_iter=4)
    assert nacc.sum() > 0 and nsw.sum() > 0 and np.isfinite(ll[:, 0]).all()
    again = set3.log_likelihood_and_prior_batch([p.reshape(-1, set3.num_params) for p in pos])
    for f in range(N_F):
        assert np.array_equal(again[f][0].reshape(ll[f].shape), ll[f]), f
        assert np.array_equal(again[f][1].reshape(lp[f].shape), lp[f]), f
        want = own3[f][0].log_likelihood_and_prior_batch(pos[f].reshape(-1, set3.num_params))
        assert np.array_equal(want[0].reshape(ll[f].shape), ll[f]), f
    assert np.array_equal(chain[:, :, :, -1], pos) and np.array_equal(llchain[:, :, :, -1], ll)
    assert np.array_equal(lnchain[:, :, -1], (betas[0] * ll + lp)[:, 0])


def test_model_fields_ptmcmc(tmp_path):
    from psfmc_amd import load_database, model_fields_ptmcmc, model_galaxy_ptmcmc
    n_f, chains, n_t = 2, 22, 4
    kinds = ('convolved_model', 'composite_ivm')
    own = [square_model(64, 1, 'fused', max_walkers=n_t * chains, seed=s) for s in range(n_f)]
    p0 = [_square_start(fld, n_t, chains, seed=5 + f) for f, (_, fld) in enumerate(own)]
    names = [str(tmp_path / ('t%d' % f)) for f in range(n_f)]

    def together():
        models = [square_model(64, 1, 'fused', max_walkers=1, seed=s)[0] for s in range(n_f)]
        return model_fields_ptmcmc(models, output_names=names, write_fits=kinds, iterations=10, burn=6,
                                   chains=chains, ntemps=n_t, tmax=50.0, random_states=[7 + f for f in range(n_f)],
                                   start_positions=p0, quiet=True)

    results = together()
    assert len(results) == n_f
    keys = ('MCNTEMPS', 'MCLNZ', 'MCLNZERR', 'MCTSWAP')
    for f, (model, _) in enumerate(own):
        # the one-field run from the same start: model_galaxy_ptmcmc draws every rung's start from numpy's global
        # generator, so the prior draws are replaced by the given positions, rung after rung
        rungs = iter(p0[f])
        model.init_params_from_priors = lambda n, it=rungs: next(it)
        _, db, (lnz, err) = model_galaxy_ptmcmc(model, output_name=str(tmp_path / ('s%d' % f)), write_fits=kinds,
                                                iterations=10, burn=6, chains=chains, ntemps=n_t, tmax=50.0,
                                                random_state=7 + f, quiet=True)
        m_t, tdb, (tlnz, terr) = results[f]
        assert tdb.colnames == db.colnames and len(tdb) == 10 * chains
        for name in db.colnames:
            assert np.array_equal(np.asarray(tdb[name]), np.asarray(db[name])), (f, name)
        for key in keys:
            assert tdb.meta[key] == db.meta[key], (f, key)
        assert (tlnz, terr) == (lnz, err) and np.isfinite(lnz)
        assert m_t.accumulated_samples == 10 * chains
        for kind in kinds:
            assert os.path.exists('{}_{}.fits'.format(names[f], kind)), (f, kind)
        model.close()
    for m, _, _ in results:
        m.close()
    # a second call does not sample again: the databases stay, the evidences come from their headers
    mtimes = [os.path.getmtime(n + '_db.fits') for n in names]
    second = together()
    assert [os.path.getmtime(n + '_db.fits') for n in names] == mtimes
    for f in range(n_f):
        stored = load_database(names[f] + '_db.fits')
        assert second[f][2] == pytest.approx(results[f][2])
        assert second[f][2][0] == pytest.approx(stored.meta['MCLNZ'])
        assert np.array_equal(second[f][1]['lnprobability'], results[f][1]['lnprobability'])
        second[f][0].close()
