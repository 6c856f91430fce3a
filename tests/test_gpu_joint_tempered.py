"""Parallel tempering of a JointModel on the device (psfmc_eval_theta_joint_split, psfmc_pt_run_joint,
DeviceTemperedSampler on a JointModel, model_joint_ptmcmc): the split evaluation against the joint log-posterior,
the scipy prior and the oracle's per-field log-likelihoods; the device sampler against its host contract bit for
bit; one rung against the joint stretch sampler; one field against its own model; the beta = 1 rung's posterior
images; the refusals; the evidence against quadrature; and the entry point.

Two fields of unequal image and PSF sides, the positions per field: field-major records and per-field sides
are where an index error shows."""
import os

import numpy as np
import pytest

import helpers
import synth_field
from test_gpu_joint import LAYOUT, _col, _joint_truth, _oracle_field, _thetas
from test_gpu_tempered import EVIDENCE_FLOOR_2D, _logsumexp, _write_field, _write_model
from test_joint_link import POS, make_field, make_model

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64, 11), (64, 96, 13)]
MAX_WALKERS = 4 * 40 * 2                     # the largest case: 4 rungs x 40 walkers x 2 fields


def _fields():
    return [make_field(ny, nx, pk, seed=60 + f) for f, (ny, nx, pk) in enumerate(SHAPES)]


@pytest.fixture(scope='module')
def joint2():
    from psfmc_amd import JointModel
    flds = _fields()
    joint = JointModel([make_model(fld) for fld in flds], per_field=POS, max_walkers=MAX_WALKERS)
    yield flds, joint
    joint.close()


def _ladder_start(joint, flds, n_t, n_w, seed):
    """[T, W, P]: rung 0 near the truth, the hotter rungs drawn from the priors."""
    p0 = np.empty((n_t, n_w, joint.num_params))
    p0[0] = _joint_truth(joint, flds) + np.random.RandomState(seed).normal(size=(n_w, joint.num_params)) * 1e-3
    for f in range(len(flds)):
        p0[0, :, _col(joint, 'PSF_Index_f%d' % f)] = np.arange(n_w) % 2
    np.random.seed(seed)
    for t in range(1, n_t):
        p0[t] = joint.init_params_from_priors(n_w)
    return p0


def test_split_evaluation(joint2):
    flds, joint = joint2
    theta = _thetas(joint, flds, 24, seed=5)
    col = lambda name: _col(joint, name)
    cs = col('1_Sersic_xy_f1')
    ir, ib = col('1_Sersic_reff'), col('1_Sersic_reff_b')
    theta[20, col('1_Sersic_mag')] = 30.0                       # a shared parameter out of support
    theta[21, col('0_PointSource_mag_f1')] = 10.0               # field 1's parameter out of support
    theta[22, ib] = theta[22, ir] + 0.5                         # reff_b > reff
    theta[23, cs:cs + 2] = (48.0, 32.0)                         # field 1's Sersic centre on a pixel centre
    ll, lp = joint.log_likelihood_and_prior_batch(theta)
    post = joint.log_posterior_batch(theta)
    fin = np.isfinite(post)
    assert fin.sum() == 20 and not fin[20:].any()
    assert np.array_equal(ll[fin] + lp[fin], post[fin])
    assert np.all(ll[~fin] == -np.inf)
    assert np.all(lp[20:23] == -np.inf) and np.isfinite(lp[23])
    prior = joint.log_priors_batch(theta)
    assert np.array_equal(np.isfinite(prior), np.isfinite(lp))
    fields = [_oracle_field(fld) for fld in flds]
    for w in range(20):
        lls = [helpers.oracle_loglike(fields[f], LAYOUT, joint.field_theta(theta[w], f)[0], has_psf_index=True)
               for f in range(2)]
        bound = 1e-11 * (abs(prior[w]) + sum(abs(v) for v in lls))
        assert abs(lp[w] - prior[w]) <= bound, (w, lp[w], prior[w])
        assert abs(ll[w] - sum(lls)) <= bound, (w, ll[w], sum(lls))
    assert abs(lp[23] - prior[23]) <= 1e-11 * abs(prior[23])
    lls = [helpers.oracle_loglike(fields[f], LAYOUT, joint.field_theta(theta[23], f)[0], has_psf_index=True)
           for f in range(2)]
    assert np.isfinite(lls[0]) and not np.isfinite(lls[1])
    # the values do not depend on the batch: 48 field records in three passes
    eng = joint.engine
    chunk = eng.get_option('chunk_walkers')
    eng.set_option('chunk_walkers', 20)
    try:
        lib, ctx = joint.context._lib, joint.context._ctx
        assert lib.psfmc_pass_size(ctx, 2 * 24) < 2 * 24
        for got, want in zip(joint.log_likelihood_and_prior_batch(theta), (ll, lp)):
            assert np.array_equal(got, want)
        for w in (0, 7, 19, 23):
            for got, want in zip(joint.log_likelihood_and_prior_batch(theta[w:w + 1]), (ll, lp)):
                assert np.array_equal(got, want[w:w + 1]), w
        perm = np.random.RandomState(1).permutation(24)
        for got, want in zip(joint.log_likelihood_and_prior_batch(theta[perm]), (ll, lp)):
            assert np.array_equal(got, want[perm])
    finally:
        eng.set_option('chunk_walkers', chunk)


# (a) half = 11: odd and smaller than a wave.  (b) T half = 80 crosses the 64-lane workgroup of the proposal
# kernel with a rung boundary inside a workgroup; chunk_walkers = 48 makes a half-step's 160 records four passes
@pytest.mark.parametrize('n_w, chunk', [(22, None), (40, 48)])
def test_device_tempered_sampler_reproduces_the_host_contract(joint2, n_w, chunk):
    from psfmc_amd.sampler import TemperedEnsembleSampler, DeviceTemperedSampler, default_betas
    flds, joint = joint2
    n_t = 4
    betas = default_betas(n_t, 50.0)
    p0 = _ladder_start(joint, flds, n_t, n_w, seed=n_w)
    eng = joint.engine
    before = eng.get_option('chunk_walkers')
    if chunk:
        eng.set_option('chunk_walkers', chunk)
    try:
        if chunk:
            lib, ctx = joint.context._lib, joint.context._ctx
            assert lib.psfmc_pass_size(ctx, n_t * (n_w // 2) * 2) < n_t * (n_w // 2) * 2
        host = TemperedEnsembleSampler(n_w, joint.num_params, betas, joint.log_likelihood_and_prior_batch)
        dev = DeviceTemperedSampler(n_w, joint, betas=betas, block=7)
        for s in (host, dev):
            s.random_state = np.random.RandomState(11).get_state()
        out_h = list(host.sample(p0, iterations=16))
        out_d = list(dev.sample(p0, iterations=16))
        assert np.array_equal(dev.chain, host.chain)
        assert np.array_equal(dev.lnprobability, host.lnprobability)
        assert np.array_equal(dev.lnlikelihood, host.lnlikelihood)
        assert np.array_equal(dev.naccepted_t, host.naccepted_t) and np.array_equal(dev.nswap, host.nswap)
        assert dev.nswap.sum() > 0 and np.all(dev.naccepted_t.sum(axis=1) > 0)
        for a, b in zip(out_d[-1], out_h[-1]):
            if isinstance(a, np.ndarray):
                assert np.array_equal(a, b)
        # resuming from a yield inside a block, at a block edge and in the next block continues the same chain
        for stop in (3, 7, 10):
            pos, ll, lp, rstate = out_d[stop - 1]
            again = DeviceTemperedSampler(n_w, joint, betas=betas, block=7)
            list(again.sample(pos, ll, lp, rstate0=rstate, iterations=16 - stop))
            assert np.array_equal(again.chain, host.chain[:, stop:]), stop
            assert np.array_equal(again.lnlikelihood, host.lnlikelihood[:, :, stop:]), stop
    finally:
        eng.set_option('chunk_walkers', before)


def test_one_rung_is_the_joint_stretch_sampler(joint2):
    from psfmc_amd.sampler import DeviceEnsembleSampler, DeviceTemperedSampler
    flds, joint = joint2
    p0 = _ladder_start(joint, flds, 1, 22, seed=4)
    ref = DeviceEnsembleSampler(22, joint, live_dangerously=True, block=6)
    one = DeviceTemperedSampler(22, joint, betas=[1.0], block=5)
    for s in (ref, one):
        s.random_state = np.random.RandomState(8).get_state()
    list(ref.sample(p0[0], iterations=14))
    list(one.sample(p0, iterations=14))
    assert np.array_equal(one.chain, ref.chain)
    assert np.array_equal(one.lnprobability, ref.lnprobability)
    assert np.array_equal(one.naccepted, ref.naccepted)
    assert ref.naccepted.sum() > 0


def test_one_field_equals_its_own_model():
    from psfmc_amd import JointModel
    from psfmc_amd.sampler import DeviceTemperedSampler, default_betas
    fld = make_field(*SHAPES[1], seed=61)
    n_t, n_w = 4, 24
    own = make_model(fld, max_walkers=n_t * n_w)
    joint = JointModel([make_model(fld)], max_walkers=n_t * n_w)
    assert joint.num_params == own.num_params
    theta = _thetas(joint, [fld], 24, seed=2)
    theta[3, _col(joint, '1_Sersic_mag')] = 30.0
    ll_j, lp_j = joint.log_likelihood_and_prior_batch(theta)
    ll_o, lp_o = own.log_likelihood_and_prior_batch(theta)
    assert np.isfinite(ll_o).sum() == 23
    assert np.array_equal(ll_j, ll_o)
    assert np.array_equal(lp_j, lp_o)
    betas = default_betas(n_t, 50.0)
    p0 = _ladder_start(joint, [fld], n_t, n_w, seed=6)
    chains = []
    for model in (joint, own):
        s = DeviceTemperedSampler(n_w, model, betas=betas, block=5)
        s.random_state = np.random.RandomState(9).get_state()
        list(s.sample(p0, iterations=12))
        chains.append((s.chain, s.lnprobability, s.lnlikelihood, s.naccepted_t, s.nswap))
    for a, b in zip(*chains):
        assert np.array_equal(a, b)
    assert chains[0][4].sum() > 0
    own.close()
    joint.close()


def test_accumulation_of_the_beta_one_rung(joint2):
    from psfmc_amd.sampler import DeviceTemperedSampler
    flds, joint = joint2
    p0 = _ladder_start(joint, flds, 3, 24, seed=5)
    joint.reset_images()
    acc = DeviceTemperedSampler(24, joint, ntemps=3, tmax=20.0, block=4, accumulate=True)
    acc.random_state = np.random.RandomState(3).get_state()
    steps = list(acc.sample(p0, iterations=6))
    cold = np.concatenate([pos[0] for pos, _, _, _ in steps])
    for f, m in enumerate(joint.field_models):
        assert m.accumulated_samples == 6 * 24
        got = {k: v.copy() for k, v in m.collect_posterior_images().items()}
        m.reset_images()
        m.accumulate_samples(joint.field_theta(cold, f))
        want = m.collect_posterior_images()
        for kind, img in want.items():
            assert img.shape == SHAPES[f][:2], (f, kind)
            fin = np.isfinite(img)
            assert np.array_equal(fin, np.isfinite(got[kind])), (f, kind)
            scale = np.abs(img[fin]).max()
            assert np.abs(got[kind][fin] - img[fin]).max() <= 1e-12 * scale, (f, kind)
        m.reset_images()


def _draws(n_iter, n_t, n_w, seed=0):
    """Valid random numbers of psfmc_pt_run_joint."""
    rs = np.random.RandomState(seed)
    half = n_w // 2
    z = 0.5 + rs.rand(n_iter, 2, n_t, half)
    partner = rs.randint(half, size=(n_iter, 2, n_t, half)).astype(np.int32)
    log_u = np.log(rs.rand(n_iter, 2, n_t, half))
    si = np.stack([[rs.permutation(n_w) for _ in range(n_t - 1)] for _ in range(n_iter)]).astype(np.int32)
    sj = np.stack([[rs.permutation(n_w) for _ in range(n_t - 1)] for _ in range(n_iter)]).astype(np.int32)
    slu = np.log(rs.rand(n_iter, n_t - 1, n_w))
    return [z, np.log(z), partner, log_u, si, sj, slu]


def test_refusals(joint2):
    from psfmc_amd import JointModel, engine
    from psfmc_amd.engine import NativeError
    from psfmc_amd.sampler import DeviceTemperedSampler, default_betas
    flds, joint = joint2
    EINVAL = -1                                                  # include/psfmc_hip.h PSFMC_EINVAL
    betas = default_betas(4, 50.0)
    # capacity: 4 rungs x 42 walkers x 2 fields = 336 > 320
    with pytest.raises(ValueError, match='F=2'):
        DeviceTemperedSampler(42, joint, betas=betas)
    ctx = joint.context

    def run(ctx, betas, n_w, change=None, n_iter=2):
        n_t = len(betas)
        p0 = _ladder_start(joint, flds, n_t, n_w, seed=1)
        args = _draws(n_iter, n_t, n_w)
        if change:
            change(args)
        nacc, nsw = np.zeros((n_t, n_w), dtype=np.int64), np.zeros(n_t - 1, dtype=np.int64)
        return ctx.pt_run_joint(betas, p0, None, None, *args, naccepted=nacc, nswap=nsw), nacc, nsw

    with pytest.raises(NativeError, match=r'2 fields.*max_walkers=320') as err:
        run(ctx, betas, 42)
    assert err.value.code == EINVAL
    with pytest.raises(NativeError, match='last rung') as err:   # a ladder not ending at 0
        run(ctx, np.array([1.0, 0.5, 0.25, 0.1]), 22)
    assert err.value.code == EINVAL

    def bad_partner(args):
        args[2][1, 1, 3, 5] = 11                                 # half = 11: one past the end

    with pytest.raises(NativeError, match='partner index 11') as err:
        run(ctx, betas, 22, bad_partner)
    assert err.value.code == EINVAL

    def bad_swap(args):
        args[4][1, 2, 0] = args[4][1, 2, 1]                      # not a permutation

    with pytest.raises(NativeError, match='permutations') as err:
        run(ctx, betas, 22, bad_swap)
    assert err.value.code == EINVAL
    with pytest.raises(NativeError, match='even') as err:
        run(ctx, betas, 21)
    assert err.value.code == EINVAL
    # a fields context whose layouts are registered but not its joint priors
    other = JointModel([make_model(fld) for fld in flds], per_field=POS, max_walkers=MAX_WALKERS)
    fields = []
    for m in other.field_models:
        sel = m.config.psf_selector
        fields.append((m.config.obs_data, m.config.obs_var, m.config.bad_px, np.stack(sel.psf_data),
                       np.stack(sel.psf_var)))
    bare = engine.FieldSetContext(fields, n_ps=1, n_sersic=1, max_walkers=MAX_WALKERS)
    try:
        for f, m in enumerate(other.field_models):
            m._register_layout(bare.layout_of(f), columns=other.field_columns(f), n_params=other.num_params)
        with pytest.raises(NativeError, match='psfmc_set_joint_priors') as err:
            run(bare, betas, 22)
        assert err.value.code == EINVAL
        with pytest.raises(NativeError, match='psfmc_set_joint_priors') as err:
            bare.eval_joint_split(_thetas(joint, flds, 4, seed=1))
        assert err.value.code == EINVAL
    finally:
        bare.close()
    # the context evaluates and samples correctly afterwards
    theta = _thetas(joint, flds, 12, seed=8)
    ll, lp = joint.log_likelihood_and_prior_batch(theta)
    assert np.isfinite(ll).all() and np.array_equal(ll + lp, joint.log_posterior_batch(theta))
    (pos, ll, lp, chain, lnchain, llchain, lpchain), nacc, nsw = run(ctx, betas, 22, n_iter=4)
    assert nacc.sum() > 0 and np.isfinite(ll[0]).all()
    again = joint.log_likelihood_and_prior_batch(pos.reshape(-1, joint.num_params))
    assert np.array_equal(again[0].reshape(ll.shape), ll) and np.array_equal(again[1].reshape(lp.shape), lp)
    assert np.array_equal(chain[:, :, -1], pos) and np.array_equal(llchain[:, :, -1], ll)


def test_evidence_against_quadrature(tmp_path):
    """The same 64 x 64 exposure twice, two free shared parameters (point-source magnitude, sky level),
    everything else constant, one PSF: ln Z by quadrature of the joint posterior over +-10 sigma of the beta = 1
    posterior against log_evidence()."""
    from psfmc_amd import JointModel
    from psfmc_amd.sampler import DeviceTemperedSampler, default_betas
    fld = synth_field.make_field(64, n_sersic=0, seed=3)
    _write_field(tmp_path, fld)
    x, y = float(fld['truth'][1]), float(fld['truth'][2])
    text = '\n'.join([
        'from numpy import array',
        "Configuration(obs_file='sci.fits', obsivm_file='ivm.fits', psf_files='psf.fits',",
        "              psfivm_files='psf_ivm.fits', mag_zeropoint={!r})".format(fld['mag_zp']),
        'Sky(adu=Uniform(loc=-0.01, scale=0.02))',
        'PointSource(xy=array(({!r}, {!r})), mag=Uniform(loc=18.0, scale=2.0))'.format(x, y),
    ]) + '\n'
    n_t, n_w = 24, 16
    path = _write_model(tmp_path, 'model2.py', text)
    joint = JointModel([path, path], max_walkers=n_t * n_w * 2)
    assert joint.num_params == 2 and len(joint.field_models) == 2
    rs = np.random.RandomState(0)
    np.random.seed(0)
    p0 = np.stack([joint.init_params_from_priors(n_w) for _ in range(n_t)])
    s = DeviceTemperedSampler(n_w, joint, betas=default_betas(n_t, 1e7), block=64)
    s.random_state = rs.get_state()
    for _ in s.sample(p0, iterations=800):
        pass
    lnz, err = s.log_evidence(0.25)
    post = s.chain[:, 200:].reshape(-1, 2)
    mu, sd = post.mean(axis=0), post.std(axis=0)
    grids = [np.linspace(m - 10 * d, m + 10 * d, 161) for m, d in zip(mu, sd)]
    gx, gy = np.meshgrid(*grids, indexing='ij')
    theta = np.stack([gx.ravel(), gy.ravel()], axis=1)
    lnpost = joint.log_posterior_batch(theta)
    cell = (grids[0][1] - grids[0][0]) * (grids[1][1] - grids[1][0])
    exact = _logsumexp(lnpost) + np.log(cell)
    print('lnZ', lnz, 'exact', exact, 'err', err)
    assert abs(lnz - exact) <= max(3 * err, EVIDENCE_FLOOR_2D), (lnz, exact, err)
    joint.close()


def test_model_joint_ptmcmc(tmp_path):
    from psfmc_amd import fits_io, load_database, model_joint_ptmcmc
    flds = _fields()
    out = str(tmp_path / 'jpt')
    kinds = ('raw_model', 'convolved_model', 'composite_ivm', 'residual', 'point_source_subtracted')
    np.random.seed(42)
    joint, db, (lnz, err) = model_joint_ptmcmc([make_model(fld) for fld in flds], per_field=POS, output_name=out,
                                               iterations=6, burn=2, ntemps=3, tmax=100.0, random_state=11,
                                               quiet=True)
    chains = 2 * joint.num_params + 2
    assert joint._max_walkers >= 3 * chains * 2
    assert db.colnames == joint.param_names + ['lnprobability', 'walker', 'sample']
    assert len(db) == 6 * chains
    db2 = load_database(out + '_db.fits')
    assert db2.colnames == db.colnames and len(db2) == len(db)
    assert db2.meta['MCFIELDS'] == 2 and db2.meta['MCNTEMPS'] == 3 and db2.meta['MCCHAINS'] == chains
    assert np.isfinite(db2.meta['MCLNZ']) and db2.meta['MCLNZERR'] >= 0 and 0 <= db2.meta['MCTSWAP'] <= 1
    assert db2.meta['MCLNZ'] == pytest.approx(lnz) and np.isfinite(err)
    theta = db2.param_matrix(joint.param_names)
    again = joint.log_posterior_batch(theta[::7])
    assert helpers.rel_err(again, db2['lnprobability'][::7]) <= 1e-12
    for m in joint.field_models:
        assert m.accumulated_samples == 6 * chains
    for f, (ny, nx, _) in enumerate(SHAPES):
        for kind in kinds:
            assert fits_io.read_image('{}_f{}_{}.fits'.format(out, f, kind)).shape == (ny, nx), (f, kind)
    joint.close()
    # a second call does not sample again: the database stays, the evidence comes from its header
    mtime = os.path.getmtime(out + '_db.fits')
    joint2, db3, (lnz2, err2) = model_joint_ptmcmc([make_model(fld) for fld in flds], per_field=POS,
                                                   output_name=out, iterations=6, burn=2, ntemps=3, tmax=100.0,
                                                   quiet=True)
    assert os.path.getmtime(out + '_db.fits') == mtime
    assert np.array_equal(db3['lnprobability'], db['lnprobability'])
    assert lnz2 == pytest.approx(lnz) and err2 == pytest.approx(err)
    joint2.close()
