"""A JointModel -- one model fitted jointly to several exposures, some parameters shared and some per field --
on the device: its log-posterior against the oracle's per-field log-likelihoods plus the scipy prior, the
-inf rules, batch independence, the one-field and the same-exposure-twice cases, the device sampler against
the host sampler (posterior images included), model_joint_mcmc, and the capacity check."""
import os

import numpy as np
import pytest

import helpers
import psfmc_oracle as orc
from test_joint_link import MAG_ZP, POS, SHAPES, make_field, make_model

pytestmark = pytest.mark.gpu

LAYOUT = helpers.synth_layout(1)


def _oracle_field(fld):
    return orc.make_field(fld['sci'], fld['ivm'], fld['psfs'], fld['pivms'], mag_zp=MAG_ZP)


def _joint_truth(joint, flds):
    """The joint vector holding every field's truth (the shared values are the same in every truth)."""
    t = np.zeros(joint.num_params)
    for f, fld in enumerate(flds):
        t[joint.field_columns(f)] = fld['truth']
    return t


def _col(joint, name):
    """The first joint column of parameter `name`."""
    return sum(joint.param_lens[:joint.param_names.index(name)])


def _thetas(joint, flds, n, seed):
    """n joint walkers near the truth, both PSFs in every field."""
    rng = np.random.RandomState(seed)
    out = _joint_truth(joint, flds) + rng.normal(size=(n, joint.num_params)) * 1e-2
    for f in range(len(flds)):
        out[:, _col(joint, 'PSF_Index_f%d' % f)] = rng.randint(0, 2, n)
    ir, ib = _col(joint, '1_Sersic_reff'), _col(joint, '1_Sersic_reff_b')
    out[:, ib] = np.minimum(out[:, ib], out[:, ir] - 1e-3)
    return out


@pytest.fixture(scope='module')
def joint3():
    from psfmc_amd import JointModel
    flds = [make_field(ny, nx, pk, seed=30 + f) for f, (ny, nx, pk) in enumerate(SHAPES)]
    joint = JointModel([make_model(fld) for fld in flds], per_field=POS, max_walkers=3 * 64)
    yield flds, joint
    joint.close()


def test_joint_log_posterior_against_the_oracle(joint3):
    flds, joint = joint3
    theta = _thetas(joint, flds, 20, seed=5)
    col = lambda name: _col(joint, name)
    cs = col('1_Sersic_xy_f1')
    ir, ib = col('1_Sersic_reff'), col('1_Sersic_reff_b')
    theta[16, col('1_Sersic_mag')] = 30.0                       # a shared parameter out of support
    theta[17, col('0_PointSource_mag_f1')] = 10.0               # field 1's parameter out of support
    theta[18, ib] = theta[18, ir] + 0.5                         # reff_b > reff
    theta[19, cs:cs + 2] = (56.0, 50.0)                         # field 1's Sersic centre on a pixel centre
    got = joint.log_posterior_batch(theta)
    prior = joint.log_priors_batch(theta)
    fields = [_oracle_field(fld) for fld in flds]
    for w in range(len(theta)):
        if w in (16, 17, 18):
            assert not np.isfinite(prior[w]) and got[w] == -np.inf, w
            continue
        lls = [helpers.oracle_loglike(fields[f], LAYOUT, joint.field_theta(theta[w], f)[0], has_psf_index=True)
               for f in range(3)]
        if w == 19:
            assert np.isfinite(prior[w]) and not np.isfinite(lls[1]) and np.isfinite([lls[0], lls[2]]).all()
            assert got[w] == -np.inf
            continue
        want = prior[w] + sum(lls)
        assert abs(got[w] - want) <= 1e-11 * (abs(prior[w]) + sum(abs(v) for v in lls)), (w, got[w], want)


def test_walker_values_do_not_depend_on_the_batch():
    from psfmc_amd import JointModel
    flds = [make_field(ny, nx, pk, seed=30 + f) for f, (ny, nx, pk) in enumerate(SHAPES)]
    joint = JointModel([make_model(fld) for fld in flds], per_field=POS, max_walkers=3 * 40)
    joint.engine.set_option('chunk_walkers', 24)                # 3 x 40 field records: five passes
    theta = _thetas(joint, flds, 40, seed=9)
    full = joint.log_posterior_batch(theta)
    assert np.isfinite(full).all()
    lib, ctx = joint.context._lib, joint.context._ctx
    assert lib.psfmc_pass_size(ctx, 3 * 40) < 3 * 40
    for w in (0, 7, 39):
        assert np.array_equal(joint.log_posterior_batch(theta[w:w + 1]), full[w:w + 1]), w
    assert np.array_equal(joint.log_posterior_batch(theta[5:14]), full[5:14])
    perm = np.random.RandomState(1).permutation(40)
    assert np.array_equal(joint.log_posterior_batch(theta[perm]), full[perm])
    joint.close()


def test_one_field_equals_its_own_model():
    from psfmc_amd import JointModel
    fld = make_field(128, 128, 21, seed=33)
    own = make_model(fld, max_walkers=64)
    joint = JointModel([make_model(fld)], max_walkers=64)
    assert joint.num_params == own.num_params
    theta = _thetas(joint, [fld], 24, seed=2)
    theta[3, _col(joint, '1_Sersic_mag')] = 30.0
    got, want = joint.log_posterior_batch(theta), own.log_posterior_batch(theta)
    assert np.isfinite(want).sum() == 23
    assert np.array_equal(got, want)
    own.close()
    joint.close()


def test_the_same_exposure_twice():
    from psfmc_amd import JointModel
    fld = make_field(*SHAPES[0], seed=30)
    own = make_model(fld, max_walkers=32)
    joint = JointModel([make_model(fld), make_model(fld)], max_walkers=64)
    assert joint.param_names[-2:] == ['PSF_Index_f0', 'PSF_Index_f1']
    theta = _thetas(joint, [fld, fld], 16, seed=4)
    theta[:, -1] = theta[:, -2]                                  # the same PSF in both copies
    got = joint.log_posterior_batch(theta)
    own_theta = joint.field_theta(theta, 0)
    ll = own.log_posterior_batch(own_theta) - own.log_priors_batch(own_theta)
    want = joint.log_priors_batch(theta) + 2 * ll
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    own.close()
    joint.close()


@pytest.mark.parametrize('n_w', [32, 22])
def test_device_sampler_equals_the_host_sampler(joint3, n_w):
    from psfmc_amd import DeviceEnsembleSampler, EnsembleSampler
    flds, joint = joint3
    p0 = _joint_truth(joint, flds) + np.random.RandomState(n_w).normal(size=(n_w, joint.num_params)) * 1e-3
    for f in range(3):
        p0[:, _col(joint, 'PSF_Index_f%d' % f)] = np.arange(n_w) % 2
    for m in joint.field_models:
        m.reset_images()
    dev = DeviceEnsembleSampler(n_w, joint, live_dangerously=True, block=8, accumulate=True)
    dev.random_state = np.random.RandomState(700 + n_w).get_state()
    for _ in dev.sample(p0, iterations=30):
        pass
    host = EnsembleSampler(n_w, joint.num_params, batch_lnpostfn=joint.log_posterior_batch, live_dangerously=True)
    host.random_state = np.random.RandomState(700 + n_w).get_state()
    for _ in host.sample(p0, iterations=30):
        pass
    assert np.array_equal(dev.chain, host.chain)
    assert np.array_equal(dev.lnprobability, host.lnprobability)
    assert np.array_equal(dev.naccepted, host.naccepted)
    assert host.naccepted.sum() > 0
    # every field's posterior images: the positions after every iteration, mapped to the field
    flat = dev.chain.transpose(1, 0, 2).reshape(-1, joint.num_params)
    for f, m in enumerate(joint.field_models):
        assert m.accumulated_samples == 30 * n_w
        got = {k: v.copy() for k, v in m.collect_posterior_images().items()}
        m.reset_images()
        m.accumulate_samples(joint.field_theta(flat, f))
        want = m.collect_posterior_images()
        for kind, img in want.items():
            assert img.shape == SHAPES[f][:2], (f, kind)
            fin = np.isfinite(img)
            assert np.array_equal(fin, np.isfinite(got[kind])), (f, kind)
            scale = np.abs(img[fin]).max()
            assert np.abs(got[kind][fin] - img[fin]).max() <= 1e-12 * scale, (f, kind)
        m.reset_images()


def test_device_sampler_proposes_in_a_second_workgroup():
    """The joint proposal kernel has one lane per proposal in workgroups of 64: with 132 walkers a half-step is
    66 proposals, two of them in a second workgroup.  Two fields, six iterations in blocks of four, no image
    sums; the chain, the log-posteriors and the counters are the host sampler's, bit for bit."""
    from psfmc_amd import DeviceEnsembleSampler, EnsembleSampler, JointModel
    n_w, n_iter = 132, 6
    flds = [make_field(ny, nx, pk, seed=30 + f) for f, (ny, nx, pk) in enumerate(SHAPES[:2])]
    joint = JointModel([make_model(fld) for fld in flds], per_field=POS, max_walkers=2 * n_w)
    try:
        p0 = _joint_truth(joint, flds) + np.random.RandomState(n_w).normal(size=(n_w, joint.num_params)) * 1e-3
        for f in range(2):
            p0[:, _col(joint, 'PSF_Index_f%d' % f)] = np.arange(n_w) % 2
        dev = DeviceEnsembleSampler(n_w, joint, live_dangerously=True, block=4)
        dev.random_state = np.random.RandomState(700 + n_w).get_state()
        for _ in dev.sample(p0, iterations=n_iter):
            pass
        host = EnsembleSampler(n_w, joint.num_params, batch_lnpostfn=joint.log_posterior_batch, live_dangerously=True)
        host.random_state = np.random.RandomState(700 + n_w).get_state()
        for _ in host.sample(p0, iterations=n_iter):
            pass
        assert np.array_equal(dev.chain, host.chain)
        assert np.array_equal(dev.lnprobability, host.lnprobability)
        assert np.array_equal(dev.naccepted, host.naccepted)
        # the second workgroup's lanes
        assert host.naccepted[n_w // 2 - 2:n_w // 2].sum() + host.naccepted[-2:].sum() > 0
    finally:
        joint.close()


def test_model_joint_mcmc(tmp_path):
    from psfmc_amd import load_database, model_joint_mcmc
    from psfmc_amd import fits_io
    shapes = [(96, 96, 11), (100, 100, 13)]
    flds = [make_field(ny, nx, pk, seed=90 + f) for f, (ny, nx, pk) in enumerate(shapes)]
    out = str(tmp_path / 'jfit')
    kinds = ('raw_model', 'convolved_model', 'composite_ivm', 'residual', 'point_source_subtracted')
    joint, db = model_joint_mcmc([make_model(fld) for fld in flds], per_field=POS, output_name=out, iterations=6,
                                 burn=2, convergence_check=lambda s, verbose=0: True, random_state=11, quiet=True)
    assert db.colnames == joint.param_names + ['lnprobability', 'walker', 'sample']
    assert db.meta['MCFIELDS'] == 2 and db.meta['MCCHAINS'] == 2 * joint.num_params + 2
    assert len(db) == 6 * (2 * joint.num_params + 2)
    assert load_database(out + '_db.fits').colnames == db.colnames
    first = {}
    for f, (ny, nx, _) in enumerate(shapes):
        for kind in kinds:
            img = fits_io.read_image('{}_f{}_{}.fits'.format(out, f, kind))
            assert img.shape == (ny, nx), (f, kind)
            first[f, kind] = np.array(img, dtype=np.float64)
    joint.close()
    for path in first:
        os.remove('{}_f{}_{}.fits'.format(out, *path))
    mtime = os.path.getmtime(out + '_db.fits')
    joint2, db2 = model_joint_mcmc([make_model(fld) for fld in flds], per_field=POS, output_name=out,
                                   iterations=6, burn=2, quiet=True)
    assert os.path.getmtime(out + '_db.fits') == mtime
    assert np.array_equal(db2['lnprobability'], db['lnprobability'])
    for (f, kind), img in first.items():
        again = np.array(fits_io.read_image('{}_f{}_{}.fits'.format(out, f, kind)), dtype=np.float64)
        assert np.abs(again - img).max() <= 1e-12 * np.abs(img).max(), (f, kind)
    joint2.close()


def test_capacity_is_checked(joint3):
    from psfmc_amd.engine import NativeError
    flds, joint = joint3
    eng = joint.engine                                           # 3 fields, max_walkers = 192: W <= 64
    theta = _thetas(joint, flds, 65, seed=3)
    with pytest.raises(NativeError, match='max_walkers=192'):
        eng.logpost_theta(theta)
    assert np.isfinite(eng.logpost_theta(theta[:64])).all()
    n_w = 66
    z = np.ones((1, 2, n_w // 2))
    with pytest.raises(NativeError, match='max_walkers=192'):
        eng.stretch_run(theta[:1].repeat(n_w, 0), None, z, z * 0, np.zeros((1, 2, n_w // 2), dtype=np.int32),
                        z * 0, np.zeros(n_w, dtype=np.int64))
