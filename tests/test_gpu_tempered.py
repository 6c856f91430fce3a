"""The parallel-tempered device sampler (psfmc_pt_run, DeviceTemperedSampler) against its host contract
(TemperedEnsembleSampler driven by the device's own lnL / lnprior), against the stretch-move device sampler at
T = 1, the posterior images of its beta = 1 rung, the evidence against quadrature, a model comparison and the
model_galaxy_ptmcmc entry point."""
import os
import shutil

import numpy as np
import pytest

import helpers
import synth_field

pytestmark = pytest.mark.gpu


def _synth_model(tmp_path, max_walkers):
    case = helpers.load_case('synth128x2')
    return helpers.build_model('synth128x2', case, tmp_path, max_walkers=max_walkers)


def test_device_tempered_sampler_reproduces_the_host_contract(tmp_path):
    from psfmc_amd.sampler import TemperedEnsembleSampler, DeviceTemperedSampler, default_betas
    model = _synth_model(tmp_path, 160)
    betas = default_betas(4, 50.0)
    np.random.seed(2)
    p0 = np.stack([model.init_params_from_priors(40) for _ in range(4)])
    host = TemperedEnsembleSampler(40, model.num_params, betas, model.log_likelihood_and_prior_batch)
    dev = DeviceTemperedSampler(40, model, betas=betas, block=7)
    for s in (host, dev):
        s.random_state = np.random.RandomState(11).get_state()
    out_h = list(host.sample(p0, iterations=16))
    out_d = list(dev.sample(p0, iterations=16))
    assert np.array_equal(dev.chain, host.chain)
    assert np.array_equal(dev.lnprobability, host.lnprobability)
    assert np.array_equal(dev.lnlikelihood, host.lnlikelihood)
    assert np.array_equal(dev.naccepted_t, host.naccepted_t) and np.array_equal(dev.nswap, host.nswap)
    assert dev.nswap.sum() > 0 and 0.0 < dev.acceptance_fraction.mean() < 1.0
    for a, b in zip(out_d[-1], out_h[-1]):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, b)
    # resuming from a yield inside a block, at a block edge and in the next block continues the same chain
    for stop in (3, 7, 10):
        pos, ll, lp, rstate = out_d[stop - 1]
        again = DeviceTemperedSampler(40, model, betas=betas, block=7)
        list(again.sample(pos, ll, lp, rstate0=rstate, iterations=16 - stop))
        assert np.array_equal(again.chain, host.chain[:, stop:]), stop
        assert np.array_equal(again.lnlikelihood, host.lnlikelihood[:, :, stop:]), stop
    # out of scope: a ladder beyond max_walkers, a bad ladder
    with pytest.raises(ValueError):
        DeviceTemperedSampler(42, model, betas=betas)
    with pytest.raises(ValueError):
        DeviceTemperedSampler(40, model, betas=[1.0, 0.5])
    model.close()


def test_split_evaluation_matches_the_posterior(tmp_path):
    model = _synth_model(tmp_path, 64)
    case = helpers.load_case('synth128x2')
    theta = case['params'][:40]
    ll, lp = model.log_likelihood_and_prior_batch(theta)
    post = model.log_posterior_batch(theta)
    fin = np.isfinite(post)
    assert np.array_equal(ll[fin] + lp[fin], post[fin])
    assert np.all(ll[~fin] == -np.inf)
    model.close()


def test_one_rung_is_the_stretch_sampler(tmp_path):
    from psfmc_amd.sampler import DeviceEnsembleSampler, DeviceTemperedSampler
    model = _synth_model(tmp_path, 64)
    np.random.seed(4)
    p0 = model.init_params_from_priors(40)
    ref = DeviceEnsembleSampler(40, model, block=6)
    one = DeviceTemperedSampler(40, model, betas=[1.0], block=5)
    for s in (ref, one):
        s.random_state = np.random.RandomState(8).get_state()
    list(ref.sample(p0, iterations=14))
    list(one.sample(p0[None], iterations=14))
    assert np.array_equal(one.chain, ref.chain)
    assert np.array_equal(one.lnprobability, ref.lnprobability)
    assert np.array_equal(one.naccepted, ref.naccepted)
    model.close()


def test_accumulation_of_the_beta_one_rung(tmp_path):
    from psfmc_amd.sampler import DeviceTemperedSampler
    model = _synth_model(tmp_path, 96)
    np.random.seed(5)
    p0 = np.stack([model.init_params_from_priors(24) for _ in range(3)])
    model.reset_images()
    acc = DeviceTemperedSampler(24, model, ntemps=3, tmax=20.0, block=4, accumulate=True)
    acc.random_state = np.random.RandomState(3).get_state()
    steps = list(acc.sample(p0, iterations=6))
    got = {k: v.copy() for k, v in model.collect_posterior_images().items()}
    assert model.accumulated_samples == 6 * 24
    model.reset_images()
    for pos, _, _, _ in steps:
        model.accumulate_samples(pos[0])
    want = model.collect_posterior_images()
    for k in want:
        assert np.allclose(got[k], want[k], rtol=1e-11, atol=1e-12 * np.abs(want[k]).max()), k
    model.close()


def _write_field(directory, fld):
    from psfmc_amd import fits_io
    for key, name in (('sci', 'sci.fits'), ('ivm', 'ivm.fits'), ('psf', 'psf.fits'), ('psf_ivm', 'psf_ivm.fits')):
        fits_io.write_image(os.path.join(str(directory), name), fld[key])


def _write_model(directory, name, text):
    path = os.path.join(str(directory), name)
    with open(path, 'w') as f:
        f.write(text)
    return path


def _logsumexp(x):
    m = np.max(x)
    return m + np.log(np.sum(np.exp(x - m)))


# the floor of tests/test_tempered.py's two-parameter problem
EVIDENCE_FLOOR_2D = 0.1


def test_evidence_against_quadrature(tmp_path):
    """Two free parameters (point-source magnitude, sky level), everything else constant: ln Z by quadrature
    of exp(lnL) pi over +-10 sigma of the beta = 1 posterior against log_evidence()."""
    from psfmc_amd import MultiComponentModel
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
    model = MultiComponentModel(_write_model(tmp_path, 'model2.py', text), max_walkers=n_t * n_w)
    assert model.num_params == 2
    rs = np.random.RandomState(0)
    p0 = np.stack([model.init_params_from_priors(n_w) for _ in range(n_t)])
    s = DeviceTemperedSampler(n_w, model, betas=default_betas(n_t, 1e7), block=64)
    s.random_state = rs.get_state()
    for _ in s.sample(p0, iterations=800):
        pass
    lnz, err = s.log_evidence(0.25)
    post = s.chain[:, 200:].reshape(-1, 2)
    mu, sd = post.mean(axis=0), post.std(axis=0)
    grids = [np.linspace(m - 10 * d, m + 10 * d, 161) for m, d in zip(mu, sd)]
    gx, gy = np.meshgrid(*grids, indexing='ij')
    theta = np.stack([gx.ravel(), gy.ravel()], axis=1)
    names = model.param_names                  # column order of the emcee vector
    assert len(names) == 2
    lnpost = np.concatenate([model.log_posterior_batch(theta[lo:lo + model._max_walkers])
                             for lo in range(0, len(theta), model._max_walkers)])
    cell = (grids[0][1] - grids[0][0]) * (grids[1][1] - grids[1][0])
    exact = _logsumexp(lnpost) + np.log(cell)
    assert abs(lnz - exact) <= max(3 * err, EVIDENCE_FLOOR_2D), (lnz, exact, err)
    model.close()


def test_model_comparison_prefers_the_host(tmp_path):
    """A point source with a Sersic host: ln Z(PS + Sersic) - ln Z(PS only) is positive by many times its error."""
    from psfmc_amd import MultiComponentModel
    from psfmc_amd.sampler import DeviceTemperedSampler, default_betas
    fld = synth_field.make_field(128, n_sersic=1, seed=0)
    _write_field(tmp_path, fld)
    res = {}
    for n_s in (0, 1):
        path = _write_model(tmp_path, 'model_%d.py' % n_s, synth_field.model_file_text(128, n_s))
        n_t = 16
        model = MultiComponentModel(path, max_walkers=1024)
        n_w = 2 * model.num_params + 2
        rs = np.random.RandomState(1 + n_s)
        p0 = np.stack([model.init_params_from_priors(n_w) for _ in range(n_t)])
        s = DeviceTemperedSampler(n_w, model, betas=default_betas(n_t, 1e6))
        s.random_state = rs.get_state()
        for _ in s.sample(p0, iterations=400):
            pass
        res[n_s] = s.log_evidence(0.5)
        model.close()
    dz = res[1][0] - res[0][0]
    err = res[1][1] + res[0][1]
    assert dz > 0 and dz > 10 * max(err, EVIDENCE_FLOOR_2D), (res, dz)


def test_model_galaxy_ptmcmc_example(tmp_path):
    from psfmc_amd import model_galaxy_ptmcmc, load_database
    src = os.path.join(helpers.GOLDEN, 'example')
    for name in os.listdir(src):
        if os.path.isfile(os.path.join(src, name)):
            shutil.copy(os.path.join(src, name), tmp_path)
    out = str(tmp_path / 'out_example')
    np.random.seed(42)
    model, db, (lnz, err) = model_galaxy_ptmcmc(str(tmp_path / 'model_example.py'), output_name=out, iterations=20,
                                                burn=10, chains=40, ntemps=4, tmax=100.0, random_state=7,
                                                quiet=True)
    assert model._max_walkers >= 4 * 40
    db2 = load_database(out + '_db.fits')
    assert len(db2) == 40 * 20 and db2.meta['MCITER'] == 20 and db2.meta['MCNTEMPS'] == 4
    assert np.isfinite(db2.meta['MCLNZ']) and db2.meta['MCLNZERR'] >= 0 and 0 <= db2.meta['MCTSWAP'] <= 1
    assert db2.meta['MCLNZ'] == pytest.approx(lnz) and np.isfinite(err)
    theta = db2.param_matrix(model.param_names)
    again = model.log_posterior_batch(theta[::37])
    assert helpers.rel_err(again, db2['lnprobability'][::37]) <= 1e-12
    assert model.accumulated_samples == 40 * 20
    assert os.path.exists(out + '_convolved_model.fits')
    model.close()
