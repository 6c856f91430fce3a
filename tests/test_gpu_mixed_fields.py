"""A FieldSet whose fields differ in image and PSF size (psfmc_ctx_create_fields_shaped): one shared transform
shape, each field embedded in it at its own place (or not at all where its side is the transform's).  Every
field's log-posteriors, sampler chains and images are held to the oracle and to the field's own context."""
import numpy as np
import pytest

import helpers
import psfmc_oracle as orc
import synth_field

pytestmark = pytest.mark.gpu

# (ny, nx, PSF side): embedded 118^2 (11-pixel PSF), embedded 100 x 112 (17), the built side 128^2 (21)
SHAPES = [(118, 118, 11), (100, 112, 17), (128, 128, 21)]
LAYOUT = helpers.synth_layout(1)
MAG_ZP = 25.0


def _field(ny, nx, pk, seed):
    """Noisy image of a point source + one Sersic, two Moffat PSFs of side pk (the second wider)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
    cx, cy = nx / 2 + 0.5, ny / 2 + 0.5
    truth = np.array([19.0, cx + 0.3, cy - 0.6,                      # PS: mag, x, y
                      35.0, 2.0, 20.5, 5.0, 3.0, cx - 1.2, cy + 0.8,  # Sersic: angle, index, mag, reff, reff_b, x, y
                      0.0])                                            # psf_index
    img = 40.0 * np.exp(-((xx - truth[8]) ** 2 + (yy - truth[9]) ** 2) / 18.0)
    img[int(truth[2]), int(truth[1])] += 300.0
    sci = (img + rng.normal(size=(ny, nx)) * 0.05).astype(np.float32)
    ivm = np.full((ny, nx), 400.0, dtype=np.float32)
    psfs, pivms = [], []
    for fwhm in (2.4, 3.1):
        p = synth_field.moffat_psf(pk, fwhm=fwhm) * 1000.0
        var = 1e-4 + np.abs(p) / 50.0
        psfs.append((p + rng.normal(size=p.shape) * np.sqrt(var)).astype(np.float32))
        pivms.append((1.0 / var).astype(np.float32))
    return dict(sci=sci, ivm=ivm, psfs=psfs, pivms=pivms, truth=truth, c=(cx, cy))


def _model(fld, max_walkers):
    from psfmc_amd import MultiComponentModel
    from psfmc_amd.ModelComponents import Configuration, PointSource, Sersic
    from psfmc_amd.distributions import Uniform, WeibullMinimum
    c = np.array(fld['c'])
    comps = [Configuration(fld['sci'], fld['ivm'], fld['psfs'], fld['pivms'], mag_zeropoint=MAG_ZP),
             PointSource(xy=Uniform(loc=c - 4, scale=8 * np.ones(2)), mag=Uniform(loc=18.0, scale=2.0)),
             Sersic(xy=Uniform(loc=c - 4, scale=8 * np.ones(2)), mag=Uniform(loc=19.0, scale=3.0),
                    reff=Uniform(loc=2.0, scale=6.0), reff_b=Uniform(loc=2.0, scale=6.0),
                    index=WeibullMinimum(c=1.5, scale=4), angle=Uniform(loc=0, scale=180), angle_degrees=True)]
    return MultiComponentModel(comps, backend='fused', max_walkers=max_walkers)


def _thetas(fld, n, seed):
    """n walkers: near-truth vectors, prior draws and out-of-support vectors (-inf), both PSFs."""
    rng = np.random.RandomState(seed)
    out = fld['truth'] + rng.normal(size=(n, len(fld['truth']))) * 1e-2
    out[:, 10] = rng.randint(0, 2, n)
    cx, cy = fld['c']
    k = n // 3
    out[k:2 * k, 0] = rng.uniform(18.0, 20.0, k)
    out[k:2 * k, 1] = rng.uniform(cx - 4, cx + 4, k)
    out[k:2 * k, 2] = rng.uniform(cy - 4, cy + 4, k)
    out[k:2 * k, 5] = rng.uniform(19.0, 22.0, k)
    out[k:2 * k, 3] = rng.uniform(0.0, 180.0, k)
    out[2 * k, 0] = 25.0                          # PS magnitude outside its prior
    out[2 * k + 1, 10] = 2.0                      # no third PSF
    out[2 * k + 2, 7] = out[2 * k + 2, 6] + 1.0   # reff_b > reff (the reference rejects it)
    out[:, 7] = np.where(np.arange(n) == 2 * k + 2, out[:, 7], np.minimum(out[:, 7], out[:, 6] - 1e-3))
    return out


def _oracle_field(fld):
    return orc.make_field(fld['sci'], fld['ivm'], fld['psfs'], fld['pivms'], mag_zp=MAG_ZP)


@pytest.fixture(scope='module')
def setup():
    from psfmc_amd import FieldSet
    flds = [_field(ny, nx, pk, seed=30 + f) for f, (ny, nx, pk) in enumerate(SHAPES)]
    fs = FieldSet([_model(fld, 1) for fld in flds], max_walkers=192)
    yield flds, fs
    fs.close()


def test_set_geometry(setup):
    flds, fs = setup
    ctx = fs.context
    assert ctx.shape is None and ctx.shapes == [(ny, nx) for ny, nx, _ in SHAPES]
    for f, (ny, nx, _) in enumerate(SHAPES):
        assert ctx.field_shape(f) == (ny, nx)
    assert (ctx.get_option('transform_ny'), ctx.get_option('transform_nx')) == (128, 128)


def _eval_segments(fs, segs):
    """psfmc_eval_theta_fields on an interleaved segment list [(field, theta block)]."""
    from psfmc_amd.engine import _dp
    ctx = fs.context
    theta = np.ascontiguousarray(np.concatenate([t for _, t in segs]))
    f, n, fp, np_ = ctx._segments([s for s, _ in segs], [len(t) for _, t in segs])
    out = np.empty(len(theta))
    ctx._check(ctx._lib.psfmc_eval_theta_fields(ctx._ctx, len(f), fp, np_, _dp(theta), None, _dp(out)))
    res, off = [], 0
    for _, t in segs:
        res.append(out[off:off + len(t)])
        off += len(t)
    return res


def test_log_posteriors_against_the_oracle_and_own_contexts(setup):
    flds, fs = setup
    n = 24
    thetas = [_thetas(fld, n, seed=50 + f) for f, fld in enumerate(flds)]
    # interleaved segments of every field: 0 2 1 0 2 1 ...
    segs, order = [], []
    for lo in range(0, n, 8):
        for f in (0, 2, 1):
            segs.append((f, thetas[f][lo:lo + 8]))
            order.append(f)
    parts = _eval_segments(fs, segs)
    got = [np.concatenate([p for p, f in zip(parts, order) if f == g]) for g in range(3)]
    tr_y, tr_x = fs.context.get_option('transform_ny'), fs.context.get_option('transform_nx')
    same_transform = []
    for f, fld in enumerate(flds):
        # alone through the set: a walker's value does not depend on the other fields of its batch
        alone = [None] * 3
        alone[f] = thetas[f]
        assert np.array_equal(fs.log_posterior_batch(alone)[f], got[f]), f
        prior = fs.models[f].log_priors_batch(thetas[f])
        assert np.isinf(prior).sum() >= 3 and np.isfinite(prior).sum() >= 2 * n // 3
        field = _oracle_field(fld)
        for i in range(n):
            if not np.isfinite(prior[i]):
                assert got[f][i] == -np.inf, (f, i)
                continue
            want = helpers.oracle_loglike(field, LAYOUT, thetas[f][i], has_psf_index=True) + prior[i]
            assert abs(got[f][i] - want) <= 1e-11 * abs(want), (f, i, got[f][i], want)
        # the field's own context
        own = _model(fld, 64)
        mine = own.log_posterior_batch(thetas[f])
        fin = np.isfinite(mine)
        assert np.array_equal(fin, np.isfinite(got[f]))
        assert np.abs(got[f][fin] - mine[fin]).max() <= 1e-12 * np.abs(mine[fin]).max(), f
        if (own.engine.get_option('transform_ny'), own.engine.get_option('transform_nx')) == (tr_y, tr_x):
            same_transform.append(f)
            assert np.array_equal(got[f], mine), f
        own.close()
    assert 2 in same_transform              # the built side 128^2: its own context has the set's transform


def test_samplers_per_field(setup):
    """The FieldSetSampler chain of every field equals the host sampler's on that field's log-posterior and,
    for the field whose own context has the set's transform, its own DeviceEnsembleSampler's bit for bit."""
    from psfmc_amd import FieldSetSampler, DeviceEnsembleSampler, EnsembleSampler
    flds, fs = setup
    n_w, n_iter = 24, 5                     # (at least twice the 11 parameters)
    p0 = [flds[f]['truth'] + np.random.RandomState(70 + f).normal(size=(n_w, 11)) * 1e-3 for f in range(3)]
    for p in p0:
        p[:, 10] = np.arange(n_w) % 2
    joint = FieldSetSampler(n_w, fs, block=2, accumulate=False)
    for f, sub in enumerate(joint.fields):
        sub.random_state = np.random.RandomState(600 + f).get_state()
    for _ in joint.sample(p0, iterations=n_iter):
        pass
    for f in range(3):
        host = EnsembleSampler(n_w, fs.num_params, batch_lnpostfn=fs.models[f].log_posterior_batch)
        host.random_state = np.random.RandomState(600 + f).get_state()
        for _ in host.sample(p0[f], iterations=n_iter):
            pass
        sub = joint.fields[f]
        assert np.array_equal(sub.chain, host.chain), f
        assert np.array_equal(sub.lnprobability, host.lnprobability), f
        assert np.array_equal(sub.naccepted, host.naccepted), f
        assert host.naccepted.sum() > 0
    own = _model(flds[2], n_w)
    solo = DeviceEnsembleSampler(n_w, own, block=2)
    solo.random_state = np.random.RandomState(602).get_state()
    for _ in solo.sample(p0[2], iterations=n_iter):
        pass
    sub = joint.fields[2]
    assert np.array_equal(sub.chain, solo.chain)
    assert np.array_equal(sub.lnprobability, solo.lnprobability)
    assert np.array_equal(sub.naccepted, solo.naccepted)
    own.close()


def test_images_at_each_fields_shape(setup):
    flds, fs = setup
    owns = []
    for f, fld in enumerate(flds):
        ny, nx, _ = SHAPES[f]
        theta = _thetas(fld, 9, seed=80 + f)[:4]            # near truth and prior draws, finite priors
        imgs = fs.models[f].sample_images(theta)
        assert set(imgs) == set(fs.context.IMAGE_KINDS)
        field = _oracle_field(fld)
        for i, t in enumerate(theta):
            comps, psf = helpers.comps_from_theta(LAYOUT, t, True)
            _, want = orc.evaluate(field, comps, psf, raw_dtype=np.float64, want_ps_sub=True)
            for kind, img in imgs.items():
                assert img.shape == (4, ny, nx), (f, kind)
                w = want[kind]
                assert np.abs(img[i] - w).max() <= 1e-10 * np.abs(w).max(), (f, kind, i)
        own = _model(fld, 16)
        own.accumulate_samples(theta)
        fs.models[f].reset_images()
        fs.models[f].accumulate_samples(theta)
        owns.append((own, theta))
    for f, (own, theta) in enumerate(owns):
        ny, nx, _ = SHAPES[f]
        want, got = own.collect_posterior_images(), fs.models[f].collect_posterior_images()
        for kind in want:
            assert got[kind].shape == (ny, nx), (f, kind)
            fin = np.isfinite(want[kind])
            assert np.array_equal(np.isfinite(got[kind]), fin)
            a, b = got[kind][fin], want[kind][fin]
            if kind == 'composite_ivm':
                # compared as the variance 1 / ivm (model variance + obs_var): where a field's own transform is not
                # the set's, the convolutions round differently, and 1 / (var + obs_var) scales a rounding of the
                # model variance by ivm^2 (1.6e5 here)
                a, b = 1.0 / a, 1.0 / b
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (f, kind)
    # clearing one field's sums leaves the others'
    for f, (_, theta) in enumerate(owns):
        fs.models[f].accumulate_samples(theta[:f + 1])
    before = [fs.context.accumulated(f) for f in range(3)]
    assert [b[1] for b in before] == [1, 2, 3]
    fs.models[1].reset_images()
    assert fs.context.accumulated(1)[1] == 0
    for f in (0, 2):
        imgs, n = fs.context.accumulated(f)
        assert n == f + 1
        for kind, img in imgs.items():
            assert img.shape == SHAPES[f][:2] and np.array_equal(img, before[f][0][kind]), (f, kind)
    for own, _ in owns:
        own.close()


def _write_model_file(directory, fld, name):
    from psfmc_amd import fits_io
    d = str(directory)
    fits_io.write_image('%s/%s_sci.fits' % (d, name), fld['sci'])
    fits_io.write_image('%s/%s_ivm.fits' % (d, name), fld['ivm'])
    for k in range(2):
        fits_io.write_image('%s/%s_psf%d.fits' % (d, name, k), fld['psfs'][k])
        fits_io.write_image('%s/%s_psfivm%d.fits' % (d, name, k), fld['pivms'][k])
    cx, cy = fld['c']
    text = '\n'.join([
        'from numpy import array',
        "Configuration(obs_file='{0}/{1}_sci.fits', obsivm_file='{0}/{1}_ivm.fits',".format(d, name),
        "              psf_files=['{0}/{1}_psf0.fits', '{0}/{1}_psf1.fits'],".format(d, name),
        "              psfivm_files=['{0}/{1}_psfivm0.fits', '{0}/{1}_psfivm1.fits'], mag_zeropoint={2!r})".format(
            d, name, MAG_ZP),
        'c = array(({!r}, {!r}))'.format(cx, cy),
        'ms = array((4.0, 4.0))',
        'PointSource(xy=Uniform(loc=c - ms, scale=2 * ms), mag=Uniform(loc=18.0, scale=2.0))',
        'Sersic(xy=Uniform(loc=c - ms, scale=2 * ms), mag=Uniform(loc=19.0, scale=3.0),',
        '       reff=Uniform(loc=2.0, scale=6.0), reff_b=Uniform(loc=2.0, scale=6.0),',
        '       index=WeibullMinimum(c=1.5, scale=4), angle=Uniform(loc=0, scale=180), angle_degrees=True)', ''])
    path = '%s/%s_model.py' % (d, name)
    with open(path, 'w') as f:
        f.write(text)
    return path


def test_model_fields_mcmc_writes_each_field_at_its_shape(tmp_path):
    from psfmc_amd import model_fields_mcmc, fits_io
    from psfmc_amd.database import load_database
    flds = [_field(118, 118, 11, seed=91), _field(100, 112, 17, seed=92)]
    files = [_write_model_file(tmp_path, fld, 'm%d' % f) for f, fld in enumerate(flds)]
    chains = 24
    p0 = [fld['truth'] + np.random.RandomState(95 + f).normal(size=(chains, 11)) * 1e-3
          for f, fld in enumerate(flds)]
    for p in p0:
        p[:, 10] = np.arange(chains) % 2
    outs = [str(tmp_path / ('out%d' % f)) for f in range(2)]
    with pytest.warns(UserWarning):                     # 4 iterations do not converge
        results = model_fields_mcmc(files, output_names=outs, iterations=4, burn=2, chains=chains,
                                    random_states=[3, 4], start_positions=p0, quiet=True)
    assert len(results) == 2
    import os
    for f, (ny, nx, _) in enumerate(SHAPES[:2]):
        db = load_database(outs[f] + '_db.fits')
        assert len(db['lnprobability']) == chains * 4
        written = [p for p in os.listdir(str(tmp_path)) if p.startswith('out%d_' % f) and p.endswith('.fits')
                   and not p.endswith('_db.fits')]
        assert len(written) == 5, written
        for p in written:
            assert fits_io.read_image(str(tmp_path / p)).shape == (ny, nx), p
    for m, _ in results:
        m.close()
