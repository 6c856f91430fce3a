"""JointModel's linking of several fields' parameters into one joint vector, checked on the host: column
order and names, per-field blocks, the PSF index always per field, each field's own vector, the joint
log-prior, and the refusals -- all without opening a GPU context."""
import numpy as np
import pytest
from scipy import stats

import synth_field

MAG_ZP = 25.0
# (ny, nx, PSF side)
SHAPES = [(118, 118, 11), (100, 112, 17), (128, 128, 21)]
PS_NAMES = ['0_PointSource_mag', '0_PointSource_xy']
SERSIC_NAMES = ['1_Sersic_angle', '1_Sersic_index', '1_Sersic_mag', '1_Sersic_reff', '1_Sersic_reff_b',
                '1_Sersic_xy']
POS = ['0_PointSource_mag', '0_PointSource_xy', '1_Sersic_xy']   # per field in the usual joint fit


def make_field(ny, nx, pk, seed, n_psf=2):
    """Noisy image of a point source + one Sersic and n_psf Moffat PSFs of side pk."""
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
    for fwhm in (2.4, 3.1)[:n_psf]:
        p = synth_field.moffat_psf(pk, fwhm=fwhm) * 1000.0
        var = 1e-4 + np.abs(p) / 50.0
        psfs.append((p + rng.normal(size=p.shape) * np.sqrt(var)).astype(np.float32))
        pivms.append((1.0 / var).astype(np.float32))
    return dict(sci=sci, ivm=ivm, psfs=psfs, pivms=pivms, truth=truth, c=(cx, cy))


def make_model(fld, max_walkers=1, sersic_mag=None, sky=False):
    """The field's MultiComponentModel: PS + Sersic (+ Sky), positions' priors centred on the field."""
    from psfmc_amd import MultiComponentModel
    from psfmc_amd.ModelComponents import Configuration, PointSource, Sersic, Sky
    from psfmc_amd.distributions import Normal, Uniform, WeibullMinimum
    c = np.array(fld['c'])
    comps = [Configuration(fld['sci'], fld['ivm'], fld['psfs'], fld['pivms'], mag_zeropoint=MAG_ZP),
             PointSource(xy=Uniform(loc=c - 4, scale=8 * np.ones(2)), mag=Uniform(loc=18.0, scale=2.0)),
             Sersic(xy=Uniform(loc=c - 4, scale=8 * np.ones(2)), mag=sersic_mag or Uniform(loc=19.0, scale=3.0),
                    reff=Uniform(loc=2.0, scale=6.0), reff_b=Uniform(loc=2.0, scale=6.0),
                    index=WeibullMinimum(c=1.5, scale=4), angle=Uniform(loc=0, scale=180), angle_degrees=True)]
    if sky:
        comps.append(Sky(adu=Normal(loc=0.0, scale=0.1)))
    return MultiComponentModel(comps, backend='fused', max_walkers=max_walkers)


@pytest.fixture
def no_gpu(monkeypatch):
    """Any attempt to load the library or create a context fails the test."""
    from psfmc_amd import engine

    def refuse(*args, **kwargs):
        raise AssertionError('the GPU was touched')
    monkeypatch.setattr(engine, 'load_library', refuse)
    monkeypatch.setattr(engine, 'FieldSetContext', refuse)
    monkeypatch.setattr(engine, 'Context', refuse)


@pytest.fixture
def fields():
    return [make_field(ny, nx, pk, seed=30 + f) for f, (ny, nx, pk) in enumerate(SHAPES)]


def test_joint_columns_and_names(no_gpu, fields):
    from psfmc_amd import JointModel
    joint = JointModel([make_model(fld) for fld in fields], per_field=POS)
    own = joint.field_models[0].param_names
    assert own == PS_NAMES + SERSIC_NAMES + ['PSF_Index']
    want = ([n + '_f%d' % f for n in PS_NAMES for f in range(3)] + SERSIC_NAMES[:-1] +
            ['1_Sersic_xy_f%d' % f for f in range(3)] + ['PSF_Index_f%d' % f for f in range(3)])
    assert joint.param_names == want
    assert joint.param_lens == [1] * 3 + [2] * 3 + [1] * 5 + [2] * 3 + [1] * 3
    assert joint.num_params == sum(joint.param_lens) == 3 * (1 + 2) + 5 + 3 * 2 + 3
    assert joint._context is None


def test_psf_index_is_per_field_by_itself(no_gpu, fields):
    from psfmc_amd import JointModel
    # the same exposure three times, nothing named per field: only the PSF index is per field
    joint = JointModel([make_model(fields[0]) for _ in range(3)])
    assert joint.param_names == PS_NAMES + SERSIC_NAMES + ['PSF_Index_f0', 'PSF_Index_f1', 'PSF_Index_f2']
    assert joint.num_params == 3 + 7 + 3
    # named per field as well: the same
    assert JointModel([make_model(fields[0]) for _ in range(3)], per_field=['PSF_Index']).param_names == \
        joint.param_names
    # one PSF per field: no PSF index at all, so everything is shared
    one = make_field(*SHAPES[0], seed=40, n_psf=1)
    joint1 = JointModel([make_model(one) for _ in range(2)])
    assert joint1.param_names == PS_NAMES + SERSIC_NAMES
    assert joint1._context is None


def test_field_theta_reads_each_fields_columns(no_gpu, fields):
    from psfmc_amd import JointModel
    joint = JointModel([make_model(fld) for fld in fields], per_field=POS)
    names, lens = joint.param_names, joint.param_lens
    start = dict(zip(names, np.concatenate([[0], np.cumsum(lens)[:-1]])))
    theta = np.arange(4 * joint.num_params, dtype=np.float64).reshape(4, -1) * 0.5
    for f, m in enumerate(joint.field_models):
        got = joint.field_theta(theta, f)
        assert got.shape == (4, m.num_params)
        pos = 0
        for name, width in zip(m.param_names, m.param_lens):
            src = name + '_f%d' % f if (name in POS or name == 'PSF_Index') else name
            assert np.array_equal(got[:, pos:pos + width], theta[:, start[src]:start[src] + width]), (f, name)
            pos += width
    assert joint._context is None


def test_log_priors_count_each_joint_column_once(no_gpu, fields):
    from psfmc_amd import JointModel
    joint = JointModel([make_model(fld) for fld in fields], per_field=POS)
    np.random.seed(3)
    theta = joint.init_params_from_priors(12)
    assert np.all(np.isfinite(joint.log_priors_batch(theta)))
    col = lambda name: sum(joint.param_lens[:joint.param_names.index(name)])
    theta[5, col('1_Sersic_mag')] = 30.0                                           # shared, out of support
    theta[6, col('0_PointSource_mag_f1')] = 10.0                                   # one field's, out of support
    ib, ir = col('1_Sersic_reff_b'), col('1_Sersic_reff')
    theta[7, ib] = theta[7, ir] + 0.5                                               # axis ratio
    got = joint.log_priors_batch(theta)
    # scipy, column by column: a shared column once, each per-field column with its field's prior
    want = np.zeros(len(theta))
    for w, t in enumerate(theta):
        lp, pos = 0.0, 0
        for name, width in zip(joint.param_names, joint.param_lens):
            base, f = (name.rsplit('_f', 1)[0], int(name.rsplit('_f', 1)[1])) if '_f' in name else (name, 0)
            c = np.array(fields[f]['c'])
            x = t[pos:pos + width]
            if base == '0_PointSource_mag':
                lp += stats.uniform(18.0, 2.0).logpdf(x).sum()
            elif base.endswith('_xy'):
                lp += stats.uniform(c - 4, 8 * np.ones(2)).logpdf(x).sum()
            elif base == '1_Sersic_mag':
                lp += stats.uniform(19.0, 3.0).logpdf(x).sum()
            elif base in ('1_Sersic_reff', '1_Sersic_reff_b'):
                lp += stats.uniform(2.0, 6.0).logpdf(x).sum()
            elif base == '1_Sersic_index':
                lp += stats.weibull_min(1.5, scale=4).logpdf(x).sum()
            elif base == '1_Sersic_angle':
                lp += stats.uniform(0, 180).logpdf(x).sum()
            elif base == 'PSF_Index':
                lp += stats.randint(0, 2).logpmf(x).sum()
            else:
                raise AssertionError(name)
            pos += width
        if t[ib] > t[ir]:
            lp = -np.inf
        want[w] = lp
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    assert not np.isfinite(got[[5, 6, 7]]).any() and np.isfinite(got[:5]).all()
    ok = np.isfinite(want)
    assert np.allclose(got[ok], want[ok], rtol=1e-13, atol=0)
    assert joint._context is None


def test_refusals(no_gpu, fields):
    from psfmc_amd import JointModel
    from psfmc_amd.distributions import Uniform
    # a shared prior that differs between fields (field 2's Sersic magnitude)
    models = [make_model(fld) for fld in fields[:2]] + [make_model(fields[2], sersic_mag=Uniform(loc=19.0,
                                                                                              scale=3.5))]
    with pytest.raises(ValueError, match=r'1_Sersic_mag.*field 2'):
        JointModel(models, per_field=POS)
    JointModel(models, per_field=POS + ['1_Sersic_mag'])                          # per field: fine
    # a per_field name that does not exist
    with pytest.raises(ValueError, match='no_such_param'):
        JointModel([make_model(fld) for fld in fields], per_field=['no_such_param'])
    # fields with different parameter lists
    with pytest.raises(ValueError, match='field 1'):
        JointModel([make_model(fields[0]), make_model(fields[1], sky=True)])
    # a prior without a device form (a gamma distribution) in field 1
    from psfmc_amd.distributions import Gamma
    bad = make_model(fields[1], sersic_mag=Gamma(2.0, loc=19.0, scale=1.0))
    with pytest.raises(ValueError, match='device form'):
        JointModel([make_model(fields[0]), bad], per_field=['1_Sersic_mag'])
    # out-of-scope back ends
    f32 = make_model(fields[2])
    f32._storage = 'f32'
    with pytest.raises(ValueError, match='f64'):
        JointModel([f32])
