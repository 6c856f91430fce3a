"""The mode search of the multi-field entry points: `find_modes` for the fields of a `FieldSet`, `find_mode` on a
`JointModel`, and `start='mode'` of `model_fields_mcmc` and `model_joint_mcmc` -- all on 64 x 64 synthetic fields
(point source + Sersic, K = 10 per field; `test_gpu_fisher._synth_model`).

`find_modes` advances the fields' searches side by side with shared device calls; its contract is that field f's
result is `find_mode(fs.models[f], ...)`'s from the same starts, bit for bit.  The joint fit is two exposures of one
scene (tests/test_joint_fisher_definition.py `two_exposures`), positions per exposure: K_joint = 14."""
import numpy as np
import pytest

import synth_field
import test_gpu_fisher as tgf
import test_joint_fisher_definition as tjd

pytestmark = pytest.mark.gpu

K = 10
PER_FIELD = ['0_PointSource_xy', '1_Sersic_xy']


def _fields(n):
    return [synth_field.make_field(64, 1, seed=s) for s in range(n)]


def test_find_modes_is_find_mode_per_field():
    from psfmc_amd import FieldSet, find_mode, find_modes
    flds = _fields(3)
    fs = FieldSet([tgf._synth_model(fld, 'fused', 1) for fld in flds], max_walkers=6 * (2 * K + 1))
    try:
        starts = [np.vstack([fld['truth'], synth_field.draw_walkers(64, 1, 1, seed=20 + f, near_truth=fld['truth'])])
                  for f, fld in enumerate(flds)]
        together = find_modes(fs, start=starts)
        assert len(together) == 3
        for f in range(3):
            alone = find_mode(fs.models[f], start=starts[f])
            got = together[f]
            print('field %d: %r against %r' % (f, got, alone))
            assert got.converged and got.ok
            assert np.array_equal(got.theta, alone.theta), f
            assert got.lnpost == alone.lnpost and got.iterations == alone.iterations, f
            assert np.array_equal(got.cov, alone.cov) and np.array_equal(got.columns, alone.columns), f
            assert got.lnpost >= fs.models[f].log_posterior_batch(flds[f]['truth'])[0]
        assert not np.array_equal(together[0].theta, together[1].theta)
        with pytest.raises(ValueError):
            find_modes(fs, start=starts[:2])
    finally:
        fs.close()


def _joint(max_walkers):
    from psfmc_amd import JointModel
    _, truth, flds = tjd.two_exposures()
    joint = JointModel([tgf._synth_model(fld, 'fused', 1) for fld in flds], per_field=PER_FIELD,
                       max_walkers=max_walkers)
    assert joint.num_params == tjd.K_JOINT
    assert all(np.array_equal(joint.field_columns(f), tjd.COL_OF[f]) for f in range(2))
    return joint, truth


def test_find_mode_of_a_joint_model():
    from psfmc_amd import find_mode
    joint, truth = _joint(2 * (2 * K + 1))
    try:
        res = find_mode(joint, start=truth)
        print('joint find_mode from the truth: %r, laplace lnZ %.3f' % (res, res.laplace_log_evidence))
        assert res.converged and res.ok and len(res.columns) == tjd.K_JOINT
        assert res.cov.shape == (tjd.K_JOINT, tjd.K_JOINT)
        np.linalg.cholesky(res.cov)
        assert np.isfinite(res.laplace_log_evidence)
        assert res.lnpost >= joint.log_posterior_batch(truth)[0]
        assert res.lnpost == joint.log_posterior_batch(res.theta)[0]
        # a shared column is tighter than either exposure's own fit would make it
        for f, m in enumerate(joint.field_models):
            own = m.fisher(res.theta[tjd.COL_OF[f]])
            single = np.diag(np.linalg.inv(own['F']))
            for j in tjd.SHARED:
                assert res.cov[j, j] < single[int(np.flatnonzero(tjd.COL_OF[f] == j)[0])], (f, j)
    finally:
        joint.close()


def _first_iteration(db):
    return np.asarray(db['lnprobability'])[np.asarray(db['sample']) == np.min(db['sample'])]


def test_model_joint_mcmc_starts_from_the_mode(tmp_path):
    """The walkers' log-posteriors at the first recorded iteration (the measure tests/test_gpu_fisher.py
    test_model_galaxy_mcmc_starts_from_the_mode takes): a Gaussian draw sits chi^2_K / 2, on average K / 2, below
    the mode; the median is held to 2 K."""
    from psfmc_amd import load_database, model_joint_mcmc
    chains = 2 * tjd.K_JOINT + 2

    def run(tag, **kw):
        joint, _ = _joint(2 * 1024)
        np.random.seed(17)                                # prior draws use numpy's global generator
        out = str(tmp_path / tag)
        model_joint_mcmc(joint, output_name=out, chains=chains, burn=0, iterations=3, random_state=5, quiet=True,
                         write_fits=(), **kw)
        joint.close()
        return out + '_db.fits'

    db = load_database(run('mode', start='mode'))
    assert db.meta['MCSTART'] == 'mode' and np.isfinite(db.meta['MCMODELP']) and db.meta['MCFIELDS'] == 2
    first = _first_iteration(db)
    assert len(first) == chains and np.all(np.isfinite(first))
    print('joint, first iteration: median %.2f below the mode (2 K = %d)' % (
        db.meta['MCMODELP'] - np.median(first), 2 * tjd.K_JOINT))
    assert db.meta['MCMODELP'] - np.median(first) <= 2 * tjd.K_JOINT
    plain, prior = run('plain'), run('prior', start='prior')
    with open(plain, 'rb') as a, open(prior, 'rb') as b:
        assert a.read() == b.read()
    assert 'MCSTART' not in load_database(prior).meta and 'MCMODELP' not in load_database(prior).meta


def test_model_fields_mcmc_starts_from_the_modes(tmp_path):
    from psfmc_amd import load_database, model_fields_mcmc
    chains = 2 * K + 2
    flds = _fields(2)

    def run(tag, **kw):
        models = [tgf._synth_model(fld, 'fused', 1) for fld in flds]
        np.random.seed(17)
        outs = [str(tmp_path / ('%s%d' % (tag, f))) for f in range(2)]
        model_fields_mcmc(models, output_names=outs, chains=chains, burn=0, iterations=3, random_states=[5, 6],
                          quiet=True, write_fits=(), **kw)
        return [o + '_db.fits' for o in outs]

    for f, name in enumerate(run('mode', start='mode')):
        db = load_database(name)
        assert db.meta['MCSTART'] == 'mode' and np.isfinite(db.meta['MCMODELP'])
        first = _first_iteration(db)
        assert len(first) == chains and np.all(np.isfinite(first))
        print('field %d, first iteration: median %.2f below the mode (2 K = %d)' % (
            f, db.meta['MCMODELP'] - np.median(first), 2 * K))
        assert db.meta['MCMODELP'] - np.median(first) <= 2 * K
    for plain, prior in zip(run('plain'), run('prior', start='prior')):
        with open(plain, 'rb') as a, open(prior, 'rb') as b:
            assert a.read() == b.read()
        assert 'MCSTART' not in load_database(prior).meta
    with pytest.raises(ValueError, match='start_positions'):
        model_fields_mcmc([tgf._synth_model(fld, 'fused', 1) for fld in flds], chains=chains, start='mode',
                          start_positions=[np.zeros((chains, K))] * 2, quiet=True)
