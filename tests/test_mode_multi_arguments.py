"""Argument checks of the joint and field-set mode search's Python layer that need no device: `start=` of
`model_joint_mcmc` and `model_fields_mcmc`, `JointModel.fisher`'s columns and steps, `mode.default_columns` /
`default_steps` on a joint model, and `find_modes`' bookkeeping (`mode._pack_fields`)."""
import numpy as np
import pytest

import test_joint_link as tjl
from test_joint_link import no_gpu, fields          # noqa: F401  (fixtures)
from psfmc_amd import mode


def test_start_mode_refuses_start_positions(no_gpu):
    from psfmc_amd import model_fields_mcmc
    with pytest.raises(ValueError, match='start_positions'):
        model_fields_mcmc(['a.py', 'b.py'], start='mode', start_positions=[np.zeros((4, 3))] * 2, chains=4)


@pytest.mark.parametrize('start', ['Mode', 'map', None, 1])
def test_bad_start_values(no_gpu, start):
    from psfmc_amd import model_fields_mcmc, model_joint_mcmc
    with pytest.raises(ValueError, match="'prior' or 'mode'"):
        model_fields_mcmc(['a.py', 'b.py'], start=start)
    with pytest.raises(ValueError, match="'prior' or 'mode'"):
        model_joint_mcmc(['a.py', 'b.py'], start=start)


def test_joint_columns_steps_and_their_refusals(no_gpu, fields):
    from psfmc_amd import JointModel
    joint = JointModel([tjl.make_model(fld) for fld in fields], per_field=tjl.POS)
    p = joint.num_params
    assert p == 3 * 3 + 5 + 3 * 2 + 3
    columns = mode.default_columns(joint)
    assert np.array_equal(columns, np.arange(p - 3))                 # the three PSF indices are discrete: left out
    theta = np.zeros(p)
    for f, fld in enumerate(fields):
        theta[joint.field_columns(f)] = fld['truth']
    step = mode.default_steps(joint, theta, columns)
    assert step.shape == (1, p - 3) and np.all(step > 0)
    # a Uniform(18, 2) magnitude: sd = 2 / sqrt(12), once per exposure
    assert np.allclose(step[0, :3], mode.STEP_FRACTION * 2.0 / np.sqrt(12.0), rtol=1e-12, atol=0)
    for bad in ([p], [-1], [0, 0], [], [[0, 1]]):
        with pytest.raises(ValueError, match='columns'):
            joint.fisher(theta, columns=bad)
    with pytest.raises(ValueError, match='joint parameter vectors'):
        joint.fisher(theta[:-1])
    with pytest.raises(ValueError, match='steps'):
        joint.fisher(theta, step=0.0)
    # exposure 0's own magnitude alone: the other exposures read none of the columns
    with pytest.raises(ValueError, match='same number'):
        joint.fisher(theta, columns=[0])


def test_pack_fields():
    assert mode._pack_fields([(0, 3), (2, 2)], 10) == [[(0, 0, 3), (2, 0, 2)]]
    assert mode._pack_fields([(0, 3), (1, 4)], 5) == [[(0, 0, 3), (1, 0, 2)], [(1, 2, 4)]]
    assert mode._pack_fields([(0, 0), (1, 7)], 3) == [[(1, 0, 3)], [(1, 3, 6)], [(1, 6, 7)]]
    assert mode._pack_fields([], 3) == []
