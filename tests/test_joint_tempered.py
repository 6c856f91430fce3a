"""Parallel tempering of a joint fit, the part that needs no GPU: model_joint_ptmcmc refuses an odd `chains` and
a bad ladder before any context is made, JointModel has the split evaluation the tempered samplers call, and the
entry point is exported."""
import numpy as np
import pytest

from test_joint_link import POS, make_field, make_model, no_gpu   # noqa: F401 (no_gpu is a fixture)

# the two fields of tests/test_gpu_joint_tempered.py: unequal image and PSF sides
SHAPES = [(64, 64, 11), (64, 96, 13)]


@pytest.fixture
def models():
    return [make_model(make_field(ny, nx, pk, seed=60 + f)) for f, (ny, nx, pk) in enumerate(SHAPES)]


def test_the_entry_point_is_exported():
    import psfmc_amd
    from psfmc_amd import fitting
    assert psfmc_amd.model_joint_ptmcmc is fitting.model_joint_ptmcmc
    assert 'model_joint_ptmcmc' in psfmc_amd.__all__


def test_joint_model_has_the_split_evaluation(no_gpu, models):
    from psfmc_amd import JointModel
    joint = JointModel(models, per_field=POS)
    assert callable(joint.log_likelihood_and_prior_batch)
    assert joint._context is None


@pytest.mark.parametrize('chains', [7, 0, 1])
def test_an_odd_number_of_chains_is_refused(no_gpu, models, tmp_path, chains):
    from psfmc_amd import model_joint_ptmcmc
    with pytest.raises(ValueError, match='chains must be an even number'):
        model_joint_ptmcmc(models, per_field=POS, output_name=str(tmp_path / 'j'), iterations=2, chains=chains,
                           ntemps=3, tmax=10.0, quiet=True)
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize('betas', [[1.0, 0.5], [0.9, 0.5, 0.0], [1.0, 0.5, 0.5, 0.0], [1.0, np.nan, 0.0], []])
def test_a_bad_ladder_is_refused(no_gpu, models, tmp_path, betas):
    from psfmc_amd import model_joint_ptmcmc
    with pytest.raises(ValueError, match='ladder|rung'):
        model_joint_ptmcmc(models, per_field=POS, output_name=str(tmp_path / 'j'), iterations=2, chains=8,
                           betas=betas, quiet=True)
    assert not list(tmp_path.iterdir())


def test_bad_default_ladder_arguments_are_refused(no_gpu, models, tmp_path):
    from psfmc_amd import model_joint_ptmcmc
    with pytest.raises(ValueError, match='tmax'):
        model_joint_ptmcmc(models, per_field=POS, output_name=str(tmp_path / 'j'), chains=8, ntemps=3, tmax=1.0)
    with pytest.raises(ValueError, match='ntemps'):
        model_joint_ptmcmc(models, per_field=POS, output_name=str(tmp_path / 'j'), chains=8, ntemps=0)


def test_the_tempered_sampler_still_refuses_other_models(no_gpu):
    from psfmc_amd.sampler import DeviceTemperedSampler
    with pytest.raises(ValueError, match='JointModel'):
        DeviceTemperedSampler(8, object(), betas=[1.0, 0.0])
