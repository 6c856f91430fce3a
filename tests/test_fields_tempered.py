"""Every field of a FieldSet tempered together, the part that needs no GPU: the names are exported, and
model_fields_ptmcmc refuses an odd or too small `chains`, a bad ladder and a wrong number of random states
before any context is made."""
import numpy as np
import pytest

from test_joint_link import make_field, make_model, no_gpu   # noqa: F401 (no_gpu is a fixture)


@pytest.fixture
def models():
    return [make_model(make_field(64, 64, 11, seed=70 + f)) for f in range(2)]


def test_the_names_are_exported():
    import psfmc_amd
    from psfmc_amd import fitting, sampler
    assert psfmc_amd.model_fields_ptmcmc is fitting.model_fields_ptmcmc
    assert psfmc_amd.FieldSetTemperedSampler is sampler.FieldSetTemperedSampler
    assert {'model_fields_ptmcmc', 'FieldSetTemperedSampler'} <= set(psfmc_amd.__all__)
    assert callable(psfmc_amd.FieldSet.log_likelihood_and_prior_batch)
    assert callable(psfmc_amd.engine.FieldSetContext.eval_split)
    assert callable(psfmc_amd.engine.FieldSetContext.pt_run_fields)


@pytest.mark.parametrize('chains', [7, 0, 1])
def test_an_odd_or_too_small_number_of_chains_is_refused(no_gpu, models, tmp_path, chains):
    from psfmc_amd import model_fields_ptmcmc
    with pytest.raises(ValueError, match='chains must be an even number'):
        model_fields_ptmcmc(models, output_names=[str(tmp_path / 'a'), str(tmp_path / 'b')], iterations=2,
                            chains=chains, ntemps=3, tmax=10.0, quiet=True)
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize('betas', [[1.0, 0.5], [0.9, 0.5, 0.0], [1.0, 0.5, 0.5, 0.0], [1.0, np.nan, 0.0], []])
def test_a_bad_ladder_is_refused(no_gpu, models, tmp_path, betas):
    from psfmc_amd import model_fields_ptmcmc
    with pytest.raises(ValueError, match='ladder|rung'):
        model_fields_ptmcmc(models, output_names=[str(tmp_path / 'a'), str(tmp_path / 'b')], iterations=2,
                            chains=8, betas=betas, quiet=True)
    assert not list(tmp_path.iterdir())


def test_bad_default_ladder_arguments_are_refused(no_gpu, models):
    from psfmc_amd import model_fields_ptmcmc
    with pytest.raises(ValueError, match='tmax'):
        model_fields_ptmcmc(models, chains=8, ntemps=3, tmax=1.0)
    with pytest.raises(ValueError, match='ntemps'):
        model_fields_ptmcmc(models, chains=8, ntemps=0)


def test_a_wrong_number_of_random_states_is_refused(no_gpu, models, tmp_path):
    from psfmc_amd import model_fields_ptmcmc
    with pytest.raises(ValueError, match='one per field'):
        model_fields_ptmcmc(models, output_names=[str(tmp_path / 'a'), str(tmp_path / 'b')], iterations=2,
                            chains=8, ntemps=3, tmax=10.0, random_states=[1, 2, 3], quiet=True)
    with pytest.raises(ValueError, match='start_positions'):
        model_fields_ptmcmc(models, output_names=[str(tmp_path / 'a'), str(tmp_path / 'b')], iterations=2,
                            chains=8, ntemps=3, tmax=10.0, start_positions=[np.zeros((3, 8, 4))], quiet=True)
    assert not list(tmp_path.iterdir())
