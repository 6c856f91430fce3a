"""
psfmc_amd -- MI355X-native batched log-posterior for psfMC-style MCMC surface
brightness modelling.  Public names mirror the reference package `psfMC`.
"""
from .models import MultiComponentModel, FieldSet, JointModel
from .ModelComponents import Moffat, Ferrer, Tied
from .batch import BatchLogPosterior
from .sampler import (EnsembleSampler, DeviceEnsembleSampler, FieldSetSampler, TemperedEnsembleSampler,
                      DeviceTemperedSampler, FieldSetTemperedSampler, default_betas, StretchMove, DEMove)
from .parallel import RankGroup, ShardedLogPosterior
from .fitting import (model_galaxy_mcmc, model_fields_mcmc, model_joint_mcmc, model_galaxy_ptmcmc,
                      model_joint_ptmcmc, model_fields_ptmcmc)
from .database import load_database
from .mode import find_mode, find_modes

__version__ = '0.1.0'
__all__ = ['MultiComponentModel', 'FieldSet', 'JointModel', 'BatchLogPosterior', 'EnsembleSampler',
           'DeviceEnsembleSampler', 'FieldSetSampler', 'TemperedEnsembleSampler', 'DeviceTemperedSampler',
           'default_betas', 'RankGroup', 'ShardedLogPosterior', 'model_galaxy_mcmc', 'model_fields_mcmc',
           'model_joint_mcmc', 'model_galaxy_ptmcmc', 'model_joint_ptmcmc', 'load_database', 'Moffat', 'Ferrer',
           'StretchMove', 'DEMove', 'FieldSetTemperedSampler', 'model_fields_ptmcmc',
           'find_mode', 'find_modes', 'Tied']
