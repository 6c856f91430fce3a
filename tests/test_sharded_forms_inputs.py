"""The inputs of tests/test_gpu_sharded_forms.py, checked without a GPU: the host `EnsembleSampler` fed the contract's
log-posterior (tests/shard_driver.py `contract_of`) on the same fields, models, start ensembles and random states must
meet every condition that keeps the GPU test from passing vacuously AT LEAST THREE TIMES OVER, so that the device run
-- whose log-posteriors differ from the contract's by 1e-9 |ll| at most -- does not sit on an edge:

  * >= 3 proposals with a non-finite prior (a PSF index outside the support) in blocks with lo > 0,
  * >= 3 accepted moves in every non-empty block -- per (half, rank) with 20 walkers; per rank (its block of either
    half) in the six-walker case, whose blocks are single walkers with six proposals each,
  * >= 3 evaluated proposals on each of the two PSFs in blocks with lo > 0.

The seeds of `shard_driver.CASES` were chosen by this test."""
import numpy as np
import pytest

import shard_driver as sd
from psfmc_amd.sampler import EnsembleSampler

HOST_CASES = sorted({c[1:] for c in sd.CASES}, key=str)


@pytest.mark.parametrize('kind,shape,ranks,n_w,seed', HOST_CASES, ids=sd.case_id)
def test_run_meets_its_conditions(kind, shape, ranks, n_w, seed):
    model = sd.make_models(kind, shape, 1)[0]
    dim = model.num_params
    assert dim <= 10 and (n_w >= 2 * dim or n_w == 6)
    p0 = sd.start_ensemble(model, shape, n_w, seed)
    lnpost = lambda thetas: np.array([sd.contract_of(kind, shape, model, t)[0] for t in thetas])
    host = EnsembleSampler(n_w, dim, batch_lnpostfn=lnpost, live_dangerously=n_w < 2 * dim)
    host.random_state = sd.random_state(seed)
    z, _, partner, _ = sd.draw(sd.random_state(seed), sd.N_ITER, n_w, dim)
    list(host.sample(p0, iterations=sd.N_ITER))
    q, acc = sd.replay(p0, host.chain, z, partner)
    assert acc.sum() == host.naccepted.sum()
    prior = model.log_priors_batch(q.reshape(-1, dim)).reshape(acc.shape)
    cond = sd.conditions(q, prior, acc, ranks)
    print(kind, shape, ranks, n_w, cond)
    assert cond['blocks'] == ([4, 3, 3] if n_w == 20 else [1, 1, 1, 0])
    assert cond['outside_behind'] >= 3 and cond['psf_min'] >= 3, cond
    assert cond['accepted_min' if n_w >= 20 else 'accepted_rank_min'] >= 3, cond
