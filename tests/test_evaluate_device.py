"""`ShardedLogPosterior.evaluate_device` (walkers resident on the GPU) with a world of one: it is ordered after
the caller's stream, its result is ordered before the caller's later work, and a tensor the library could not
read as [W, num_params] float64 on the model's device is refused before anything is launched."""
import numpy as np
import pytest

import synth_field
from test_gpu_fullsize import make_model


def sharded_model():
    from psfmc_amd.parallel import ShardedLogPosterior
    model, fld = make_model(256, 1, 'fused', max_walkers=16)
    return model, fld, ShardedLogPosterior(model)


@pytest.mark.gpu
def test_evaluate_device_waits_for_the_callers_stream():
    """theta_dev is written by a copy queued behind a long kernel on torch's current stream: evaluate_device must
    read it only after that copy, and `out.cpu()` on the current stream must see the finished result."""
    import torch
    model, fld, sharded = sharded_model()
    theta = np.vstack([fld['truth'][None, :], synth_field.draw_walkers(256, 1, 7, seed=3)])
    want = model.log_posterior_batch(theta)
    assert np.isfinite(want).all()
    dev = torch.device('cuda:%d' % model._device)
    src = torch.from_numpy(theta).to(dev)
    # a first call creates the rank group's side stream (the one point where it used to wait for the caller)
    assert np.array_equal(sharded.evaluate_device(src).cpu().numpy(), want)
    theta_dev = torch.full(theta.shape, float('nan'), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    torch.cuda._sleep(100_000_000)                # tens of ms of busy kernel on the current stream ...
    theta_dev.copy_(src)                          # ... and the real vectors behind it
    out = sharded.evaluate_device(theta_dev)
    assert np.array_equal(out.cpu().numpy(), want)
    model.close()


def _rejected(theta_dev, match):
    model, _, sharded = sharded_model()
    with pytest.raises(ValueError, match=match):
        sharded.evaluate_device(theta_dev)
    assert model._engine is None                  # refused before the context was even created


def _params():
    model, _, _ = sharded_model()
    return model.num_params


def test_evaluate_device_rejects_float32():
    import torch
    _rejected(torch.zeros((4, _params()), dtype=torch.float32), 'float64')


def test_evaluate_device_rejects_wrong_width():
    import torch
    _rejected(torch.zeros((4, _params() + 1), dtype=torch.float64), r'\[W, ')


def test_evaluate_device_rejects_one_dimensional():
    import torch
    _rejected(torch.zeros(_params(), dtype=torch.float64), r'\[W, ')


def test_evaluate_device_rejects_non_contiguous():
    import torch
    _rejected(torch.zeros((4, 2 * _params()), dtype=torch.float64)[:, ::2], 'contiguous')


def test_evaluate_device_rejects_host_tensor():
    import torch
    _rejected(torch.zeros((4, _params()), dtype=torch.float64), 'must be on cuda')


def test_evaluate_device_rejects_non_tensor():
    _rejected(np.zeros((4, _params())), 'torch tensor')
