#!/usr/bin/env python3
"""Throughput of a joint fit (`JointModel`: one parameter vector per walker over F fields) against the same
fields as a FieldSet of independent ensembles (one MI355X), F = 1, 2 and 4 fields of 256^2, 256 walkers:

  joint      log-posteriors/s of joint walkers (raw vectors resident in HBM, psfmc_eval_theta_joint_device),
             the field evaluations/s behind them (F per walker), and device-sampler iterations/s
             (DeviceEnsembleSampler, one ensemble of 256 joint walkers)
  fieldset   the same F fields with 256 walkers EACH (psfmc_eval_theta_device_fields: field evaluations/s) and
             FieldSetSampler iterations/s (F ensembles of 256 walkers stepped together)

A joint walker over F fields is F field evaluations, so joint walkers/s x F is the number to hold against the
FieldSet's field evaluations/s.  Every field: 1 PointSource + 1 Sersic, fp64.
  tools/time_joint_fit.py [--fields 1,2,4] [--iters 20] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
import numpy as np                                    # noqa: E402
import torch                                          # noqa: E402

from bench import timed_calls                         # noqa: E402
from time_mixed_fields import make_model              # noqa: E402

SIDE, PSF_SIDE, N_W = 256, 25, 256
PER_FIELD = ('0_PointSource_mag', '0_PointSource_xy', '1_Sersic_xy')


def _models(n_f):
    """n_f synthetic 256^2 fields (own noise and PSF draws, the same priors) and their near-truth walkers."""
    probs = [make_model(SIDE, SIDE, PSF_SIDE, 200 + f, N_W) for f in range(n_f)]
    return [m for m, _ in probs], [t for _, t in probs]


def _run_sampler(sampler, p0, iters):
    """Iterations/s of `iters` iterations in one block, after a short warm-up."""
    for _ in sampler.sample(p0, iterations=2):
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in sampler.sample(p0, iterations=iters):
        pass
    torch.cuda.synchronize()
    return iters / (time.perf_counter() - t0)


def time_joint(n_f, iters, dev, sync):
    from psfmc_amd import DeviceEnsembleSampler, JointModel
    models, thetas = _models(n_f)
    joint = JointModel(models, per_field=PER_FIELD, max_walkers=n_f * N_W)
    theta = np.zeros((N_W, joint.num_params))
    for f, t in enumerate(thetas):
        theta[:, joint.field_columns(f)] = t
    th = torch.from_numpy(theta).to(dev)
    out = torch.empty(N_W, dtype=torch.float64, device=dev)
    ctx = joint.context
    per_call, n = timed_calls(lambda: ctx.logpost_theta_joint_device(N_W, th.data_ptr(), out.data_ptr()), sync)
    got = out.cpu().numpy()
    sampler = DeviceEnsembleSampler(N_W, joint, block=iters)
    sampler.random_state = np.random.RandomState(5).get_state()
    its = _run_sampler(sampler, theta, iters)
    rec = {'joint_lnpost_per_s': N_W / per_call, 'field_evals_per_s': n_f * N_W / per_call, 'calls': n,
           'finite': int(np.isfinite(got).sum()), 'num_params': joint.num_params,
           'sampler_iters_per_s': its, 'acceptance': float(sampler.acceptance_fraction.mean()),
           'transform': [int(ctx.get_option('transform_ny')), int(ctx.get_option('transform_nx'))]}
    joint.close()
    return rec


def time_fieldset(n_f, iters, dev, sync):
    from psfmc_amd import FieldSet, FieldSetSampler
    models, thetas = _models(n_f)
    fs = FieldSet(models, max_walkers=n_f * N_W)
    th = torch.from_numpy(np.concatenate(thetas)).to(dev)
    out = torch.empty(n_f * N_W, dtype=torch.float64, device=dev)
    seg_f, seg_n = list(range(n_f)), [N_W] * n_f
    per_call, n = timed_calls(lambda: fs.context.logpost_theta_device(seg_f, seg_n, th.data_ptr(), out.data_ptr()),
                              sync)
    sampler = FieldSetSampler(N_W, fs, block=iters)
    for f, sub in enumerate(sampler.fields):
        sub.random_state = np.random.RandomState(10 + f).get_state()
    its = _run_sampler(sampler, np.array(thetas), iters)
    rec = {'field_evals_per_s': n_f * N_W / per_call, 'calls': n, 'sampler_iters_per_s': its,
           'finite': int(np.isfinite(out.cpu().numpy()).sum())}
    fs.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fields', default='1,2,4')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    sync = lambda: torch.cuda.synchronize(dev)
    res = {'workload': 'F fields of %d^2 (%d-pixel PSF), %d walkers, 1 PointSource + 1 Sersic, fp64; joint: '
                       'Sersic structure and magnitude shared, %s per field' % (SIDE, PSF_SIDE, N_W, list(PER_FIELD)),
           'device': torch.cuda.get_device_name(dev)}
    for n_f in (int(v) for v in args.fields.split(',')):
        res['F=%d' % n_f] = {'joint': time_joint(n_f, args.iters, dev, sync),
                             'fieldset': time_fieldset(n_f, args.iters, dev, sync)}
        print(json.dumps({'F': n_f, **res['F=%d' % n_f]}), flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
