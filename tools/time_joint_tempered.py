#!/usr/bin/env python3
"""Per-iteration time of a parallel-tempered JOINT fit (DeviceTemperedSampler on a JointModel,
psfmc_pt_run_joint) against the sum of the fields' own one-field tempered runs (psfmc_pt_run) at the same
ladder and ensemble, one MI355X.  Default: F = 2 fields of 128^2 (one PointSource + one Sersic each, positions
and the point-source magnitude per field), T = 16 rungs, W = 38 walkers per rung.  Whole `sample()` calls: host
draws and transfers included.
  tools/time_joint_tempered.py [--fields 2] [--side 128] [--temps 16] [--walkers 38] [--iters 400] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
import numpy as np                                    # noqa: E402

from time_mixed_fields import make_model              # noqa: E402

PSF_SIDE = 25
PER_FIELD = ('0_PointSource_mag', '0_PointSource_xy', '1_Sersic_xy')


def timed(sampler, p0, iters):
    """ms per iteration of `iters` iterations in one block, after a warm-up of the same length (the library's
    tempering state grows with the block: a shorter warm-up would leave a reallocation inside the timed run)."""
    list(sampler.sample(p0, iterations=iters))
    sampler.reset()
    t0 = time.perf_counter()
    list(sampler.sample(p0, iterations=iters))
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    from psfmc_amd import JointModel
    from psfmc_amd.sampler import DeviceTemperedSampler, default_betas
    ap = argparse.ArgumentParser()
    ap.add_argument('--fields', type=int, default=2)
    ap.add_argument('--side', type=int, default=128)
    ap.add_argument('--temps', type=int, default=16)
    ap.add_argument('--walkers', type=int, default=38)
    ap.add_argument('--iters', type=int, default=400)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    n_f, n_t, n_w = args.fields, args.temps, args.walkers
    betas = default_betas(n_t, 1e4)
    probs = [make_model(args.side, args.side, PSF_SIDE, 300 + f, n_t * n_w) for f in range(n_f)]
    # the fields' own runs: every rung starts near the truth (the time per iteration does not depend on it)
    own_ms = []
    for model, theta in probs:
        s = DeviceTemperedSampler(n_w, model, betas=betas, block=args.iters)
        s.random_state = np.random.RandomState(1).get_state()
        own_ms.append(timed(s, theta.reshape(n_t, n_w, -1), args.iters))
    joint = JointModel([m for m, _ in probs], per_field=PER_FIELD, max_walkers=n_t * n_w * n_f)
    p0 = np.zeros((n_t * n_w, joint.num_params))
    for f, (_, theta) in enumerate(probs):
        p0[:, joint.field_columns(f)] = theta
    s = DeviceTemperedSampler(n_w, joint, betas=betas, block=args.iters)
    s.random_state = np.random.RandomState(1).get_state()
    joint_ms = timed(s, p0.reshape(n_t, n_w, -1), args.iters)
    accept = float(s.acceptance_fraction.mean())
    row = dict(fields=n_f, side=args.side, temps=n_t, walkers=n_w, iters=args.iters, joint_params=joint.num_params,
               joint_ms_per_iter=round(joint_ms, 4), own_ms_per_iter=[round(v, 4) for v in own_ms],
               own_sum_ms_per_iter=round(sum(own_ms), 4), ratio=round(joint_ms / sum(own_ms), 3),
               joint_acceptance=round(accept, 3))
    print(json.dumps(row), flush=True)
    lines = ['F  side   T    W  P_joint  joint ms/it  one-field runs ms/it (sum)        joint / sum',
             '%d %5d %3d %4d %8d %12.3f  %s (%.3f) %12.3f' % (
                 n_f, args.side, n_t, n_w, joint.num_params, joint_ms, ' + '.join('%.3f' % v for v in own_ms),
                 sum(own_ms), joint_ms / sum(own_ms))]
    print('\n'.join(lines))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    joint.close()
    for model, _ in probs:
        model.close()


if __name__ == '__main__':
    main()
