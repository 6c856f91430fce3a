"""Per-iteration time of F fields tempered TOGETHER (FieldSetTemperedSampler, psfmc_pt_run_fields) against the same
fields tempered one after another, each with DeviceTemperedSampler on a context of its own (psfmc_pt_run), for
F in {1, 4, 8} fields of 128^2 (PS + 1 Sersic), W in {22, 64} walkers and T in {4, 16} rungs.  An iteration is one
iteration of every field's ladder.  Each figure covers whole sample() calls of at least --seconds after a warm-up of
the same length; the last column is what the host's draws of the random numbers cost per iteration, alone.  One JSON
line per configuration, a table at the end.
Usage: python tools/time_fields_tempered.py [--side 128] [--fields 1 4 8] [--walkers 22 64] [--temps 4 16]
[--seconds 1.5] [--block 64] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import synth_field                                      # noqa: E402
from psfmc_amd import FieldSet, FieldSetTemperedSampler, MultiComponentModel      # noqa: E402
from psfmc_amd.ModelComponents import Configuration, PointSource, Sersic          # noqa: E402
from psfmc_amd.distributions import Uniform, WeibullMinimum                       # noqa: E402
from psfmc_amd.sampler import DeviceTemperedSampler, default_betas                # noqa: E402


def build(side, seed, max_walkers):
    """The synthetic field `seed` with the priors of synth_field.model_file_text."""
    fld = synth_field.make_field(side, 1, seed=seed)
    c = np.array((side / 2 + 0.5,) * 2)
    comps = [Configuration(fld['sci'], fld['ivm'], fld['psf'], fld['psf_ivm'], mag_zeropoint=fld['mag_zp']),
             PointSource(xy=Uniform(loc=c - 8, scale=16 * np.ones(2)), mag=Uniform(loc=18.0, scale=2.0)),
             Sersic(xy=Uniform(loc=c - 8, scale=16 * np.ones(2)), mag=Uniform(loc=19.0, scale=5.0),
                    reff=Uniform(loc=2.0, scale=side / 16.0), reff_b=Uniform(loc=2.0, scale=side / 16.0),
                    index=WeibullMinimum(c=1.5, scale=4), angle=Uniform(loc=0, scale=180), angle_degrees=True)]
    return MultiComponentModel(comps, backend='fused', max_walkers=max_walkers), fld


def run_together(sampler, p0, iters):
    sampler.reset()
    for f, sub in enumerate(sampler.fields):
        sub.random_state = np.random.RandomState(1 + f).get_state()
    t0 = time.perf_counter()
    for _ in sampler.sample(p0, iterations=iters):
        pass
    return time.perf_counter() - t0


def run_in_turn(samplers, p0, iters):
    total = 0.0
    for f, s in enumerate(samplers):
        s.reset()
        s.random_state = np.random.RandomState(1 + f).get_state()
        t0 = time.perf_counter()
        for _ in s.sample(p0[f], iterations=iters):
            pass
        total += time.perf_counter() - t0
    return total


def draw_ms(sampler, block):
    """ms per iteration the host spends drawing every field's random numbers of a block (they are drawn while the GPU
    runs the block before, so an iteration takes the longer of the two)."""
    t0 = time.perf_counter()
    for sub in sampler.fields:
        sub._draw(block)
    return (time.perf_counter() - t0) / block * 1e3


def timed(run, block, seconds):
    """ms per iteration over whole sample() calls of at least `seconds`: the second of two runs of one block sizes
    the timed run (the first pays the one-time costs), a warm-up of the timed length, then the timed run."""
    run(block)
    per_iter = run(block) / block
    iters = max(block, int(np.ceil(seconds / per_iter / block)) * block)
    run(iters)
    return run(iters) / iters * 1e3, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=128)
    ap.add_argument('--fields', type=int, nargs='+', default=[1, 4, 8])
    ap.add_argument('--walkers', type=int, nargs='+', default=[22, 64])
    ap.add_argument('--temps', type=int, nargs='+', default=[4, 16])
    ap.add_argument('--seconds', type=float, default=1.5)
    ap.add_argument('--block', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    n_max, cap = max(args.fields), max(args.walkers) * max(args.temps)
    own = [build(args.side, f, cap) for f in range(n_max)]
    rows = []
    for n_f in args.fields:
        fs = FieldSet([build(args.side, f, 1)[0] for f in range(n_f)], max_walkers=n_f * cap)
        for w in args.walkers:
            for t in args.temps:
                betas = default_betas(t, 1e4)
                p0 = np.array([synth_field.draw_walkers(args.side, 1, t * w, seed=2 + f, near_truth=fld['truth'])
                               .reshape(t, w, -1) for f, (_, fld) in enumerate(own[:n_f])])
                together = FieldSetTemperedSampler(w, fs, betas=betas, block=args.block)
                ms_set, it_set = timed(lambda n: run_together(together, p0, n), args.block, args.seconds)
                ms_draw = draw_ms(together, args.block)
                solos = [DeviceTemperedSampler(w, m, betas=betas, block=args.block) for m, _ in own[:n_f]]
                ms_own, it_own = timed(lambda n: run_in_turn(solos, p0, n), args.block, args.seconds)
                row = dict(side=args.side, fields=n_f, walkers=w, temps=t, together_ms_per_iter=round(ms_set, 4),
                           in_turn_ms_per_iter=round(ms_own, 4), gain=round(ms_own / ms_set, 3),
                           host_draw_ms_per_iter=round(ms_draw, 4),
                           together_iters=it_set, in_turn_iters=it_own)
                rows.append(row)
                print(json.dumps(row), flush=True)
        fs.close()
    for m, _ in own:
        m.close()
    lines = ['side  F    W   T   together ms/it  in turn ms/it  in turn / together  host draws ms/it']
    for r in rows:
        lines.append('%4d %2d %4d %3d %15.3f %14.3f %18.2f %17.3f' % (
            r['side'], r['fields'], r['walkers'], r['temps'], r['together_ms_per_iter'], r['in_turn_ms_per_iter'],
            r['gain'], r['host_draw_ms_per_iter']))
    print('\n'.join(lines))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
