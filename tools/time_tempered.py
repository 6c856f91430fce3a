"""Per-iteration time of the parallel-tempered device sampler (DeviceTemperedSampler, psfmc_pt_run) for
T in {1, 4, 8, 16} rungs x W in {22, 64, 256} walkers on 128^2 and 256^2 synthetic fields (PS + 1 Sersic), against
the stretch-move device sampler (DeviceEnsembleSampler) at the same W.  One JSON line per configuration, a table at
the end.  Usage: python tools/time_tempered.py [--sides 128 256] [--temps 1 4 8 16] [--walkers 22 64 256]
[--iters 40] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import synth_field                                      # noqa: E402
from psfmc_amd import MultiComponentModel, fits_io      # noqa: E402
from psfmc_amd.sampler import DeviceEnsembleSampler, DeviceTemperedSampler, default_betas   # noqa: E402


def build(side, directory, max_walkers):
    fld = synth_field.make_field(side, n_sersic=1, seed=0)
    for key, name in (('sci', 'sci.fits'), ('ivm', 'ivm.fits'), ('psf', 'psf.fits'), ('psf_ivm', 'psf_ivm.fits')):
        fits_io.write_image(os.path.join(directory, name), fld[key])
    path = os.path.join(directory, 'model.py')
    with open(path, 'w') as f:
        f.write(synth_field.model_file_text(side, 1))
    return MultiComponentModel(path, max_walkers=max_walkers), fld


def timed(sampler, p0, iters):
    # warm-up of the same length: the library's sampler state grows with the block, so a shorter warm-up would
    # leave a reallocation inside the timed run
    list(sampler.sample(p0, iterations=iters))
    sampler.reset()
    t0 = time.perf_counter()
    list(sampler.sample(p0, iterations=iters))
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sides', type=int, nargs='+', default=[128, 256])
    ap.add_argument('--temps', type=int, nargs='+', default=[1, 4, 8, 16])
    ap.add_argument('--walkers', type=int, nargs='+', default=[22, 64, 256])
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rows = []
    for side in args.sides:
        with tempfile.TemporaryDirectory() as tmp:
            model, fld = build(side, tmp, max(args.temps) * max(args.walkers))
            for w in args.walkers:
                base = synth_field.draw_walkers(side, 1, w * max(args.temps), seed=2, near_truth=fld['truth'])
                ref = DeviceEnsembleSampler(w, model, block=args.iters)
                ref.random_state = np.random.RandomState(1).get_state()
                ms_ref = timed(ref, base[:w], args.iters)
                for t in args.temps:
                    s = DeviceTemperedSampler(w, model, betas=default_betas(t, 1e4), block=args.iters)
                    s.random_state = np.random.RandomState(1).get_state()
                    ms = timed(s, base[:t * w].reshape(t, w, -1), args.iters)
                    row = dict(side=side, walkers=w, temps=t, ms_per_iter=round(ms, 4),
                               stretch_ms_per_iter=round(ms_ref, 4), ratio=round(ms / ms_ref, 3))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            model.close()
    lines = ['side  W    T   tempered ms/it  stretch ms/it  ratio']
    for r in rows:
        lines.append('%4d %4d %3d %14.3f %14.3f %6.2f' % (r['side'], r['walkers'], r['temps'], r['ms_per_iter'],
                                                         r['stretch_ms_per_iter'], r['ratio']))
    print('\n'.join(lines))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
