"""Iterations per second of `DeviceEnsembleSampler` by proposal move, on a 256^2 field with one PointSource and one
Sersic, at 22 and at 256 walkers:
  (a) moves=None with `speculate` 0 -- the plain two-half-step stretch path (three stages per half-step),
  (b) moves=None at the library's default (whole-iteration launches for small ensembles),
  (c) DEMove(),
  (d) the half-and-half mixture [(StretchMove(), 1), (DEMove(), 1)]
(c and d: psfmc_move_run, four stages per half-step).  Each is timed over whole `sample()` calls -- host draws,
uploads and the chain's download included -- for at least `seconds` after a warm-up.  No pass/fail threshold.
usage: python3 tools/time_moves.py [side] [seconds]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tools')]
import synth_field                                              # noqa: E402
from test_gpu_fullsize import make_model                        # noqa: E402
from psfmc_amd.sampler import DEMove, DeviceEnsembleSampler, StretchMove   # noqa: E402

BLOCK = 64


def rate(model, n_w, moves, p0, seconds):
    s = DeviceEnsembleSampler(n_w, model, moves=moves, block=BLOCK, live_dangerously=True)
    s.random_state = np.random.RandomState(5).get_state()
    pos, lnp = p0, None
    for pos, lnp, _ in s.sample(pos, iterations=BLOCK):            # warm-up
        pass
    done, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for pos, lnp, _ in s.sample(pos, lnprob0=lnp, iterations=2 * BLOCK, storechain=False):
            pass
        done += 2 * BLOCK
    return done / (time.perf_counter() - t0), s.acceptance_fraction.mean()


def main():
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    for n_w in (22, 256):
        model, fld = make_model(side, 1, 'fused', max_walkers=max(3 * n_w // 2 + 1, 64))
        p0 = synth_field.draw_walkers(side, 1, n_w, seed=4, near_truth=fld['truth'])
        eng = model.engine
        rows = []
        for tag, moves, speculate in (('(a) stretch, speculate 0', None, 0),
                                      ('(b) stretch, default', None, -1),
                                      ('(c) DEMove()', DEMove(), -1),
                                      ('(d) stretch + DE, half and half', [(StretchMove(), 1), (DEMove(), 1)], -1)):
            eng.set_option('speculate', speculate)
            before = eng.get_option('speculated_runs')
            r, acc = rate(model, n_w, moves, p0, seconds)
            rows.append((tag, r, acc, eng.get_option('speculated_runs') > before))
        eng.set_option('speculate', -1)
        base = rows[0][1]
        for tag, r, acc, spec in rows:
            print('%4d^2 P=%d %3d walkers  %-32s %8.1f iterations/s  %7.1f us/iteration  time x%.3f of (a)  '
                  'acceptance %.2f%s' % (side, model.num_params, n_w, tag, r, 1e6 / r, base / r, acc,
                                         '  [whole-iteration launches]' if spec else ''), flush=True)
        model.close()


if __name__ == '__main__':
    main()
