"""Iterations per second of the tempered and field-set device samplers by proposal move (`set_moves`), fields with
one PointSource and one Sersic:
  (1) `DeviceTemperedSampler`, T = 16 rungs of 22 walkers on one 128^2 field (psfmc_pt_run / psfmc_pt_move_run),
  (2) `FieldSetTemperedSampler`, T = 4 rungs of 22 walkers on each of eight 128^2 fields (psfmc_pt_run_fields /
      psfmc_pt_move_run_fields),
  (3) `FieldSetSampler`, eight 128^2 fields of 256 walkers (psfmc_stretch_run_fields / psfmc_pt_move_run_fields
      with one rung),
each with (a) no moves, (b) DEMove(), (c) the half-and-half mixture [(StretchMove(), 1), (DEMove(), 1)], (d)
StretchMove() through `set_moves` -- the proposals and the acceptance of (a) on the entry points of (b).  Each is
timed over whole `sample()` calls -- host draws, uploads and the chains' download included -- for at least `seconds`
after a warm-up.  Beside it, the host's share: the time the samplers' `_draw` takes per iteration on its own (the
draws of the next block run while the GPU works on the current one, so a run is never faster than its draws).
No pass/fail threshold.
usage: python3 tools/time_tempered_moves.py [seconds]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tools')]
import synth_field                                              # noqa: E402
from test_gpu_fullsize import make_model                        # noqa: E402
from psfmc_amd import FieldSet, FieldSetSampler, FieldSetTemperedSampler   # noqa: E402
from psfmc_amd.sampler import DEMove, DeviceTemperedSampler, StretchMove, default_betas   # noqa: E402

BLOCK, SIDE, N_F = 64, 128, 8
MOVES = (('(a) stretch (no moves)', None), ('(b) DEMove()', DEMove()),
         ('(c) stretch + DE, half and half', [(StretchMove(), 1), (DEMove(), 1)]),
         ('(d) StretchMove() by set_moves', StretchMove()))


def ladder_start(fld, n_t, n_w, seed):
    """[T, W, P]: rung 0 near the truth, the hotter rungs drawn from the priors."""
    p0 = [synth_field.draw_walkers(SIDE, 1, n_w, seed=seed, near_truth=fld['truth'], jitter=1e-3)]
    p0 += [synth_field.draw_walkers(SIDE, 1, n_w, seed=100 * seed + t) for t in range(1, n_t)]
    return np.array(p0)


def rate(sample, state, seconds):
    """sample(state, iterations) -> the next state; (iterations per second over at least `seconds`, the state)."""
    state = sample(state, BLOCK)                                   # warm-up
    done, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        state = sample(state, 2 * BLOCK)
        done += 2 * BLOCK
    return done / (time.perf_counter() - t0)


def draw_us(sampler):
    """Microseconds per iteration of the host's random draws alone (every field's `_draw`), over three blocks."""
    members = getattr(sampler, 'fields', [sampler])
    t0 = time.perf_counter()
    for _ in range(3):
        for m in members:
            m._draw(BLOCK)
    return (time.perf_counter() - t0) / (3 * BLOCK) * 1e6


def one_ladder(seconds):
    n_t, n_w = 16, 22
    model, fld = make_model(SIDE, 1, 'fused', max_walkers=n_t * n_w)
    betas = default_betas(n_t, 1e6)
    for tag, moves in MOVES:
        s = DeviceTemperedSampler(n_w, model, betas=betas, block=BLOCK)
        s.set_moves(moves)
        s.random_state = np.random.RandomState(5).get_state()

        def sample(state, n):
            for state in s.sample(*state[:3], iterations=n, storechain=False):
                pass
            return state
        yield ('T=16 x 22 walkers, one field', tag, rate(sample, (ladder_start(fld, n_t, n_w, 3), None, None), seconds),
               draw_us(s))
    model.close()


def field_ladders(seconds):
    n_t, n_w = 4, 22
    pairs = [make_model(SIDE, 1, 'fused', max_walkers=1, seed=s) for s in range(N_F)]
    fs = FieldSet([m for m, _ in pairs], max_walkers=N_F * n_t * n_w)
    p0 = np.array([ladder_start(fld, n_t, n_w, 3 + f) for f, (_, fld) in enumerate(pairs)])
    for tag, moves in MOVES:
        s = FieldSetTemperedSampler(n_w, fs, betas=default_betas(n_t, 50.0), block=BLOCK)
        s.set_moves(moves)
        for f, sub in enumerate(s.fields):
            sub.random_state = np.random.RandomState(5 + f).get_state()

        def sample(state, n):
            for out in s.sample(*state, iterations=n, storechain=False):
                pass
            return tuple(np.array([r[j] for r in out]) for j in range(3))
        yield 'T=4 x 22 walkers, eight fields', tag, rate(sample, (p0, None, None), seconds), draw_us(s)
    fs.close()


def field_ensembles(seconds):
    n_w = 256
    pairs = [make_model(SIDE, 1, 'fused', max_walkers=1, seed=s) for s in range(N_F)]
    fs = FieldSet([m for m, _ in pairs], max_walkers=N_F * n_w)
    p0 = np.array([synth_field.draw_walkers(SIDE, 1, n_w, seed=4 + f, near_truth=fld['truth'])
                   for f, (_, fld) in enumerate(pairs)])
    for tag, moves in MOVES:
        s = FieldSetSampler(n_w, fs, block=BLOCK)
        s.set_moves(moves)
        for f, sub in enumerate(s.fields):
            sub.random_state = np.random.RandomState(5 + f).get_state()

        def sample(state, n):
            for out in s.sample(*state, iterations=n, storechain=False):
                pass
            return tuple(np.array([r[j] for r in out]) for j in range(2))
        yield 'eight fields x 256 walkers', tag, rate(sample, (p0, None), seconds), draw_us(s)
    fs.close()


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 1.5
    for case in (one_ladder, field_ladders, field_ensembles):
        rows = list(case(seconds))
        base = rows[0][2]
        for what, tag, r, draws in rows:
            print('%d^2  %-32s %-34s %8.1f iterations/s  %8.1f us/iteration  time x%.3f of (a)  host draws alone '
                  '%6.1f us/iteration' % (SIDE, what, tag, r, 1e6 / r, base / r, draws), flush=True)


if __name__ == '__main__':
    main()
