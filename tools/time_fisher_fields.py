#!/usr/bin/env python3
"""Timings of the several-field Fisher entries (profiles/fisher_fields_timing.txt; the bar: a one-call form is not
slower than the loop it replaces).

  python3 tools/time_fisher_fields.py            for 8 and 64 fields of 64^2 and 128^2 (sky + point source + Sersic,
                                                 K = 11): us per `FieldSet.fisher` call of all fields beside the loop
                                                 `fs.models[f].fisher` over them; for 3 exposures, `JointModel.fisher`
                                                 (positions and sky per exposure, K_joint = 21) beside three per-field
                                                 stencils over ALL joint columns; and `find_modes` of 8 fields beside 8
                                                 `find_mode` calls, with the share of the time spent in device calls
  python3 tools/time_fisher_fields.py --loops [--package DIR]
                                                 the loops alone, which is all a commit without `FieldSet.fisher` offers;
                                                 DIR: the directory that holds THAT commit's built psfmc_amd package, to
                                                 time its loop instead of this tree's"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]
sys.path.insert(0, sys.argv[sys.argv.index('--package') + 1] if '--package' in sys.argv else ROOT)
SIDES, COUNTS, REPS = (64, 128), (8, 64), 30
K = 11


def _model(side, seed):
    import numpy as np
    import synth_field
    from psfmc_amd import MultiComponentModel
    from psfmc_amd.ModelComponents import Configuration, PointSource, Sersic, Sky
    from psfmc_amd.distributions import Normal, Uniform, WeibullMinimum
    fld = synth_field.make_field(side, 1, seed=seed)
    c = np.array((side / 2 + 0.5,) * 2)
    comps = [Configuration(fld['sci'], fld['ivm'], fld['psf'], fld['psf_ivm'], mag_zeropoint=fld['mag_zp']),
             Sky(adu=Normal(loc=0.0, scale=0.01)),
             PointSource(xy=Uniform(loc=c - 8, scale=16 * np.ones(2)), mag=Uniform(loc=18.0, scale=2.0)),
             Sersic(xy=Uniform(loc=c - 8, scale=16 * np.ones(2)), mag=Uniform(loc=19.0, scale=5.0),
                    reff=Uniform(loc=2.0, scale=side / 16.0), reff_b=Uniform(loc=2.0, scale=side / 16.0),
                    index=WeibullMinimum(c=1.5, scale=4), angle=Uniform(loc=0, scale=180), angle_degrees=True)]
    return MultiComponentModel(comps, backend='fused', max_walkers=1), np.concatenate([[0.0], fld['truth']])


def _time(call, reps=REPS):
    for _ in range(3):
        call()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return (time.perf_counter() - t0) / reps * 1e6


def sets(loops_only):
    from psfmc_amd import FieldSet
    for side in SIDES:
        for n in COUNTS:
            made = [_model(side, seed) for seed in range(n)]
            fs = FieldSet([m for m, _ in made], max_walkers=n * (2 * K + 1))
            thetas = [t for _, t in made]
            loop = _time(lambda: [fs.models[f].fisher(thetas[f]) for f in range(n)])
            line = '%3d fields of %3d^2, K = %d: loop of fs.models[f].fisher %9.1f us' % (n, side, K, loop)
            if not loops_only:
                one = _time(lambda: fs.fisher(thetas))
                line += ';  one FieldSet.fisher call %9.1f us;  loop / call %.2f' % (one, loop / one)
            print(line + '  (host call to host result, %d repeats)' % REPS)
            fs.close()


def joint():
    import numpy as np
    from psfmc_amd import JointModel
    for side in SIDES:
        made = [_model(side, 0) for _ in range(3)]
        models = [m for m, _ in made]
        per_field = [n for n in models[0].param_names if n.endswith('_xy') or 'Sky' in n]
        jm = JointModel(models, per_field=per_field, max_walkers=3 * (2 * 21 + 1))
        theta = np.zeros(jm.num_params)
        for f, (_, t) in enumerate(made):
            theta[jm.field_columns(f)] = t
        from psfmc_amd import mode
        columns = mode.default_columns(jm)
        k_joint = len(columns)
        step = mode.default_steps(jm, theta, columns)

        def wide():
            # what the one-field entry offers a joint fit: per exposure a stencil over ALL joint columns, 2 K_joint + 1
            # images of which 2 K_field + 1 differ, its derived rows included as JointModel.fisher's are
            vecs = mode.stencil(theta, step, columns)[0]
            return [m.engine.fisher_rows(m.derived_rows(vecs[:, jm.field_columns(f)])[None], 0.5 / step)
                    for f, m in enumerate(jm.field_models)]
        one, loop = _time(lambda: jm.fisher(theta, step=step, columns=columns)), _time(wide)
        print('3 exposures of %3d^2, K_field = %d, K_joint = %d: JointModel.fisher %9.1f us;  three per-exposure stencils '
              'over all joint columns (%d walkers each) %9.1f us;  loop / call %.2f' % (
                  side, K, k_joint, one, 2 * k_joint + 1, loop, loop / one))
        # the device calls alone, rows made beforehand: 3 x 23 walkers and the link against 3 x 43 walkers
        place = np.full(jm.num_params, -1)
        place[columns] = np.arange(k_joint)
        col_of = np.array([place[jm.field_columns(f)] for f in range(3)])
        vecs = mode.stencil(theta, step, columns)[0]
        wide_rows = [m.derived_rows(vecs[:, jm.field_columns(f)])[None] for f, m in enumerate(jm.field_models)]
        own = [mode.stencil(theta[jm.field_columns(f)], step[:, col_of[f]], np.arange(K))[0] for f in range(3)]
        rows = np.stack([m.derived_rows(v) for m, v in zip(jm.field_models, own)])[None]
        inv2h = np.stack([0.5 / step[0, col_of[f]] for f in range(3)])[None]
        ctx = jm.context
        one = _time(lambda: ctx.fisher_rows_joint(col_of, rows, inv2h, k_joint))
        loop = _time(lambda: [m.engine.fisher_rows(r, 0.5 / step) for m, r in zip(jm.field_models, wide_rows)])
        print('    the device calls alone: fisher_rows_joint %9.1f us;  three fisher_rows calls %9.1f us;  loop / call %.2f'
              % (one, loop, loop / one))
        jm.close()


def searches():
    import numpy as np
    from psfmc_amd import FieldSet, engine, find_mode, find_modes
    n, side = 8, 64
    made = [_model(side, seed) for seed in range(n)]
    fs = FieldSet([m for m, _ in made], max_walkers=n * 4 * (2 * K + 1))
    starts = [t[None, :] for _, t in made]
    spent = [0.0]

    def timed(fn):
        def call(*args, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*args, **kw)
            finally:
                spent[0] += time.perf_counter() - t0
        return call
    for name in ('fisher_rows', 'fisher_rows_fields', 'logpost_theta'):
        setattr(fs.context, name, timed(getattr(fs.context, name)))
    for label, call in (('find_modes of the set', lambda: find_modes(fs, start=starts)),
                        ('8 find_mode calls', lambda: [find_mode(fs.models[f], start=starts[f]) for f in range(n)])):
        call()
        spent[0] = 0.0
        t0 = time.perf_counter()
        call()
        wall = time.perf_counter() - t0
        print('%d fields of %d^2 from the truth, %s: %.1f ms, %.1f ms of it (%.0f %%) inside the context\'s device '
              'calls' % (n, side, label, wall * 1e3, spent[0] * 1e3, 100.0 * spent[0] / wall))
    fs.close()


if __name__ == '__main__':
    loops_only = '--loops' in sys.argv[1:]
    sets(loops_only)
    if not loops_only:
        print('image passes: mixed (the records of all fields of a call in common passes of chunk_walkers walkers)')
        joint()
        searches()
