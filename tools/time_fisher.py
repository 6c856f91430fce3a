#!/usr/bin/env python3
"""Timings of the Fisher entry and of fits started from the mode (profiles/fisher_timing.txt; reports, no bar).

  python3 tools/time_fisher.py             us per `model.fisher` call (K = 10: point source + Sersic) at 128^2 and 256^2
                                           beside `log_posterior_batch` of the same 2K+1 = 21 walkers, and -- for the
                                           J0005-0006 example with 38 chains -- the iteration at which the ensemble's
                                           median log-posterior first comes within K of its final maximum, for
                                           start='prior' and start='mode'
  rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/time_fisher.py --trace
  python3 tools/time_fisher.py --analyse OUT/.../*_kernel_trace.csv
                                           the share of the Gram kernel (and of the stash and finish kernels) in the
                                           kernel time of the traced `fisher` calls"""
import csv
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]
SIZES, REPS = (128, 256), 200


def _model(side):
    from test_gpu_fullsize import make_model
    return make_model(side, 1, 'fused', max_walkers=64)


def timings():
    import numpy as np
    from psfmc_amd import mode
    for side in SIZES:
        model, fld = _model(side)
        theta = fld['truth']
        columns = mode.default_columns(model)
        step = mode.default_steps(model, theta, columns)
        vecs = mode.stencil(theta, step, columns)[0]
        out = {}
        for name, call in (('fisher', lambda: model.fisher(theta, step=step, columns=columns)),
                           ('log_posterior_batch of the 21 walkers', lambda: model.log_posterior_batch(vecs))):
            for _ in range(20):
                call()
            t0 = time.perf_counter()
            for _ in range(REPS):
                call()
            out[name] = (time.perf_counter() - t0) / REPS * 1e6
        print('%4d^2  K = %d: ' % (side, len(columns)) + ';  '.join('%s %.1f us' % kv for kv in out.items()) +
              '  (host call to host result, %d calls each)' % REPS)
        model.close()


def trace():
    from psfmc_amd import mode
    for side in SIZES:
        model, fld = _model(side)
        columns = mode.default_columns(model)
        step = mode.default_steps(model, fld['truth'], columns)
        for _ in range(50):
            model.fisher(fld['truth'], step=step, columns=columns)
        model.close()


def analyse(path):
    rows = list(csv.DictReader(open(path)))
    total, part = 0.0, {'k_fisher_gram': 0.0, 'k_fisher_stash': 0.0, 'k_fisher_finish': 0.0}
    for r in rows:
        dur = (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
        total += dur
        for key in part:
            if key in r['Kernel_Name']:
                part[key] += dur
    print('kernel time of the traced fisher calls (%d launches, set-up included): %.0f us' % (len(rows), total))
    for key, val in part.items():
        print('  %-16s %8.0f us  %5.1f %%' % (key, val, 100.0 * val / total))


def example_fits(iterations=3000):
    """The flow of `model_galaxy_mcmc` without burn-in and outputs: the device sampler from prior draws and from
    the mode (`fitting._start_from_mode`, which is what start='mode' runs)."""
    import numpy as np
    from psfmc_amd import MultiComponentModel, DeviceEnsembleSampler, EnsembleSampler, fitting, mode
    src = os.path.join(ROOT, 'tests', 'golden', 'example')
    for start in ('prior', 'mode'):
        with tempfile.TemporaryDirectory() as tmp:
            for name in os.listdir(src):
                if os.path.isfile(os.path.join(src, name)):
                    shutil.copy(os.path.join(src, name), tmp)
            model = MultiComponentModel(os.path.join(tmp, 'model_example.py'), max_walkers=1024)
            k = len(mode.default_columns(model))
            model.engine                                                          # (registers the priors)
            sampler = (EnsembleSampler(38, model.num_params, batch_lnpostfn=model.log_posterior_batch)
                       if model._host_priors else DeviceEnsembleSampler(38, model))
            fitting._seed(sampler, 7)
            np.random.seed(42)
            model.log_posterior_batch(model.init_params_from_priors(2))          # (context set-up is not the search)
            t0 = time.perf_counter()
            if start == 'mode':
                pos, meta = fitting._start_from_mode(sampler, model, 38)
            else:
                pos, meta = model.init_params_from_priors(38), {}
            t1 = time.perf_counter()
            sampler.run_mcmc(pos, iterations)
            t2 = time.perf_counter()
            lnp = np.asarray(sampler.lnprobability)
            median, top = np.median(lnp, axis=0), np.max(lnp)
            near = np.flatnonzero(median >= top - k)
            print('J0005-0006 example, 38 chains, %d iterations, start=%r: median log-posterior within K = %d of the '
                  'final maximum %.2f first at iteration %s (median at iteration 0: %.2f; start positions %.3f s, '
                  'sampling %.3f s%s)' % (iterations, start, k, top, near[0] if len(near) else 'never', median[0],
                                         t1 - t0, t2 - t1, ', MCMODELP %.2f' % meta['MCMODELP'] if meta else ''))
            model.close()


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--analyse':
        analyse(sys.argv[2])
    elif len(sys.argv) > 1 and sys.argv[1] == '--trace':
        trace()
    else:
        timings()
        example_fits()
