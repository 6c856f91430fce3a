#!/usr/bin/env python3
"""model_galaxy_mcmc iterations per second on the example field with priors of the newer device families
(include/psfmc_hip.h psfmc_set_priors): the host galaxy's Sersic index under a LogNormal and its magnitude
under a TruncatedNormal.  Two ensembles are timed: the reference's default (chains = 2 P + 2 = 38 for its 18
parameters; 22 is below the host sampler's bound of more than 2 P walkers) and 256 chains.  In a tree whose
library lacks those families, the model falls back to the host sampler, which copies the walkers to and from
the device every half-step.  In one that has them, it takes the device sampler.  Each line says which ran.

  tools/time_prior_fallback.py [--iterations N] [--burn N] [--chains 38,256]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, R + '/tests', R + '/oracle', R + '/tools']
import helpers                                             # noqa: E402
from psfmc_amd import model_galaxy_mcmc, MultiComponentModel      # noqa: E402

# the host galaxy of the example model: index ~ LogNormal (median 2.5), magnitude ~ TruncatedNormal on the
# example's own range [qso_mag, 27.5]
SWAPS = [('       index=WeibullMinimum(c=1.5, scale=4),\n       angle=Uniform(loc=0, scale=180), angle_degrees=True)\n\nblob_xy',
          '       index=LogNormal(0.5, scale=2.5),\n       angle=Uniform(loc=0, scale=180), angle_degrees=True)\n\nblob_xy'),
         ('       mag=Uniform(loc=qso_mag, scale=27.5 - qso_mag),',
          '       mag=TruncatedNormal(qso_mag - 22.0, 27.5 - 22.0, loc=22.0, scale=1.0),'),
         ('import Normal, Uniform, WeibullMinimum', 'import Normal, Uniform, WeibullMinimum, LogNormal, TruncatedNormal')]


def model_file(tmp):
    src = os.path.join(helpers.GOLDEN, 'example')
    for name in os.listdir(src):
        if os.path.isfile(os.path.join(src, name)):
            shutil.copy(os.path.join(src, name), tmp)
    path = os.path.join(tmp, 'model_example.py')
    with open(path) as f:
        text = f.read()
    for old, new in SWAPS:
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    with open(path, 'w') as f:
        f.write(text)
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=400)
    ap.add_argument('--burn', type=int, default=100)
    ap.add_argument('--chains', default='38,256')
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    mf = model_file(tmp)
    for chains in [int(c) for c in a.chains.split(',')]:
        model = MultiComponentModel(mf, max_walkers=1024)
        model.engine
        path = 'host sampler (host-prior fallback)' if model._host_priors else 'device sampler'
        np.random.seed(5)
        model_galaxy_mcmc(model, output_name=os.path.join(tmp, 'warm%d' % chains), iterations=10, burn=10,
                          chains=chains, random_state=11, quiet=True, write_fits=[])
        t0 = time.perf_counter()
        model_galaxy_mcmc(model, output_name=os.path.join(tmp, 'run%d' % chains), iterations=a.iterations,
                          burn=a.burn, chains=chains, random_state=11, quiet=True, write_fits=[])
        dt = time.perf_counter() - t0
        n_it = a.iterations + a.burn
        print('chains %4d  %-36s %d iterations in %.2f s: %8.1f iterations/s (%.3f ms each, database and '
              'statistics included)' % (chains, path, n_it, dt, n_it / dt, dt * 1e3 / n_it), flush=True)
        model.close()
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
