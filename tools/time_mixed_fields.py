#!/usr/bin/env python3
"""Log-posterior throughput of a FieldSet whose fields differ in size, against its alternatives (one MI355X):

  mixed     8 fields x 256 walkers in ONE context, image sides 96 ... 128, PSF sides 11 ... 25 (one shared transform)
  own       the same 8 fields, one context per field (each on its own transform), called one after the other
  largest   8 fields x 256 walkers of the largest side (128^2, 25-pixel PSF) in one context

Every field: 1 PointSource + 1 Sersic, raw vectors resident in HBM -> log-posterior, fp64, evals/s.
  tools/time_mixed_fields.py [--out FILE]
  tools/time_mixed_fields.py --single 170 [--walkers 2048]   one embedded one-field context (A/B runs of the
                                                              library with PSFMC_LIB)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
import numpy as np                                    # noqa: E402
import torch                                          # noqa: E402

import synth_field                                    # noqa: E402
from bench import timed_calls                         # noqa: E402

SIDES = [96, 128, 100, 120, 112, 128, 104, 96]
PSF_SIDES = [11, 25, 13, 21, 17, 15, 23, 19]
N_W = 256


def make_model(ny, nx, pk, seed, max_walkers):
    """A synthetic field of ny x nx with a pk-pixel Moffat PSF; returns (model, near-truth walkers)."""
    from psfmc_amd import MultiComponentModel
    from psfmc_amd.ModelComponents import Configuration, PointSource, Sersic
    from psfmc_amd.distributions import Uniform, WeibullMinimum
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
    c = np.array((nx / 2 + 0.5, ny / 2 + 0.5))
    img = 40.0 * np.exp(-((xx - c[0]) ** 2 + (yy - c[1]) ** 2) / 18.0)
    sci = (img + rng.normal(size=(ny, nx)) * 0.05).astype(np.float32)
    ivm = np.full((ny, nx), 400.0, dtype=np.float32)
    psf = (synth_field.moffat_psf(pk, fwhm=2.5) * 1000.0).astype(np.float32)
    pivm = (1.0 / (1e-4 + np.abs(psf) / 50.0)).astype(np.float32)
    comps = [Configuration(sci, ivm, psf, pivm, mag_zeropoint=25.0),
             PointSource(xy=Uniform(loc=c - 4, scale=8 * np.ones(2)), mag=Uniform(loc=18.0, scale=2.0)),
             Sersic(xy=Uniform(loc=c - 4, scale=8 * np.ones(2)), mag=Uniform(loc=19.0, scale=3.0),
                    reff=Uniform(loc=2.0, scale=6.0), reff_b=Uniform(loc=2.0, scale=6.0),
                    index=WeibullMinimum(c=1.5, scale=4), angle=Uniform(loc=0, scale=180), angle_degrees=True)]
    model = MultiComponentModel(comps, backend='fused', max_walkers=max_walkers)
    truth = np.array([19.0, c[0] + 0.3, c[1] - 0.6, 35.0, 2.0, 20.5, 5.0, 3.0, c[0] - 1.2, c[1] + 0.8])
    theta = truth + rng.normal(size=(max_walkers, len(truth))) * 1e-2
    return model, theta


def time_set(specs, dev, sync):
    from psfmc_amd import FieldSet
    probs = [make_model(ny, nx, pk, 100 + f, N_W) for f, (ny, nx, pk) in enumerate(specs)]
    fs = FieldSet([m for m, _ in probs], max_walkers=len(specs) * N_W)
    th = torch.from_numpy(np.concatenate([t for _, t in probs])).to(dev)
    out = torch.empty(len(specs) * N_W, dtype=torch.float64, device=dev)
    seg_f, seg_n = list(range(len(specs))), [N_W] * len(specs)
    call = lambda: fs.context.logpost_theta_device(seg_f, seg_n, th.data_ptr(), out.data_ptr(), None)
    per_call, n = timed_calls(call, sync)
    got = out.cpu().numpy()
    want = np.concatenate([m.log_posterior_batch(t[:4]) for m, t in probs])
    rel = float(np.max(np.abs(got.reshape(len(specs), N_W)[:, :4].ravel() - want) / np.abs(want)))
    rec = {'value': len(specs) * N_W / per_call, 'unit': 'evals/s', 'calls': n, 'timed_s': per_call * n,
           'transform': [int(fs.context.get_option('transform_ny')), int(fs.context.get_option('transform_nx'))],
           'finite': int(np.isfinite(got).sum()), 'max_rel_vs_own_context': rel}
    fs.close()
    for m, _ in probs:
        m.close()
    return rec


def time_own(specs, dev, sync):
    probs = [make_model(ny, nx, pk, 100 + f, N_W) for f, (ny, nx, pk) in enumerate(specs)]
    ths = [torch.from_numpy(t).to(dev) for _, t in probs]
    out = torch.empty(N_W, dtype=torch.float64, device=dev)

    def call():
        for (m, _), th in zip(probs, ths):
            m.engine.logpost_theta_device(N_W, th.data_ptr(), 0, out.data_ptr(), None)
    per_call, n = timed_calls(call, sync)
    rec = {'value': len(specs) * N_W / per_call, 'unit': 'evals/s', 'calls': n, 'timed_s': per_call * n,
           'transforms': [[int(m.engine.get_option('transform_ny')), int(m.engine.get_option('transform_nx'))]
                          for m, _ in probs]}
    for m, _ in probs:
        m.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--single', type=int, default=0)
    ap.add_argument('--walkers', type=int, default=2048)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    sync = lambda: torch.cuda.synchronize(dev)
    if args.single:
        m, theta = make_model(args.single, args.single, 25, 7, args.walkers)
        th = torch.from_numpy(theta).to(dev)
        out = torch.empty(args.walkers, dtype=torch.float64, device=dev)
        call = lambda: m.engine.logpost_theta_device(args.walkers, th.data_ptr(), 0, out.data_ptr(), None)
        per_call, n = timed_calls(call, sync)
        print(json.dumps({'lib': os.environ.get('PSFMC_LIB', 'default'), 'side': args.single,
                          'transform': [int(m.engine.get_option('transform_ny')),
                                        int(m.engine.get_option('transform_nx'))],
                          'walkers': args.walkers, 'evals_per_s': args.walkers / per_call, 'calls': n}))
        m.close()
        return
    mixed = list(zip(SIDES, SIDES, PSF_SIDES))
    res = {'workload': '8 fields x 256 walkers, image sides %s, PSF sides %s, 1 PointSource + 1 Sersic, '
                       'raw vectors resident in HBM -> log-posterior, fp64' % (SIDES, PSF_SIDES),
           'device': torch.cuda.get_device_name(dev)}
    res['mixed_fieldset'] = time_set(mixed, dev, sync)
    res['one_context_per_field'] = time_own(mixed, dev, sync)
    big = max(SIDES)
    res['same_shape_fieldset_largest'] = time_set([(big, big, max(PSF_SIDES))] * len(SIDES), dev, sync)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
