"""Cost of the pixel-integrated Sersic profile (`Sersic(..., integrate=True)`): log-posterior evaluations per second
of the same synthetic field (PS + 1 Sersic) with the keyword and without it, vectors resident on the device
(psfmc_eval_theta_device, what bench.py times), at 256^2 with 4096 walkers (the headline shape) and at 128^2 with 22
walkers.  One JSON line per configuration, a table at the end.
Usage: python tools/time_integrated.py [--shapes 256:4096 128:22] [--seconds 1.0] [--out FILE]"""
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


def build(side, directory, max_walkers, integrate):
    fld = synth_field.make_field(side, n_sersic=1, seed=0)
    for key, name in (('sci', 'sci.fits'), ('ivm', 'ivm.fits'), ('psf', 'psf.fits'), ('psf_ivm', 'psf_ivm.fits')):
        fits_io.write_image(os.path.join(directory, name), fld[key])
    text = synth_field.model_file_text(side, 1)
    if integrate:
        text = text.replace('angle_degrees=True)', 'angle_degrees=True, integrate=True)')
    path = os.path.join(directory, 'model_%d.py' % integrate)
    with open(path, 'w') as f:
        f.write(text)
    return MultiComponentModel(path, max_walkers=max_walkers), fld


def evals_per_second(model, theta, seconds):
    import torch
    eng = model.engine
    d_theta = torch.as_tensor(theta, dtype=torch.float64, device='cuda').contiguous()
    d_out = torch.empty(len(theta), dtype=torch.float64, device='cuda')
    call = lambda: eng.logpost_theta_device(len(theta), d_theta.data_ptr(), 0, d_out.data_ptr())
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        n += 20
        dt = time.perf_counter() - t0
        if dt >= seconds:
            break
    assert torch.isfinite(d_out).all()
    return n * len(theta) / dt, d_out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['256:4096', '128:22'], help='side:walkers')
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rows = []
    for shape in args.shapes:
        side, n_w = (int(v) for v in shape.split(':'))
        with tempfile.TemporaryDirectory() as tmp:
            rates = {}
            for integrate in (0, 1, 0, 1):                  # alternating, the better of two runs each
                model, fld = build(side, tmp, n_w, integrate)
                theta = synth_field.draw_walkers(side, 1, n_w, seed=2, near_truth=fld['truth'])
                rate, _ = evals_per_second(model, theta, args.seconds)
                rates[integrate] = max(rates.get(integrate, 0.0), rate)
                model.close()
            row = dict(side=side, walkers=n_w, default_evals_per_s=round(rates[0], 1),
                       integrated_evals_per_s=round(rates[1], 1), ratio=round(rates[1] / rates[0], 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
    lines = ['side     W   default evals/s  integrated evals/s  ratio']
    for r in rows:
        lines.append('%4d %5d %16.0f %19.0f %6.3f' % (r['side'], r['walkers'], r['default_evals_per_s'],
                                                     r['integrated_evals_per_s'], r['ratio']))
    print('\n'.join(lines))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
