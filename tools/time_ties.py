"""Cost of ties (`Tied(source, ratio, offset)`): log-posterior evaluations per second of a quasar + host model whose host
shares the point source's centre (with a free offset) and fits its axis ratio q -- `Sersic(xy=Tied(centre, offset=...),
reff_b=Tied(size, ratio=...))` -- against its UNTIED TWIN (the same components, an own prior on the host's xy and
reff_b: as many free columns, three, as the tied host's offset and ratio), on the synthetic field of the other timing tools.
  eval     vectors resident on the device (psfmc_eval_theta_device, what bench.py times): 256^2, 4096 walkers
  sampler  the device sampler's run of n iterations (psfmc_stretch_run: 22 walkers take the whole-iteration route,
           where the record derivation is about a fifth of a step): 128^2, 22 walkers; evaluations = walkers x iterations
Order per shape: twin, tied, twin, tied, twin -- the twin's own run-to-run spread beside the ratio.  --untied-only
times the twin alone (three runs): with PSFMC_LIB naming another build of the library, that build's rate for a model
without ties.  One JSON line per shape.
Usage: python tools/time_ties.py [--shapes eval:256:4096 sampler:128:22] [--seconds 1.0] [--untied-only] [--out FILE]"""
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

MODEL = """
centre = Uniform(loc=({c} - 8, {c} - 8), scale=(16, 16))
size = Uniform(loc=2.0, scale={s})
Sky(adu=Normal(loc=0, scale=0.01))
PointSource(xy=centre, mag=Uniform(loc=18.0, scale=2.0))
Sersic(xy={xy}, mag=Uniform(loc=19.0, scale=5.0), reff=size, reff_b={reff_b},
       index=Uniform(loc=0.5, scale=6), angle=Uniform(loc=0, scale=180), angle_degrees=True)
"""
TIED = dict(xy='Tied(centre, offset=Normal(loc=(0, 0), scale=(0.5, 0.5)))', reff_b='Tied(size, ratio=Uniform(loc=0.1, scale=0.8))')
TWIN = dict(xy='Uniform(loc=({c} - 8, {c} - 8), scale=(16, 16))', reff_b='Uniform(loc=0.2, scale={s})')
RANGES = {'adu': (-1e-3, 1e-3), 'angle': (10.0, 170.0), 'index': (0.7, 3.0), 'mag': (19.5, 21.0),
          'reff_b_ratio': (0.3, 0.8), 'xy_offset': (-0.5, 0.5)}


def build(side, directory, max_walkers, tied):
    """The tied model or its twin, and a function drawing n_w vectors inside every support."""
    fld = synth_field.make_field(side, n_sersic=1, seed=0)
    for key, name in (('sci', 'sci.fits'), ('ivm', 'ivm.fits'), ('psf', 'psf.fits'), ('psf_ivm', 'psf_ivm.fits')):
        fits_io.write_image(os.path.join(directory, name), fld[key])
    head = synth_field.model_file_text(side, 0)
    head = head[:head.index('PointSource(')]                       # the Configuration alone
    c, s = side / 2.0 + 0.5, side / 8.0
    terms = {k: v.format(c=c, s=s) for k, v in (TIED if tied else TWIN).items()}
    path = os.path.join(directory, 'model_t%d.py' % tied)
    with open(path, 'w') as f:
        f.write(head + MODEL.format(c=c, s=s, **terms))
    model = MultiComponentModel(path, max_walkers=max_walkers)

    def draw(n_w, seed=3):
        rng = np.random.RandomState(seed)
        cols = []
        for name, width in zip(model.param_names, model.param_lens):
            attr = name.split('_', 2)[2]
            if attr == 'xy':
                cols.append(c + rng.uniform(-3.0, 3.0, (n_w, 2)))
            elif attr == 'reff':
                cols.append(rng.uniform(side / 16.0, side / 8.0, (n_w, 1)))
            elif attr == 'reff_b':
                cols.append(rng.uniform(2.0, side / 16.0, (n_w, 1)))
            elif name.endswith('PointSource_mag'):
                cols.append(rng.uniform(18.5, 19.5, (n_w, 1)))
            else:
                cols.append(rng.uniform(*RANGES[attr], size=(n_w, width)))
        return np.hstack(cols)
    return model, draw


def eval_rate(model, theta, seconds):
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
    return n * len(theta) / dt


def sampler_rate(model, theta, seconds, block=256):
    """psfmc_stretch_run of `block` iterations, repeated: the run returns when the device has finished."""
    from psfmc_amd.sampler import DeviceEnsembleSampler
    n_w = len(theta)
    s = DeviceEnsembleSampler(n_w, model, block=block, live_dangerously=True)
    s.random_state = np.random.RandomState(5).get_state()
    lnp = model.log_posterior_batch(theta)
    assert np.all(np.isfinite(lnp))
    draws, _ = s._draw(block)
    eng = model.engine
    run = lambda: eng.stretch_run(theta.copy(), lnp.copy(), *draws, np.zeros(n_w, dtype=np.int64), store=True)
    run()
    n, t0 = 0, time.perf_counter()
    while True:
        out = run()
        n += block
        dt = time.perf_counter() - t0
        if dt >= seconds:
            break
    assert np.all(np.isfinite(out[1]))
    return n * n_w / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['eval:256:4096', 'sampler:128:22'], help='eval|sampler:side:walkers')
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--untied-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []
    for shape in args.shapes:
        how, side, n_w = shape.split(':')
        side, n_w = int(side), int(n_w)
        order = (0, 0, 0) if args.untied_only else (0, 1, 0, 1, 0)
        rates, params = {0: [], 1: []}, {}
        with tempfile.TemporaryDirectory() as tmp:
            for tied in order:
                model, draw = build(side, tmp, 2 * n_w if how == 'sampler' else n_w, bool(tied))
                rate = (eval_rate if how == 'eval' else sampler_rate)(model, draw(n_w), args.seconds)
                rates[tied].append(round(rate, 1))
                params[tied] = model.num_params
                model.close()
        row = dict(how=how, side=side, walkers=n_w, twin_params=params[0], twin_evals_per_s=rates[0], lib=os.environ.get('PSFMC_LIB', 'in-tree'))
        if rates[1]:
            row.update(tied_evals_per_s=rates[1], tied_params=params[1],
                       ratio_of_medians=round(float(np.median(rates[1]) / np.median(rates[0])), 4),
                       twin_spread=round(float((max(rates[0]) - min(rates[0])) / np.median(rates[0])), 4))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
