"""Cost of the general components (`Sersic(..., boxiness=...)`, `Sky(..., slope=...)`): log-posterior evaluations per
second of the same synthetic field (Sky + PS + 1 Sersic) with one general Sersic and a tilted sky and without the
keywords, vectors resident on the device (psfmc_eval_theta_device, what bench.py times), at 256^2 with 4096 walkers
(the headline shape) and at 128^2 with 22 walkers.  One JSON line per configuration, a table at the end.
--fourier: the cost of the azimuthal modes instead -- Sky + PS + one Sersic with a free boxiness and two free modes
(`fourier={1: ..., 3: ...}`) against the same model with the boxiness only.
--spiral: the cost of the spiral arms -- the same model with a free boxiness and a free spiral (all six values)
against the boxiness only.
--radial: the cost of the radial laws -- Sky + PS + one boxy `Ferrer` and one `Moffat` against the same model with two
boxy `Sersic`s.
--mean: the cost of the pixel-averaged mode -- the `--radial` model with `pixel_mean=True` on both components against
the same model without it.
--truncation: the cost of a truncated component -- the `--radial` model with an inner and an outer truncation on the
Ferrer and an outer one on the Moffat (all six radii free) against the same model untruncated.
--bending: the cost of bending modes -- the `--radial` model with modes 2 and 3 on the Ferrer and mode 2 on the Moffat
(all three amplitudes free) against the same model without bending.
Usage: python tools/time_general.py [--fourier | --spiral | --radial | --mean | --truncation | --bending] [--shapes 256:4096 128:22] [--seconds 1.0] [--out FILE]"""
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


SKY = ('Sky(adu=Normal(loc=0, scale=0.01))', 'Sky(adu=Normal(loc=0, scale=0.01), slope=Normal(loc=(0, 0), scale=(1e-4, 1e-4)))')


def build(side, directory, max_walkers, general):
    fld = synth_field.make_field(side, n_sersic=1, seed=0)
    for key, name in (('sci', 'sci.fits'), ('ivm', 'ivm.fits'), ('psf', 'psf.fits'), ('psf_ivm', 'psf_ivm.fits')):
        fits_io.write_image(os.path.join(directory, name), fld[key])
    text = synth_field.model_file_text(side, 1)
    text = text.replace('PointSource(', SKY[general] + '\nPointSource(', 1)
    if general:
        text = text.replace('angle_degrees=True)', 'angle_degrees=True, boxiness=Uniform(loc=-1, scale=2))')
    path = os.path.join(directory, 'model_%d.py' % general)
    with open(path, 'w') as f:
        f.write(text)
    return MultiComponentModel(path, max_walkers=max_walkers), fld


FOURIER = (', fourier={1: (Uniform(loc=-0.4, scale=0.8), Uniform(loc=-180, scale=360)), '
           '3: (Uniform(loc=-0.4, scale=0.8), Uniform(loc=-180, scale=360))}')


SPIRAL = (", spiral={'r_in': Uniform(loc=0, scale=4), 'r_out': Uniform(loc=5, scale=15), "
          "'winding': Uniform(loc=-400, scale=800), 'alpha': Uniform(loc=0, scale=1), "
          "'inclination': Uniform(loc=0, scale=70), 'sky_angle': Uniform(loc=-90, scale=180)}")


def build_fourier(side, directory, max_walkers, modes, extra=FOURIER):
    """Sky + PS + one Sersic with a free boxiness, and with `modes` the `extra` keyword (two free Fourier modes, or
    the free spiral) beside it."""
    fld = synth_field.make_field(side, n_sersic=1, seed=0)
    for key, name in (('sci', 'sci.fits'), ('ivm', 'ivm.fits'), ('psf', 'psf.fits'), ('psf_ivm', 'psf_ivm.fits')):
        fits_io.write_image(os.path.join(directory, name), fld[key])
    text = synth_field.model_file_text(side, 1).replace('PointSource(', SKY[0] + '\nPointSource(', 1)
    text = text.replace('angle_degrees=True)', 'angle_degrees=True, boxiness=Uniform(loc=-1, scale=2)%s)'
                        % (extra if modes else ''))
    path = os.path.join(directory, 'model_f%d.py' % modes)
    with open(path, 'w') as f:
        f.write(text)
    return MultiComponentModel(path, max_walkers=max_walkers), fld


RADIAL_COMMON = ('xy=Uniform(loc=c - ms, scale=2 * ms), mag=Uniform(loc=19.0, scale=5.0), '
                 'angle=Uniform(loc=0, scale=180), angle_degrees=True')
# the free values the timed vectors draw, by the parameter's attribute: (low, high) in units of the side where scaled
RADIAL_RANGES = {'adu': (-1e-3, 1e-3), 'alpha': (0.5, 3.0), 'angle': (10.0, 170.0), 'beta': (1.2, 1.9),
                 'boxiness': (-0.5, 0.5), 'index': (0.7, 3.0), 'mag': (19.5, 21.0)}


TRUNC_RANGE = {'trunc_in_lo': (0.0, 0.01), 'trunc_in_hi': (0.02, 0.04), 'trunc_out_lo': (0.06, 0.08),
               'trunc_out_hi': (0.10, 0.12)}                            # in units of the side


def build_radial(side, directory, max_walkers, laws, mean=False, trunc=False, bend=False):
    """Sky + PS + a boxy Ferrer and a Moffat (`laws`; with `mean` both have `pixel_mean=True`, with `trunc` the
    Ferrer both truncations and the Moffat an outer one, every radius free, with `bend` the Ferrer bending modes 2 and 3
    and the Moffat mode 2, every amplitude free), or two boxy Sersics with the same radii;
    the model and a function drawing n_w vectors inside every support."""
    fld = synth_field.make_field(side, n_sersic=1, seed=0)
    for key, name in (('sci', 'sci.fits'), ('ivm', 'ivm.fits'), ('psf', 'psf.fits'), ('psf_ivm', 'psf_ivm.fits')):
        fits_io.write_image(os.path.join(directory, name), fld[key])
    text = synth_field.model_file_text(side, 0).replace('PointSource(', SKY[0] + '\nPointSource(', 1)
    big, small = 'Uniform(loc=%r, scale=%r)' % (side / 16.0 + 2.0, side / 8.0), 'Uniform(loc=2.0, scale=%r)' % (side / 16.0)
    box = 'boxiness=Uniform(loc=-1, scale=2)'
    if mean:
        box += ', pixel_mean=True'
    radius = 'Uniform(loc=0.0, scale=%r)' % float(side)
    cut = lambda sides: (", truncation={%s}" % ', '.join("'%s': (%s, %s)" % (k, radius, radius) for k in sides)
                         if trunc else '')
    amp = 'Uniform(loc=-1.0, scale=2.0)'
    cut_bend = lambda sides, modes: cut(sides) + (
        ', bending={%s}' % ', '.join('%d: %s' % (m, amp) for m in modes) if bend else '')
    if laws:
        text += 'Ferrer(%s, r_out=%s, r_out_b=%s, alpha=Uniform(loc=0, scale=4), beta=Uniform(loc=-2, scale=3.95), %s%s)\n' % (
            RADIAL_COMMON, big, small, box, cut_bend(('inner', 'outer'), (2, 3)))
        text += 'Moffat(%s, fwhm=%s, fwhm_b=%s, beta=Uniform(loc=1.05, scale=8)%s%s)\n' % (
            RADIAL_COMMON, big, small, ', pixel_mean=True' if mean else '', cut_bend(('outer',), (2,)))
    else:
        for _ in range(2):
            text += 'Sersic(%s, reff=%s, reff_b=%s, index=Uniform(loc=0.5, scale=6), %s)\n' % (RADIAL_COMMON, big, small, box)
    path = os.path.join(directory, 'model_r%d%d%d%d.py' % (laws, mean, trunc, bend))
    with open(path, 'w') as f:
        f.write(text)
    model = MultiComponentModel(path, max_walkers=max_walkers)

    def draw(n_w, seed=3):
        rng = np.random.RandomState(seed)
        cols = []
        for name, width in zip(model.param_names, model.param_lens):
            attr = name.split('_', 2)[2]
            if attr == 'xy':
                cols.append(side / 2.0 + 0.5 + rng.uniform(-4.0, 4.0, (n_w, 2)))
            elif attr in ('r_out', 'fwhm', 'reff'):
                cols.append(rng.uniform(side / 16.0 + 2.0, side / 8.0, (n_w, 1)))
            elif attr in ('r_out_b', 'fwhm_b', 'reff_b'):
                cols.append(rng.uniform(2.0, side / 16.0, (n_w, 1)))
            elif attr in TRUNC_RANGE:
                cols.append(side * rng.uniform(*TRUNC_RANGE[attr], size=(n_w, 1)))
            elif attr.startswith('bend'):
                cols.append(rng.uniform(-0.4, 0.4, (n_w, 1)))
            elif name.endswith('PointSource_mag'):
                cols.append(rng.uniform(18.5, 19.5, (n_w, 1)))
            else:
                cols.append(rng.uniform(*RADIAL_RANGES[attr], size=(n_w, width)))
        return np.hstack(cols)
    return model, draw


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
    ap.add_argument('--fourier', action='store_true', help='boxiness + two free modes against boxiness only')
    ap.add_argument('--spiral', action='store_true', help='boxiness + a free spiral against boxiness only')
    ap.add_argument('--radial', action='store_true', help='a boxy Ferrer and a Moffat against two boxy Sersics')
    ap.add_argument('--mean', action='store_true', help='the --radial model with pixel_mean=True against the same without')
    ap.add_argument('--truncation', action='store_true',
                    help='the --radial model with truncated components against the same untruncated')
    ap.add_argument('--bending', action='store_true',
                    help='the --radial model with bending modes against the same without')
    args = ap.parse_args()
    if args.fourier + args.spiral + args.radial + args.mean + args.truncation + args.bending > 1:
        ap.error('--fourier, --spiral, --radial, --mean, --truncation and --bending exclude each other')
    rows = []
    for shape in args.shapes:
        side, n_w = (int(v) for v in shape.split(':'))
        with tempfile.TemporaryDirectory() as tmp:
            rates = {}
            for general in (0, 1, 0, 1):                  # alternating, the better of two runs each
                if args.radial or args.mean or args.truncation or args.bending:
                    model, draw = (build_radial(side, tmp, n_w, 1, mean=bool(general)) if args.mean else
                                   build_radial(side, tmp, n_w, 1, trunc=bool(general)) if args.truncation else
                                   build_radial(side, tmp, n_w, 1, bend=bool(general)) if args.bending else
                                   build_radial(side, tmp, n_w, general))
                    rate, _ = evals_per_second(model, draw(n_w), args.seconds)
                    rates[general] = max(rates.get(general, 0.0), rate)
                    model.close()
                    continue
                if args.spiral:
                    model, fld = build_fourier(side, tmp, n_w, general, SPIRAL)
                else:
                    model, fld = (build_fourier if args.fourier else build)(side, tmp, n_w, general)
                theta = synth_field.draw_walkers(side, 1, n_w, seed=2, near_truth=fld['truth'])
                rng = np.random.RandomState(3)
                theta = np.hstack([rng.normal(size=(n_w, 1)) * 1e-3, theta])            # the sky level
                if args.spiral:                # the boxiness; alpha, incl, r_in, r_out, sky, wind behind reff_b
                    theta = np.insert(theta, [5], rng.uniform(-0.5, 0.5, (n_w, 1)), axis=1)
                    if general:
                        theta = np.insert(theta, [10] * 6, np.c_[rng.uniform(0.1, 0.9, n_w), rng.uniform(5, 60, n_w),
                                                                 rng.uniform(0.5, 3.5, n_w), rng.uniform(6, 19, n_w),
                                                                 rng.uniform(-80, 80, n_w), rng.uniform(-350, 350, n_w)],
                                          axis=1)
                elif args.fourier:                                 # the boxiness, then (a_1, phi_1, a_3, phi_3)
                    theta = np.insert(theta, [5], rng.uniform(-0.5, 0.5, (n_w, 1)), axis=1)
                    if general:
                        theta = np.insert(theta, [6, 6, 6, 6], np.c_[rng.uniform(-0.3, 0.3, n_w), rng.uniform(-180, 180, n_w),
                                                                     rng.uniform(-0.3, 0.3, n_w), rng.uniform(-180, 180, n_w)],
                                          axis=1)
                elif general:                                                          # the slope, the boxiness
                    theta = np.insert(theta, [1, 1, 5], np.c_[rng.normal(size=(n_w, 2)) * 1e-5,
                                                              rng.uniform(-0.5, 0.5, n_w)], axis=1)
                rate, _ = evals_per_second(model, theta, args.seconds)
                rates[general] = max(rates.get(general, 0.0), rate)
                model.close()
            row = dict(side=side, walkers=n_w, default_evals_per_s=round(rates[0], 1),
                       general_evals_per_s=round(rates[1], 1), ratio=round(rates[1] / rates[0], 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
    lines = ['side     W    unbent evals/s       bent evals/s  ratio' if args.bending else
             'side     W untruncated evals/s  truncated evals/s  ratio' if args.truncation else
             'side     W   centres evals/s  pixel means evals/s  ratio' if args.mean else
             'side     W 2 Sersics evals/s Ferrer + Moffat evals/s ratio' if args.radial else
             'side     W  boxiness evals/s box + spiral evals/s  ratio' if args.spiral else
             'side     W   default evals/s     general evals/s  ratio' if not args.fourier else
             'side     W  boxiness evals/s  box + modes evals/s  ratio']
    for r in rows:
        lines.append('%4d %5d %16.0f %19.0f %6.3f' % (r['side'], r['walkers'], r['default_evals_per_s'],
                                                     r['general_evals_per_s'], r['ratio']))
    print('\n'.join(lines))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
