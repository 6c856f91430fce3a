"""The general components (boxiness, Fourier modes, spiral arms, the Moffat and Ferrer laws, truncation, bending) at
the extremes a `Uniform` prior can reach: the extreme list, the models and walkers that carry it, and a LONG-DOUBLE
evaluation of one general component per pixel -- what tests/test_gpu_general_extremes.py holds the device to, and what
tests/test_general_extremes_reference.py pins without a GPU.  The sibling of the raster-extremes part of
tests/helpers.py (`extreme_specs`, `longdouble_sersic`, `extreme_references`), for `general_pixel` (psfmc_general.h)
and its pixel-mean twin (psfmc_general_mean.h).

The long-double text below is written from the formulas in the header of csrc/psfmc_general.h and DESIGN.md
sections 15-18, 26 and 32; it calls none of the product's image functions.  As in `helpers.longdouble_sersic` the
PER-WALKER SCALARS are the fp64 values the host definition computes -- the derived row (kappa, 1/(2n), Sigma_e, the
ellipse matrix), A(c), Q, cos / sin of the sky angle and of the inclination, the winding in radians, cos / sin of
m phi_m, Sigma_0 and g of the laws, r_a / r_b, e = c + 2 and 2 / e, and the two constants of every ramp (its argument is
k1 rho + k0 with k1 = 4 r_major / (hi - lo), k0 = -2 (lo + hi) / (hi - lo); r_major = 1 for the spiral's, whose radius is
in pixels) -- and every per-pixel operation is in numpy
`longdouble`: the per-pixel error of the fp64 kernels is what is measured.  The tanh ramps are 1 / (1 + exp(-+2a)):
the same function without the cancellation of (1 -+ tanh a) / 2, which loses every digit for a >~ 20."""
import numpy as np

import fuzz_shapes
import helpers
import psfmc_oracle as orc
import test_gpu_general_components as tgg
from extra_contract import EDGE_MARGIN
from helpers import RASTER_FLOOR, RASTER_ORACLE_FACTOR
from psfmc_amd import MultiComponentModel
from psfmc_amd.ModelComponents import Configuration, Ferrer, Moffat, PointSource, Sersic, Sky
from psfmc_amd.distributions import Normal, Uniform
from test_gpu_general_components import RAW_BOUND

SHAPE, EMBEDDED = (64, 64), (70, 66)
E_DEF_CAP = 1e-9                 # at most one extreme in ten may have the fp64 definition farther than this from exact
CLASSES = {'Sersic': Sersic, 'Moffat': Moffat, 'Ferrer': Ferrer}
LEVELS = ('plain', 'fou', 'spi', 'fou+spi', 'rad', 'tru', 'bnd')       # GenLevel of psfmc_hip.hip, in its order
# family: (component class, keywords beside the boxiness, the lowest level whose kernels have its block)
FAMILIES = {'box': ('Sersic', (), 'plain'), 'fou': ('Sersic', ('fourier',), 'fou'), 'spi': ('Sersic', ('spiral',), 'spi'),
            'mof': ('Moffat', (), 'rad'), 'fer': ('Ferrer', (), 'rad'), 'tru': ('Sersic', ('truncation',), 'tru'),
            'bnd': ('Sersic', ('bending',), 'bnd')}
# what a dark third component carries to LIFT a context to a level above its family's own
LIFTS = {'fou+spi': {'fou': 'spiral', 'spi': 'fourier'}, 'tru': 'truncation', 'bnd': 'bending'}


# ---------------------------------------------------------------------------------------------------------------
# the long-double evaluation
# ---------------------------------------------------------------------------------------------------------------
def component_args(comp, mag_zp):
    """(law, row, pars, boxiness, modes, spiral, truncation, bending) of a component at its current values: the
    arguments of the definition's functions (`Sersic.bent_image`) and of `longdouble_general`."""
    get = lambda k: getattr(comp, k)
    a, ph = comp._fourier_values(get) if comp.has_fourier else ((), ())
    return (comp.radial_law, comp.derived_row(mag_zp), comp._radial_values(get) if comp.radial_law else None,
            float(np.ravel(comp.boxiness)[0]) if comp.has_boxiness else 0.0,
            [(int(m), float(x), float(y)) for m, x, y in zip(comp.fourier_modes, a, ph)],
            comp._spiral_values(get) if comp.has_spiral else None, comp.truncation_tuple(), comp.bending_list())


def walker_scalars(law, row, pars, boxiness, modes, spiral):
    """The fp64 per-walker scalars that are not in the row: (area = A(c) Q, central brightness -- Sigma_e / (A Q
    cos(incl)) of the Sersic law in the definition's order of operations, Sigma_0 of the others)."""
    area = Sersic.superellipse_area_ratio(boxiness)
    if modes:
        area = area * Sersic.fourier_area_ratio(boxiness, modes)
    if law is not None:
        return area, Sersic.radial_central(law, row, pars, boxiness, modes, spiral)
    sb = row[8] / area
    return area, (sb / np.cos(float(spiral[4])) if spiral is not None else sb)


def general_value(ns, law, row, pars, boxiness, modes, spiral, truncation, bending, x, y):
    """(value, Ferrer's x or None) of one general component at pixel coordinates (x, y), in the arithmetic of `ns`: a
    namespace with `num` (a conversion from fp64), `where`, `fabs`, `hypot`, `sqrt`, `exp`, `expm1`, `log`, `cos`,
    `sin`, `power` -- numpy longdouble on arrays (`longdouble_general`) or mpmath at 50 digits on one pixel."""
    num = ns.num
    x0, y0, m00, m01, m10, m11, kappa, p, _ = [num(float(v)) for v in row]
    e64 = float(boxiness) + 2.0
    e, two_e = num(e64), num(2.0 / e64)
    _, central = walker_scalars(law, row, pars, boxiness, modes, spiral)
    central = num(float(central))
    dx, dy = x - x0, y - y0
    X, Y = dx, dy
    if spiral is not None:
        r_in, r_out, wind, alpha, incl, sky = [float(s) for s in spiral]
        cs, sn, ci = num(float(np.cos(sky))), num(float(np.sin(sky))), num(float(np.cos(incl)))
        X = cs * dx + sn * dy
        Y = (-sn * dx + cs * dy) / ci
        r = ns.hypot(X, Y)
        # (the ramp's argument k1 r + k0 from its two fp64 constants, as the kernels' per-walker records hold them)
        a = num(4.0 / (r_out - r_in)) * r + num(-2.0 * (r_in + r_out) / (r_out - r_in))
        T = 1 / (1 + ns.exp(-2 * a))
        P = ns.where(r > 0, ns.power(ns.where(r > 0, r, 1) / num(r_out), num(alpha)), 1.0 if alpha == 0 else 0.0)
        t = num(wind) * T * P
        ct, st = ns.cos(t), ns.sin(t)
        X, Y = ct * X + st * Y, -st * X + ct * Y
    u = m00 * X + m01 * Y
    v = m10 * X + m11 * Y
    if bending:
        ratio = num(float((1.0 / np.hypot(row[2], row[3])) / (1.0 / np.hypot(row[4], row[5]))))
        f, um = 0 * u, u
        todo = {int(m): float(a) for m, a in bending}
        for m in range(1, max(todo) + 1):
            if m > 1:
                um = um * u
            if m in todo:
                f = f + num(todo[m]) * um
        v = v + ratio * f
    centre = (u == 0) & (v == 0)
    rho2 = ns.power(ns.power(ns.fabs(u), e) + ns.power(ns.fabs(v), e), two_e)
    if modes:
        ruv = ns.hypot(u, v)
        c1, s1 = u / ruv, v / ruv
        cm, sm, eps = c1, s1, 0 * u
        todo = {int(m): (float(a), float(phi)) for m, a, phi in modes}
        for m in range(1, max(todo) + 1):
            if m > 1:
                cm, sm = cm * c1 - sm * s1, sm * c1 + cm * s1
            if m in todo:
                a, phi = todo[m]
                eps = eps + num(a) * (cm * num(float(np.cos(m * phi))) - sm * num(float(np.sin(m * phi))))
        rho2 = rho2 * (1 + eps) ** 2
    xk = None
    if law is None:
        q = rho2 / (dx * dx + dy * dy)
        L = ns.log(rho2)
        g = -2 * kappa * p * ns.exp(L * (p - num(0.5)))
        val = central * ns.exp(-kappa * ns.expm1(L * p)) * (1 + g * (q / 12 * g))
    elif law == 'moffat':
        beta = float(pars[0])
        gm = num(float(4.0 * np.expm1(np.log(2.0) / beta)))
        val = ns.where(centre, central, central * ns.power(1 + gm * rho2, num(-beta)))
    else:
        alpha, k = float(pars[0]), 2.0 - float(pars[1])
        xk = ns.where(centre, 0.0, ns.power(rho2, num(0.5 * k)))
        inside = xk < 1
        val = ns.where(inside, central * ns.power(ns.where(inside, 1 - xk, 1), num(alpha)), 0.0)
    if truncation is not None:
        r_major = float(1.0 / np.hypot(row[2], row[3]))
        rho = ns.sqrt(ns.where(centre, 0.0, rho2))
        for side, sign in ((0, -2), (1, 2)):
            lo, hi = truncation[2 * side], truncation[2 * side + 1]
            if lo is not None:
                # (a = 2 (2 s - lo - hi) / (hi - lo) with s = r_major rho, from its two fp64 constants)
                span = float(hi) - float(lo)
                a = num(4.0 * r_major / span) * rho + num(-2.0 * (float(lo) + float(hi)) / span)
                val = val * (1 / (1 + ns.exp(sign * a)))
    return val, xk


class _LongDouble(object):
    num = staticmethod(np.longdouble)
    where, fabs, hypot, sqrt = staticmethod(np.where), staticmethod(np.abs), staticmethod(np.hypot), staticmethod(np.sqrt)
    exp, expm1, log, cos, sin = (staticmethod(np.exp), staticmethod(np.expm1), staticmethod(np.log), staticmethod(np.cos),
                                 staticmethod(np.sin))
    power = staticmethod(np.power)


def longdouble_general(law, row, pars, boxiness, modes, spiral, truncation, bending, shape):
    """(image, Ferrer's x or None) of one general component on a `shape` image, every per-pixel operation in numpy
    `longdouble` (x87: 64-bit significand) -- `Sersic.bent_image` written out from the formulas, the ramps as
    1 / (1 + exp(-+2a))."""
    assert np.finfo(np.longdouble).nmant >= 63, 'numpy longdouble is not the 80-bit type here'
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.longdouble)
    with np.errstate(all='ignore'):
        return general_value(_LongDouble, law, row, pars, boxiness, modes, spiral, truncation, bending, xx, yy)


def mpmath_general(law, row, pars, boxiness, modes, spiral, truncation, bending, x, y, digits=50):
    """The same formulas at one pixel with mpmath at `digits` digits (the fp64 per-walker scalars as they are)."""
    import mpmath as mp

    class ns(object):
        num = staticmethod(lambda v: mp.mpf(float(v)))
        where = staticmethod(lambda c, a, b: a if c else b)
        fabs, hypot, sqrt, exp, expm1, log, cos, sin = (staticmethod(abs), staticmethod(mp.hypot), staticmethod(mp.sqrt),
                                                        staticmethod(mp.exp), staticmethod(mp.expm1),
                                                        staticmethod(lambda v: mp.log(v) if v != 0 else mp.mpf('-inf')),
                                                        staticmethod(mp.cos), staticmethod(mp.sin))
        power = staticmethod(lambda a, b: mp.power(a, b) if a != 0 else (mp.mpf(1) if b == 0 else mp.mpf(0)))
    with mp.workdps(digits):
        val, _ = general_value(ns, law, row, pars, boxiness, modes, spiral, truncation, bending, mp.mpf(int(x)), mp.mpf(int(y)))
        return mp.mpf(val)


# ---------------------------------------------------------------------------------------------------------------
# the extreme list
# ---------------------------------------------------------------------------------------------------------------
def slot_centres(ny, nx):
    return [(nx * 0.34 + 0.3, ny * 0.4 + 0.4), (nx * 0.66 - 0.4, ny * 0.6 - 0.2)]


def _keyword_values(keys, role):
    """The keywords' values of a slot: role 'extreme' (the base the overrides are applied to: every keyword present
    and neutral or soft, so that an override is the only extreme), 'ordinary' (the neighbour) or 'dark'."""
    out = {}
    if 'fourier' in keys:
        out.update({'f%d_%s' % (m, k): 0.0 for m in Sersic.FOURIER_MODES for k in ('amp', 'phase')})
        if role == 'ordinary':
            out.update(f2_amp=0.15, f2_phase=30.0, f3_amp=-0.1, f3_phase=25.0)
    if 'spiral' in keys:
        out.update(spiral_r_in=2.0, spiral_r_out=9.0, spiral_wind=150.0, spiral_alpha=0.0, spiral_incl=35.0,
                   spiral_sky=20.0)
    if 'truncation' in keys:
        # (the base: an inner ramp inside the first half pixel and an outer one near the image's far side)
        out.update(dict(trunc_in_lo=1.0, trunc_in_hi=3.0, trunc_out_lo=12.0, trunc_out_hi=18.0) if role == 'ordinary' else
                   dict(trunc_in_lo=0.25, trunc_in_hi=0.5, trunc_out_lo=40.0, trunc_out_hi=60.0))
    if 'bending' in keys:
        out.update({'bend%d' % m: 0.0 for m in Sersic.BEND_MODES})
        if role == 'ordinary':
            out.update(bend2=0.2)
    return out


def slot_values(family, role, slot, ny, nx):
    """{attribute: value} of one of the two general slots of a family's model."""
    cls, keys, _ = FAMILIES[family]
    if role == 'dark':                   # every pixel exactly zero on the device and in fp64, five sides to the left
        xy = (-5.0 * nx + 0.3, ny * 0.5 + 0.3)
        vals = {'Sersic': dict(angle=10.0, index=0.1, mag=20.0, reff=3.0, reff_b=2.0),
                'Moffat': dict(angle=10.0, beta=500.0, mag=20.0, fwhm=0.5, fwhm_b=0.5),
                'Ferrer': dict(angle=10.0, alpha=1.0, beta=0.0, mag=20.0, r_out=1.0, r_out_b=1.0)}[cls]
        vals.update(xy=xy, boxiness=0.0)
    else:
        vals = {'Sersic': [dict(angle=30.0, index=1.5, mag=19.0, reff=6.0, reff_b=4.0, boxiness=0.5),
                           dict(angle=110.0, index=2.5, mag=18.5, reff=7.0, reff_b=3.5, boxiness=-0.4)],
                'Moffat': [dict(angle=30.0, beta=2.5, mag=19.0, fwhm=6.0, fwhm_b=4.0, boxiness=0.5),
                           dict(angle=110.0, beta=1.8, mag=18.5, fwhm=8.0, fwhm_b=5.0, boxiness=-0.4)],
                'Ferrer': [dict(angle=30.0, alpha=2.0, beta=0.0, mag=18.0, r_out=22.0, r_out_b=14.0, boxiness=0.5),
                           dict(angle=110.0, alpha=0.5, beta=1.5, mag=18.3, r_out=23.0, r_out_b=15.0, boxiness=-0.4)]
                }[cls][slot]
        vals.update(xy=slot_centres(ny, nx)[slot])
    vals.update(_keyword_values(keys, 'extreme' if role == 'dark' else role))
    return vals


def general_extreme_specs(ny, nx):
    """(name, family, overrides of the slot's values, flags) of every extreme, in the style of
    `helpers.extreme_specs`.  Flags: 'on_pixel' (the centre of a Sersic-law component IS a pixel centre: NaN there,
    -inf), 'near_pixel' (1e-7 px off one: the log-likelihood keeps the 1e-5 of the raster extremes, for their reason),
    'below_floor' (the component's whole image is below RASTER_FLOOR), 'ramp' (a spiral whose ramp exponent passes
    1024 inside r_in, or comes near it: finite at every pixel in the definition and in the reference)."""
    ix, iy = int(nx * 0.5), ny // 2
    left = (-5.0 * nx + 0.3, ny * 0.5 + 0.3)
    on, near = (float(ix), float(iy)), (ix + 1e-7, iy - 3e-8)
    spi = lambda **kw: {'spiral_' + k: v for k, v in kw.items()}
    tru = lambda **kw: {'trunc_' + k: v for k, v in kw.items()}
    six = {'f%d_amp' % m: a for m, a in zip(Sersic.FOURIER_MODES, (0.3, -0.2, 0.19, -0.1, 0.1, -0.1))}
    six.update({'f%d_phase' % m: 40.0 * m for m in Sersic.FOURIER_MODES})
    # a_1 with v' = 0 through pixel centres: axes along the grid (angle -90, which the derived row takes exactly: m01 =
    # m10 = 0, u = dx / r_a, v = dy / r_b), the centre on a pixel corner, v' = (dy + a_1 dx) / r_b: a_1 = -1 puts the
    # ridge on the diagonal pixels dy = dx.  Radii 8 and 4: 1 / r_a, 1 / r_b and r_a / r_b are powers of two, so every
    # product is exact and v' IS 0 there in any order of operations, fused or not (the CPU companion asserts it)
    ridge = dict(angle=-90.0, xy=(ix + 0.5, iy + 0.5), reff=8.0, reff_b=4.0, bend1=-1.0)
    specs = [
        # -- boxiness (and the positions and magnitudes of the Sersic law) --
        ('box-base', 'box', {}, ()),
        ('c-1.9', 'box', dict(boxiness=-1.9), ()), ('c-1.5', 'box', dict(boxiness=-1.5), ()),
        ('c0', 'box', dict(boxiness=0.0), ()), ('c3', 'box', dict(boxiness=3.0), ()), ('c10', 'box', dict(boxiness=10.0), ()),
        ('c3-q0.01', 'box', dict(boxiness=3.0, reff=20.0, reff_b=0.2), ()),
        ('ser-on-pixel', 'box', dict(xy=on), ('on_pixel',)),
        ('ser-near-pixel', 'box', dict(xy=near, index=2.0), ('near_pixel',)),
        ('ser-left5', 'box', dict(xy=left, index=4.0), ()),
        ('ser-mag8', 'box', dict(mag=8.0), ()), ('ser-mag60', 'box', dict(mag=60.0), ()),
        # -- Fourier modes --
        ('fou-one-0.99', 'fou', dict(f1_amp=0.99, f1_phase=20.0), ()), ('fou-six-0.99', 'fou', six, ()),
        ('fou-m6-0.9', 'fou', dict(f6_amp=0.9, f6_phase=10.0), ()),
        ('fou-phase0', 'fou', dict(f2_amp=0.3, f2_phase=0.0), ()), ('fou-phase90', 'fou', dict(f2_amp=0.3, f2_phase=90.0), ()),
        ('fou-phase1e6', 'fou', dict(f2_amp=0.3, f2_phase=1e6), ()),
        ('fou-amp0', 'fou', dict(f3_amp=0.0, f3_phase=45.0), ()), ('fou-amp1e-300', 'fou', dict(f3_amp=1e-300, f3_phase=45.0), ()),
        # -- spiral: (r_in + r_out) / (r_out - r_in) = 100, 172, 181 (9, 9.1), 182, 2000 --
        ('spi-ramp100', 'spi', spi(r_in=9.0, r_out=9.0 * 101 / 99), ('ramp',)),
        ('spi-ramp172', 'spi', spi(r_in=9.0, r_out=9.0 * 173 / 171), ('ramp',)),
        ('spi-ramp181', 'spi', spi(r_in=9.0, r_out=9.1), ('ramp',)),
        ('spi-ramp182', 'spi', spi(r_in=9.0, r_out=9.0 * 183 / 181), ('ramp',)),
        ('spi-ramp2000', 'spi', spi(r_in=9.0, r_out=9.0 * 2001 / 1999), ('ramp',)),
        ('spi-rin0', 'spi', spi(r_in=0.0, r_out=1e-3), ()), ('spi-rout1e4', 'spi', spi(r_out=1e4), ()),
        ('spi-wind1e4', 'spi', spi(wind=1e4), ()), ('spi-wind1e6', 'spi', spi(wind=1e6), ()),
        ('spi-alpha0', 'spi', spi(alpha=0.0, wind=-200.0), ()), ('spi-alpha1e-3', 'spi', spi(alpha=1e-3), ()),
        ('spi-alpha5', 'spi', spi(alpha=5.0), ()), ('spi-incl89.9', 'spi', spi(incl=89.9), ()),
        ('spi-on-pixel-alpha0', 'spi', dict(xy=on), ('on_pixel',)),
        ('spi-on-pixel-alpha1', 'spi', dict(xy=on, **spi(alpha=1.0)), ('on_pixel',)),
        # -- Moffat --
        ('mof-beta1.0001', 'mof', dict(beta=1.0001), ()), ('mof-beta1.5', 'mof', dict(beta=1.5), ()),
        ('mof-beta50', 'mof', dict(beta=50.0), ()), ('mof-beta500', 'mof', dict(beta=500.0, fwhm=30.0, fwhm_b=20.0), ()),
        ('mof-fwhm0.05', 'mof', dict(fwhm=0.05, fwhm_b=0.05), ()), ('mof-fwhm3000', 'mof', dict(fwhm=3000.0, fwhm_b=2500.0), ()),
        ('mof-q0.01', 'mof', dict(fwhm=20.0, fwhm_b=0.2), ()),
        ('mof-on-pixel', 'mof', dict(xy=on), ()), ('mof-near-pixel', 'mof', dict(xy=near), ()),
        ('mof-left5', 'mof', dict(xy=left), ()),
        ('mof-mag8', 'mof', dict(mag=8.0), ()), ('mof-mag60', 'mof', dict(mag=60.0), ()),
        # -- Ferrer --
        ('fer-alpha0', 'fer', dict(alpha=0.0), ()), ('fer-alpha0.01', 'fer', dict(alpha=0.01), ()),
        ('fer-alpha20', 'fer', dict(alpha=20.0), ()),
        ('fer-beta1.999', 'fer', dict(beta=1.999), ()), ('fer-beta-50', 'fer', dict(beta=-50.0), ()),
        ('fer-rout0.3', 'fer', dict(r_out=0.3, r_out_b=0.3, xy=(ix + 0.1, iy - 0.1)), ()),
        ('fer-rout3000', 'fer', dict(r_out=3000.0, r_out_b=2500.0), ()),
        ('fer-on-pixel', 'fer', dict(xy=on), ()), ('fer-near-pixel', 'fer', dict(xy=near), ()),
        ('fer-left5', 'fer', dict(xy=left, r_out=600.0, r_out_b=400.0), ()),
        ('fer-mag8', 'fer', dict(mag=8.0), ()), ('fer-mag60', 'fer', dict(mag=60.0), ()),
        # -- truncation --
        ('tru-in-1e-3', 'tru', tru(in_lo=10.0, in_hi=10.001), ()), ('tru-out-1e-3', 'tru', tru(out_lo=10.0, out_hi=10.001), ()),
        ('tru-lo0', 'tru', tru(in_lo=0.0, in_hi=4.0), ()), ('tru-hi1e6', 'tru', tru(out_lo=5.0, out_hi=1e6), ()),
        ('tru-out-first-pixel', 'tru', dict(xy=(ix + 0.5, iy + 0.5), **tru(out_lo=0.0, out_hi=1e-3)), ('below_floor',)),
        ('tru-in-beyond', 'tru', tru(in_lo=200.0, in_hi=300.0), ()),
        ('tru-overlap', 'tru', tru(in_lo=2.0, in_hi=14.0, out_lo=5.0, out_hi=9.0), ()),
        # -- bending --
        ('bnd-a4+3-q0.01', 'bnd', dict(reff=0.5, reff_b=0.005, bend4=3.0), ()),
        ('bnd-a4-3-q0.01', 'bnd', dict(reff=0.5, reff_b=0.005, bend4=-3.0), ()),
        ('bnd-ridge', 'bnd', ridge, ()), ('bnd-a1-3', 'bnd', dict(bend1=3.0), ()),
        ('bnd-amp0', 'bnd', dict(bend2=0.0, bend3=0.0), ()), ('bnd-amp1e-300', 'bnd', dict(bend2=1e-300, bend3=-1e-300), ()),
        ('bnd-a2-3-c3', 'bnd', dict(bend2=3.0, boxiness=3.0), ()),
    ]
    return specs


# solo cases with fewer than 500 pixels above RASTER_FLOOR, each with its reason (the CPU test holds the list to this)
FEW_PIXELS = {
    'fer-rout0.3': 'a cut-off radius of 0.3 px: one pixel centre is inside it, the law is exactly 0 on the others',
    'bnd-a4+3-q0.01': "v' = v + 300 u^4 with u = x / 0.5: rho^2 passes 1e10 a few pixels from the centre and the "
                      'n = 1.5 law underflows',
    'bnd-a4-3-q0.01': 'as bnd-a4+3-q0.01, bent the other way',
    'tru-out-1e-3': 'an outer ramp 1e-3 px wide at radius 10 along the major axis of a 7 x 3.5 component: the disc '
                    'inside it has 144 pixels, and 0.08 px beyond it the factor is below 1e-280',
}
# cases whose fp64 DEFINITION is farther than E_DEF_CAP from the long-double image, each with its reason (the CPU test
# holds the list to this and caps it at a tenth of the list).  EMPTY: with the truncation factors written as
# 1 / (1 + exp(-+2a)) (`Sersic.truncation_weight`) the definition's worst is several 1e-11 (spi-alpha5: a winding angle
# of thousands of radians), and the 1e-3-px ramps, whose argument amplifies the rounding of rho by r / width = 1e4, stay
# at one or two 1e-11 -- both bound the device at 4 x that, none needs the cap.  (The last digits of these figures are
# those of the platform's libm; the CPU companion prints them per case and asserts only the cap.)
LOOSENED = {}
# the reduced list of the pixel-mean kernels: spiral ramps, truncation tails, bending, one case of each law
MEAN_CASES = ('box-base', 'c3', 'fou-six-0.99', 'spi-ramp100', 'spi-ramp181', 'spi-ramp2000', 'mof-beta1.5', 'fer-alpha0.01',
              'tru-in-beyond', 'tru-hi1e6', 'tru-overlap', 'bnd-ridge', 'bnd-a1-3', 'bnd-a2-3-c3')


def specs_of(family, names=None, shape=SHAPE):
    return [s for s in general_extreme_specs(*shape) if s[1] == family and (names is None or s[0] in names)]


# ---------------------------------------------------------------------------------------------------------------
# models, walkers, references
# ---------------------------------------------------------------------------------------------------------------
def U(lo, hi):
    return Uniform(loc=lo, scale=hi - lo)


def _keyword_priors(keys):
    """Every value of the keywords free, under Uniform priors that hold every value of the list."""
    kw = dict(boxiness=U(-1.99, 12.0))
    if 'fourier' in keys:
        kw['fourier'] = {m: (U(-1.0, 1.0), U(-1e3, 2e6)) for m in Sersic.FOURIER_MODES}
    if 'spiral' in keys:
        kw['spiral'] = dict(r_in=U(0.0, 2e4), r_out=U(0.0, 2e4), winding=U(-2e6, 2e6), alpha=U(0.0, 10.0),
                            inclination=U(-90.0, 90.0), sky_angle=U(-360.0, 360.0))
    if 'truncation' in keys:
        kw['truncation'] = {k: (U(0.0, 2e6), U(0.0, 2e6)) for k in ('inner', 'outer')}
    if 'bending' in keys:
        kw['bending'] = {m: U(-5.0, 5.0) for m in Sersic.BEND_MODES}
    return kw


def lift_of(family, level):
    """The keyword of the dark third component that lifts the family's context to `level` (None: the family's own)."""
    own = FAMILIES[family][2]
    assert LEVELS.index(level) >= LEVELS.index(own) or (level, own) == ('fou+spi', 'spi'), (family, level)
    if level == own:
        return None
    lift = LIFTS[level]
    return lift[family] if isinstance(lift, dict) else lift


def build_model(fld, family, level=None, mean=False, backend='fused', max_walkers=16):
    """Sky + PointSource + two slots of the family's class, every parameter free under wide Uniform priors, and --
    where `level` is above the family's own -- a third, DARK Sersic with constants only that carries the keyword of
    that level: the context then runs that level's kernels, in which the family's blocks are wave-uniform branches."""
    ny, nx = fld['shape']
    cls, keys, own = FAMILIES[family]
    wide = lambda: Uniform(loc=np.array([-2e4, -2e4]), scale=np.array([4e4, 4e4]))
    comps = [Configuration(fld['sci'], fld['ivm'], fld['psf'], fld['psf_ivm'], mag_zeropoint=fld['mag_zp']),
             Sky(adu=Normal(loc=0.05, scale=0.05)), PointSource(xy=wide(), mag=U(0.0, 70.0))]
    for _ in range(2):
        kw = dict(xy=wide(), mag=U(0.0, 70.0), angle=U(-1e3, 2e6), angle_degrees=True, pixel_mean=mean,
                  **_keyword_priors(keys))
        if cls == 'Sersic':
            kw.update(reff=U(0.001, 5000.0), reff_b=U(0.001, 5000.0), index=U(0.05, 20.0))
        elif cls == 'Moffat':
            kw.update(fwhm=U(0.001, 5000.0), fwhm_b=U(0.001, 5000.0), beta=U(1.0, 1000.0))
        else:
            kw.update(r_out=U(0.001, 5000.0), r_out_b=U(0.001, 5000.0), alpha=U(0.0, 50.0), beta=U(-100.0, 2.0))
        comps.append(CLASSES[cls](**kw))
    lift = lift_of(family, level or own)
    if lift is not None:
        d = slot_values('box', 'dark', 0, ny, nx)
        extra = {'fourier': dict(fourier={2: (0.1, 30.0)}), 'truncation': dict(truncation={'outer': (12.0, 18.0)}),
                 'spiral': dict(spiral=dict(r_in=2.0, r_out=9.0, winding=150.0)), 'bending': dict(bending={2: 0.1})}[lift]
        comps.append(Sersic(xy=d['xy'], mag=d['mag'], reff=d['reff'], reff_b=d['reff_b'], index=d['index'],
                            angle=d['angle'], angle_degrees=True, boxiness=0.0, **extra))
    return MultiComponentModel(comps, backend=backend, max_walkers=max_walkers)


def level_of(model):
    """The GenLevel a context of this model runs (psfmc_hip.hip general_launch), from the model's own block tags."""
    if any(model.sersic_bending_masks):
        return 'bnd'
    if any(model.sersic_truncation_flags):
        return 'tru'
    if any(model.sersic_radial_kinds):
        return 'rad'
    return ('plain', 'fou', 'spi', 'fou+spi')[int(any(model.sersic_fourier_masks)) + 2 * int(any(model.sersic_spiral_flags))]


def theta_of(model, values):
    """One parameter vector from {parameter name: value}; every free parameter must be named and no other."""
    vals = dict(values)
    out = []
    for name in model.param_names:
        out += list(np.ravel(vals.pop(name)))
    assert not vals, sorted(vals)
    return np.array(out, dtype=np.float64)


def named_walker(family, head, slots):
    cls = FAMILIES[family][0]
    vals = {'0_Sky_adu': head[0], '1_PointSource_mag': head[1], '1_PointSource_xy': head[2]}
    for j, s in enumerate(slots):
        vals.update({'%d_%s_%s' % (2 + j, cls, k): v for k, v in s.items()})
    return vals


def extreme_walkers(model, family, names=None, shape=SHAPE):
    """The walker list of one family: every extreme twice, as `helpers.extreme_walkers` -- MIXED (the extreme in slot
    k % 2, the other slot the family's ordinary boxy component, sky and point source on) and SOLO (the other slot dark,
    no sky, the point source's window empty: the raw model is the extreme component alone).
    Returns (theta [n, P], info: list of dict(name, family, kind, slot, flags))."""
    ny, nx = shape
    theta, info = [], []
    for k, (name, fam, over, flags) in enumerate(specs_of(family, names, shape)):
        slot = k % 2
        for kind in ('mixed', 'solo'):
            slots = [slot_values(family, 'ordinary' if kind == 'mixed' else 'dark', j, ny, nx) for j in range(2)]
            ext = slot_values(family, 'extreme', slot, ny, nx)
            ext.update(over)
            slots[slot] = ext
            head = ((0.01, 19.0, (nx * 0.4 + 0.25, ny * 0.45 - 0.2)) if kind == 'mixed' else
                    (0.0, 19.0, (-50.3, ny * 0.45 - 0.2)))
            theta.append(theta_of(model, named_walker(family, head, slots)))
            info.append(dict(name=name, family=family, kind=kind, slot=slot, flags=flags))
    return np.array(theta), info


def ordinary_walkers(model, family, n, seed=0, shape=SHAPE):
    """n distinct well-behaved walkers of the family's model: both slots ordinary, perturbed."""
    ny, nx = shape
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        slots = [slot_values(family, 'ordinary', j, ny, nx) for j in range(2)]
        for s in slots:
            s['angle'] += rng.uniform(-20, 20)
            s['mag'] += rng.uniform(-0.5, 0.5)
            s['xy'] = tuple(np.asarray(s['xy']) + rng.uniform(-3, 3, 2))
            s['boxiness'] += rng.uniform(-0.2, 0.2)
        head = (0.01 + rng.uniform(-0.005, 0.005), 19.0 + rng.uniform(-0.5, 0.5),
                (nx * 0.4 + rng.uniform(-3, 3), ny * 0.45 + rng.uniform(-3, 3)))
        out.append(theta_of(model, named_walker(family, head, slots)))
    return np.array(out)


def general_pixel_errors(img, exact, sigma0, edge=None):
    """`helpers.pixel_errors` -- (largest relative error over the pixels above RASTER_FLOOR, their number, largest
    |img| over the other finite pixels) -- with the error of a model that has a Ferrer taken relative to
    max(|pixel|, Sigma_0) as `extra_contract.law_error` takes it: next to the cut-off the law is far below the peak and
    exactly 0 beyond it.  `edge`: the mask of the pixels within EDGE_MARGIN of a Ferrer's cut-off, which are not
    compared.  sigma0 = 0: `helpers.pixel_errors` itself."""
    if not sigma0:
        return helpers.pixel_errors(img, exact)
    exact, img = np.asarray(exact), np.asarray(img)
    fin = np.isfinite(exact) & (~edge if edge is not None else True)
    big = fin & (np.abs(exact) > RASTER_FLOOR)
    with np.errstate(all='ignore'):
        scale = np.maximum(np.abs(exact), np.longdouble(sigma0))
        err = float(np.max(np.abs(img[fin].astype(np.longdouble) - exact[fin]) / scale[fin])) if fin.any() else 0.0
        low = float(np.max(np.abs(img[fin & ~big]))) if (fin & ~big).any() else 0.0
    return err, int(big.sum()), low


def longdouble_raw_model(model, theta, memo=None):
    """(the raw model of one vector with every general component from `longdouble_general`, the sky's level and the
    point source from the fp64 oracle; the smallest Sigma_0 of its Ferrer components, 0 without one; the mask of the
    pixels where a Ferrer's |1 - x| is below EDGE_MARGIN: the pixels the comparison leaves out)."""
    model.param_values = np.asarray(theta, dtype=np.float64)
    shape = model.config.obs_data.shape
    zp = model.config.mag_zeropoint
    base = np.zeros(shape)
    sigma0, edge = 0.0, np.zeros(shape, dtype=bool)
    for comp in model.components:
        if isinstance(comp, PointSource):
            orc.add_point_source(base, np.ravel(comp.xy), float(np.ravel(comp.mag)[0]), zp, orc.array_coords(shape),
                                 comp.shift_method)
        elif isinstance(comp, Sky):
            base += float(np.ravel(comp.adu)[0])
    raw = base.astype(np.longdouble)
    for comp in model.components:
        if isinstance(comp, Sersic):
            args = component_args(comp, zp)
            key = repr((args, shape))
            got = memo.get(key) if memo is not None else None
            if got is None:
                got = longdouble_general(*args, shape=shape)
                if memo is not None:
                    memo[key] = got
            img, xk = got
            raw = raw + img
            if xk is not None:
                central = float(walker_scalars(*args[:6])[1])
                sigma0 = central if not sigma0 else min(sigma0, central)
                edge |= np.asarray(np.abs(1 - xk) < EDGE_MARGIN)
    return raw, sigma0, edge


_REFS = {}


def extreme_references(family, level=None, shape=SHAPE, names=None):
    """Everything the device is held to for one family's walkers in a context of `level` (None: the family's own),
    computed once per process and left unchanged: dict(fld, field, theta, info, ll [n] (the contract's: the fp64 numpy
    definition through the oracle's convolution and likelihood; -inf where not finite), images (the contract's, per
    walker), exact (long-double raw models), sigma0 [n], edge (per walker: the pixels left out next to a Ferrer's cut-off),
    e_def [n] (the definition's largest pixel error
    against them), n_rel [n], bound [n], ll_bound [n])."""
    key = (family, level, shape, names)
    if key in _REFS:
        return _REFS[key]
    fld = tgg.make_field(shape[0], shape[1], seed=31)
    field = tgg.oracle_field(fld)
    model = build_model(fld, family, level, backend='hipfft', max_walkers=1)
    theta, info = extreme_walkers(model, family, names, shape)
    n = len(theta)
    ll, images, exact = np.empty(n), [], []
    sigma0, edge, e_def, n_rel = np.empty(n), [], np.empty(n), np.empty(n, dtype=int)
    bound, ll_bound = np.empty(n), np.empty(n)
    memo = {}
    for i, t in enumerate(theta):
        with np.errstate(all='ignore'):
            want, imgs = tgg.contract_evaluate(model, field, t)
        ll[i] = want if np.isfinite(want) else -np.inf
        images.append(imgs)
        ex, sigma0[i], near = longdouble_raw_model(model, t, memo)
        exact.append(ex)
        edge.append(near)
        e_def[i], n_rel[i], _ = general_pixel_errors(imgs['raw_model'], ex, sigma0[i], near)
        bound[i] = max(RAW_BOUND, RASTER_ORACLE_FACTOR * e_def[i])
        if np.isfinite(ll[i]):
            ll_bound[i] = (1e-5 * abs(ll[i]) if 'near_pixel' in info[i]['flags']
                           else fuzz_shapes.fuzz_bound(field, imgs, ll[i]))
        else:
            ll_bound[i] = 0.0
    refs = dict(fld=fld, field=field, shape=shape, theta=theta, info=info, ll=ll, images=images, exact=exact,
                sigma0=sigma0, edge=edge, e_def=e_def, n_rel=n_rel, bound=bound, ll_bound=ll_bound)
    _REFS[key] = refs
    return refs
