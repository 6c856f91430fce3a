"""Shared test helpers: golden-case loading, model construction from the
golden arrays (through the product's own FITS writer + model-file DSL), and an
INDEPENDENT theta -> oracle-components translation (it knows each case's
component layout from the case definition, not from the product's packing
code)."""
import os

import numpy as np

import psfmc_oracle as orc
import synth_field

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# component layout of each golden case, in model-file order
LAYOUT = {
    'example': [('sky',), ('ps', 'lanczos3'), ('sersic', True), ('sersic', True)],
    'synth256': [('ps', 'lanczos3'), ('sersic', True)],
    'synth128x2': [('ps', 'lanczos3'), ('sersic', True), ('sersic', True)],
    'edge': [('sky',), ('ps', 'bilinear'), ('ps', 'lanczos3'), ('sersic', False)],
}
HAS_PSF_INDEX = {'edge'}
# vectors whose result is ill-conditioned (Sersic centre 1e-6 px from a pixel
# centre: the core pixel amplifies last-bit differences in dx, dy by ~1e8), so
# even numpy 1.26 vs numpy 2.2 runs of the SAME oracle differ at 1e-8
ILL_CONDITIONED = {'edge': [27]}


def well_conditioned(name, n):
    keep = np.ones(n, dtype=bool)
    keep[ILL_CONDITIONED.get(name, [])] = False
    return keep


def load_case(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False))


# "light" golden cases (BASELINE configs 3 and 4): the fixture holds the vectors and the REFERENCE's scalars
# only; the field is regenerated from its seed (tools/synth_field.py, the same code and seed
# tests/golden/make_golden.py fed the reference with) and compared through the fixture's `field_check`
LIGHT = {'synth512x2': (512, 2), 'synth1024x4': (1024, 4)}


def field_check(arrays):
    """tests/golden/make_golden.py field_check: float64 sums and a few pixels of every input array."""
    vals = []
    for a in [arrays['sci'], arrays['ivm']] + list(arrays['psfs']) + list(arrays['psf_ivms']):
        a = np.asarray(a, dtype=np.float64)
        vals += [a.sum(), np.abs(a).sum(), (a * a).sum(), a[0, 0], a[a.shape[0] // 2, a.shape[1] // 3], a[-1, -1]]
    return np.array(vals)


def load_light_case(name):
    """(case dict with the regenerated arrays filled in, synth field dict)."""
    n_side, n_sersic = LIGHT[name]
    case = load_case(name)
    fld = synth_field.make_field(n_side, n_sersic, seed=0)
    case.update(sci=fld['sci'], ivm=fld['ivm'], psfs=np.asarray([fld['psf']]), psf_ivms=np.asarray([fld['psf_ivm']]))
    # the arrays the reference was fed with are float32 FITS images: the regenerated ones must be those, to the bit
    # (sums of ~1e6 float32 values as float64: differences of one ulp of a pixel would show at 1e-13)
    got = field_check(case)
    assert np.allclose(got, case['field_check'], rtol=1e-13, atol=0), 'regenerated field differs from the fixture\'s'
    LAYOUT.setdefault(name, synth_layout(n_sersic))
    return case, fld


def synth_layout(n_sersic):
    return [('ps', 'lanczos3')] + [('sersic', True)] * n_sersic


def comps_from_theta(layout, theta, has_psf_index=False):
    """emcee vector -> (oracle comps, psf_index).  Packing: alphabetical inside
    a component (PointSource: mag, x, y; Sersic: angle, index, mag, reff,
    reff_b, x, y), components in file order, psf_index last."""
    theta = np.asarray(theta, dtype=np.float64)
    pos, comps = 0, []
    for item in layout:
        if item[0] == 'sky':
            comps.append(dict(type='sky', adu=theta[pos]))
            pos += 1
        elif item[0] == 'ps':
            comps.append(dict(type='ps', mag=theta[pos], xy=theta[pos + 1:pos + 3],
                              method=item[1]))
            pos += 3
        else:
            a, n, m, re, rb, x, y = theta[pos:pos + 7]
            comps.append(dict(type='sersic', angle=a, index=n, mag=m, reff=re,
                              reff_b=rb, xy=np.array([x, y]),
                              angle_degrees=item[1]))
            pos += 7
    psf_index = theta[pos] if has_psf_index else 0
    return comps, psf_index


def oracle_field(case):
    return orc.make_field(case['sci'], case['ivm'], list(case['psfs']),
                          list(case['psf_ivms']), mask=case.get('mask'),
                          mag_zp=float(case['mag_zp']))


def oracle_loglike(field, layout, theta, has_psf_index=False, raw_dtype=np.float64):
    comps, psf = comps_from_theta(layout, theta, has_psf_index)
    if has_psf_index and not (0 <= np.rint(psf) < len(field.psf_spec)):
        return -np.inf
    return orc.log_likelihood(field, comps, psf, raw_dtype=raw_dtype)


def write_case_files(name, case, directory):
    """FITS inputs + model file for a golden case, via the product's writer.
    Returns the model file path."""
    from psfmc_amd import fits_io
    directory = str(directory)
    if name == 'example':
        return os.path.join(GOLDEN, 'example', 'model_example.py')
    fits_io.write_image(os.path.join(directory, 'sci.fits'), case['sci'])
    fits_io.write_image(os.path.join(directory, 'ivm.fits'), case['ivm'])
    if name == 'edge':
        for k in range(len(case['psfs'])):
            fits_io.write_image(os.path.join(directory, 'psf%d.fits' % k), case['psfs'][k])
            fits_io.write_image(os.path.join(directory, 'psfivm%d.fits' % k),
                                case['psf_ivms'][k])
        fits_io.write_image(os.path.join(directory, 'mask.fits'), case['mask'])
        with open(os.path.join(GOLDEN, 'edge_model.py')) as f:
            text = f.read()
    else:
        fits_io.write_image(os.path.join(directory, 'psf.fits'), case['psfs'][0])
        fits_io.write_image(os.path.join(directory, 'psf_ivm.fits'), case['psf_ivms'][0])
        n_side = case['sci'].shape[0]
        n_sersic = len(LAYOUT[name]) - 1
        text = synth_field.model_file_text(n_side, n_sersic)
    path = os.path.join(directory, 'model.py')
    with open(path, 'w') as f:
        f.write(text)
    return path


def build_model(name, case, directory, **kwargs):
    from psfmc_amd import MultiComponentModel
    return MultiComponentModel(write_case_files(name, case, directory), **kwargs)


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), 'finite masks differ'
    assert np.array_equal(got[~fin], ref[~fin]), 'non-finite values differ'
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - ref[fin]) / np.abs(ref[fin])))


def longdouble_weight_map(field, raw, psf_index):
    """models.py:265-280 with the two transforms of the variance convolution in numpy `longdouble`
    (x87 80-bit: 64-bit significand): the composite inverse-variance map to ~1e-19 of the norm of
    raw^2, i.e. 'exact' next to any fp64 evaluation -- the yardstick for how far the fp64 oracle
    itself sits from the true weight map (tests/test_oracle_precision.py, test_gpu_random.py)."""
    ld = np.longdouble
    shape = raw.shape
    k = int(np.rint(psf_index))
    kernel = np.fft.irfft2(np.asarray(field.var_spec[k]).astype(np.clongdouble), s=shape)
    spec = np.fft.rfft2(kernel.astype(ld))
    model_var = np.fft.ifftshift(np.fft.irfft2(np.fft.rfft2(np.asarray(raw, dtype=ld) ** 2) * spec, s=shape))
    with np.errstate(all='ignore'):
        return 1 / (model_var + np.asarray(field.obs_var, dtype=ld))


# ---------------------------------------------------------------------------
# The Sersic rasteriser at prior-reachable extremes (tests/test_gpu_raster_extremes.py on the device,
# tests/test_raster_extremes_reference.py for the references and the conditions that need no GPU)
# ---------------------------------------------------------------------------
# One image shape per FORM of the fused rasteriser, 64 rows each (the row length selects the form, the row count
# does not; 64 is the smallest built ny).  The rules, from the kernels' sources:
#   psfmc_device.h pow_tabs_side        transform rows of up to 256 pixels: log2 + exp2 per pixel, else power tables
#   psfmc_fused_path.h raster_group     G = 2 on the power-of-two kernels from 512 on; G = 4 (with the prefetch chain)
#                                       on general sides above 256 with more than 16 complex registers per lane,
#                                       except 264 / 286 / 294; else G = 1
#   psfmc_rows3_path.h rows3_pick       sides above 1024: one row per wave, G = 1 without prefetch
#   k_rows_fwd / k_rows3_fwd            the WRAP variants (embedded images) of a power-table kernel run G = 1
# (tag, image shape, PSF shape, back end, form, wrap, what get_option must report: pow_tabs, rows3 forward bit,
# raster_group).  An embedded image's transform side is the library's choice (choose_embedding): the table gives
# the range it must fall in and the test reads the side back.
RASTER_FORMS = [
    ('logexp-64',    (64, 64),   (21, 21), 'fused',  'logexp', False, dict(pow_tabs=0, rows3_fwd=0, raster_group=0)),
    ('logexp-256',   (64, 256),  (21, 21), 'fused',  'logexp', False, dict(pow_tabs=0, rows3_fwd=0, raster_group=0)),
    ('g1-264',       (64, 264),  (21, 21), 'fused',  'g1',     False, dict(pow_tabs=1, rows3_fwd=0, raster_group=1)),
    ('g4-288',       (64, 288),  (21, 21), 'fused',  'g4',     False, dict(pow_tabs=1, rows3_fwd=0, raster_group=4)),
    ('g2-512',       (64, 512),  (21, 21), 'fused',  'g2',     False, dict(pow_tabs=1, rows3_fwd=0, raster_group=2)),
    ('rows3-1152',   (64, 1152), (21, 21), 'fused',  'rows3',  False, dict(pow_tabs=1, rows3_fwd=1, raster_group=1)),
    ('wrap-logexp',  (64, 170),  (21, 21), 'fused',  'logexp', True,  dict(pow_tabs=0, rows3_fwd=0, raster_group=0)),
    ('wrap-g1',      (64, 270),  (21, 21), 'fused',  'g1',     True,  dict(pow_tabs=1, rows3_fwd=0, raster_group=1)),
    ('wrap-rows3',   (64, 1100), (21, 21), 'fused',  'rows3',  True,  dict(pow_tabs=1, rows3_fwd=1, raster_group=1)),
    ('hipfft-200',   (64, 200),  (21, 21), 'hipfft', 'ocml',   False, None),
]
RASTER_FLOOR = 1e-280            # per-pixel relative checks run above it; below, the device must stay under 10 x it
EXTREME_LAYOUT = [('sky',), ('ps', 'lanczos3')] + [('sersic', True)] * 3
EXTREME_ZP = 25.0
# per-pixel bound: max(the project's 1e-11, 4 x the fp64 oracle's own error against the long-double image)
RASTER_PIXEL_BOUND, RASTER_ORACLE_FACTOR = 1e-11, 4.0


def longdouble_sersic(shape, xy, mag, reff, reff_b, index, angle, angle_degrees, mag_zp):
    """The oracle's `add_sersic` (Sersic.py:98-153) with every per-pixel operation in numpy `longdouble` (x87: 64-bit
    significand).  The per-walker scalars -- kappa, Sigma_e, the ellipse matrix, 1 / (2n) -- are the fp64 values the
    oracle computes and the host hands to the kernels: the per-pixel error of an fp64 rasteriser is what this
    measures."""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63, 'numpy longdouble is not the 80-bit type here'
    kappa64 = orc.sersic_kappa(index)
    kappa = ld(kappa64)
    sbeff = ld(orc.sersic_sb_eff(orc.mag_to_flux(mag, mag_zp), index, reff, reff_b, kappa64))
    xform = orc.sersic_xform(reff, reff_b, angle, angle_degrees).astype(ld)
    radius_pow = ld(0.5 / index)
    offs = (orc.array_coords(shape).astype(ld) - np.asarray(xy, dtype=np.float64).astype(ld)).T
    with np.errstate(all='ignore'):
        sq_radii = np.sum(np.dot(xform, offs) ** 2, axis=0)
        sq_delta_r = sq_radii / np.sum(offs ** 2, axis=0)
        sb = np.exp(-kappa * np.expm1(np.log(sq_radii) * radius_pow))
        grad = -kappa * 2 * radius_pow * np.exp(np.log(sq_radii) * (radius_pow - ld(0.5)))
        cent = sq_delta_r / 12 * grad
        return (sbeff * sb * (1 + grad * cent)).reshape(shape)


def longdouble_raw_model(field, comps, memo=None):
    """The raw model of `comps` with the Sersic components from `longdouble_sersic`; the sky and the point sources
    from the fp64 oracle (a constant and a product of two fp64 weights: exact enough).  `memo` (a dict) keeps the
    components' images by their parameters: the walkers of one list share most of their slots."""
    raw = orc.raw_model(field, [c for c in comps if c['type'] != 'sersic'], raw_dtype=np.float64).astype(np.longdouble)
    for c in comps:
        if c['type'] == 'sersic':
            args = (tuple(field.shape), (float(c['xy'][0]), float(c['xy'][1])), float(c['mag']), float(c['reff']),
                    float(c['reff_b']), float(c['index']), float(c['angle']), bool(c.get('angle_degrees', False)),
                    float(field.mag_zp))
            img = memo.get(args) if memo is not None else None
            if img is None:
                img = longdouble_sersic(*args)
                if memo is not None:
                    memo[args] = img
            raw = raw + img
    return raw


def pixel_errors(img, exact):
    """(largest relative error of `img` against the long-double image over the pixels above RASTER_FLOOR, number of
    such pixels, largest |img| over the other finite pixels)."""
    exact = np.asarray(exact)
    fin = np.isfinite(exact)
    big = fin & (np.abs(exact) > RASTER_FLOOR)
    img = np.asarray(img)
    with np.errstate(all='ignore'):
        rel = float(np.max(np.abs(img[big].astype(np.longdouble) - exact[big]) / np.abs(exact[big]))) if big.any() else 0.0
        low = float(np.max(np.abs(img[fin & ~big]))) if (fin & ~big).any() else 0.0
    return rel, int(big.sum()), low


def extreme_slots(ny, nx):
    """The three ordinary Sersic slots [angle (degrees), index, mag, reff, reff_b, x, y] of an ny x nx image."""
    return np.array([[30.0, 1.0, 19.0, 4.0, 2.5, nx * 0.25 + 0.3, ny * 0.31 + 0.4],
                     [75.0, 2.5, 18.5, 5.0, 3.0, nx * 0.5 + 0.7, ny * 0.52 + 0.3],
                     [140.0, 4.0, 19.5, 3.0, 2.0, nx * 0.75 - 0.4, ny * 0.7 - 0.2]])


def extreme_dark_slot(ny, nx):
    """A slot whose every pixel underflows to zero (n = 0.1, five sides to the left): the neighbours of a `solo`
    walker, whose raw model is then the extreme component alone."""
    return np.array([10.0, 0.1, 20.0, 3.0, 2.0, -5.0 * nx + 0.3, ny * 0.5 + 0.3])


def extreme_specs(ny, nx):
    """(name, overrides of the slot's parameters, flags) of every extreme; x / y are absolute positions.  Flags:
    'on_pixel' (the centre IS a pixel centre: NaN there, -inf), 'near_pixel' (1e-7 px off one: the log-likelihood
    keeps the 1e-5 of test_power_table_rasteriser_extreme_indices, for the reason it states), 'below_floor' (the
    component's whole image is below RASTER_FLOOR: no relative check, the device must be under 1e-279 everywhere)."""
    ix, iy = int(nx * 0.5), ny // 2
    left = -5.0 * nx + 0.3
    specs = [
        ('base', {}, ()),
        # index
        ('n0.1', dict(index=0.1, reff=9.0, reff_b=7.0), ()), ('n0.3', dict(index=0.3), ()), ('n8', dict(index=8.0), ()),
        ('n15', dict(index=15.0), ()),
        # reff
        ('reff-tiny', dict(reff=0.05, reff_b=0.05), ()), ('reff-huge', dict(reff=3000.0, reff_b=2500.0), ()),
        # axis ratio
        ('round', dict(reff=4.0, reff_b=4.0), ()), ('q0.01', dict(reff=20.0, reff_b=0.2), ()),
        ('q0.01-n0.1', dict(reff=20.0, reff_b=0.2, index=0.1), ()),
        ('q0.01-n15', dict(reff=20.0, reff_b=0.2, index=15.0), ()),
        # angles (degrees): the cosines of 90 and 270 are 6e-17 and -2e-16 in fp64
        ('ang0', dict(angle=0.0), ()), ('ang90', dict(angle=90.0), ()), ('ang180', dict(angle=180.0), ()),
        ('ang270', dict(angle=270.0), ()), ('ang-90', dict(angle=-90.0), ()), ('ang1e6', dict(angle=1e6), ()),
        # centres
        ('corner', dict(x=ix + 0.5, y=iy + 0.5), ()),
        ('near-pixel', dict(x=ix + 1e-7, y=iy - 3e-8, index=2.0), ('near_pixel',)),
        ('on-pixel', dict(x=float(ix), y=float(iy)), ('on_pixel',)),
        ('off-corner-n6', dict(x=nx - 1 + 28.4, y=ny - 1 + 28.2, index=6.0), ()),
        ('left5', dict(x=left, index=4.0), ()),
        ('left5-reff-tiny', dict(x=left, reff=0.05, reff_b=0.05), ()),
        ('left5-n0.1', dict(x=left, index=0.1), ('below_floor',)),
        ('left5-q0.01-n0.1', dict(x=left, index=0.1, reff=20.0, reff_b=0.2), ('below_floor',)),
        # magnitudes (zero-point 25)
        ('mag8', dict(mag=8.0), ()), ('mag35', dict(mag=35.0), ()), ('mag60', dict(mag=60.0), ()),
        # the two ends of the power tables' exponent range (psfmc_device.h kPowTabE: rho^2 = 2^e m, e clamped to
        # [-128, 127]): e = -128 at pixel (0, 0), 1.15e-16 px from the centre of a round n = 1, r_eff = 2500 profile
        # (rho^2 = 2.1e-39; the centroid term there, 4e-8 of the pixel, is proportional to (rho^2)^(2p)), and e = 127
        # on every pixel of an n = 15, r_eff = 1 profile 1.1e19 px to the left (rho^2 = 1.2e38; 2^(1/30) per exponent
        # step, values of 1e-227: above the floor)
        ('tab-low', dict(x=1.15e-16, y=0.0, reff=2500.0, reff_b=2500.0, index=1.0), ()),
        ('tab-high', dict(x=-1.1e19, index=15.0, reff=1.0, reff_b=1.0), ()),
    ]
    return specs


# cases with fewer than 500 pixels in the relative check, each with its reason (the CPU test holds the list to this)
FEW_PIXELS = {
    'left5-n0.1': 'exp(-kappa rho^10) with rho >= 100: every pixel underflows to zero',
    'left5-q0.01-n0.1': 'as left5-n0.1, along the 0.2-px minor axis',
    'q0.01-n0.1': 'the n = 0.1 profile ends 1.2 r_eff out and its minor axis is 0.2 px: a line of 60 ... 72 pixels',
}
_SLOT_COL = dict(angle=0, index=1, mag=2, reff=3, reff_b=4, x=5, y=6)


def extreme_walkers(ny, nx):
    """The walker list of one shape: every extreme of `extreme_specs` twice -- MIXED (the extreme in slot k % 3, its
    two neighbours ordinary, sky and point source on: the prefetch chain hands tables from an extreme component to an
    ordinary one and back) and SOLO (the same slot, the neighbours dark, no sky, the point source's window empty:
    the raw model is the extreme component alone, so that its every pixel is in the relative check).
    Returns (theta [n, 25], info: list of dict(name, kind, slot, flags))."""
    slots = extreme_slots(ny, nx)
    dark = extreme_dark_slot(ny, nx)
    theta, info = [], []
    for k, (name, over, flags) in enumerate(extreme_specs(ny, nx)):
        slot = k % 3
        for kind in ('mixed', 'solo'):
            s = slots.copy() if kind == 'mixed' else np.array([slots[slot] if j == slot else dark for j in range(3)])
            for key, val in over.items():
                s[slot, _SLOT_COL[key]] = val
            head = [0.01, 19.0, nx * 0.4 + 0.25, ny * 0.45 - 0.2] if kind == 'mixed' else [0.0, 19.0, -50.3, ny * 0.45 - 0.2]
            theta.append(np.concatenate([head, s.ravel()]))
            info.append(dict(name=name, kind=kind, slot=slot, flags=flags))
    return np.array(theta), info


def ordinary_walkers(ny, nx, n, seed=0):
    """n distinct well-behaved walkers of the extreme model (the ordinary slots, perturbed): what a batch is padded
    with, and the walkers whose bits must not depend on the extreme ones beside them."""
    rng = np.random.RandomState(seed)
    slots = extreme_slots(ny, nx)
    out = []
    for _ in range(n):
        s = slots.copy()
        s[:, 0] += rng.uniform(-20, 20, 3)
        s[:, 1] *= rng.uniform(0.8, 1.25, 3)
        s[:, 2] += rng.uniform(-0.5, 0.5, 3)
        s[:, 3] *= rng.uniform(0.9, 1.3, 3)
        s[:, 4] *= rng.uniform(0.7, 1.0, 3)
        s[:, 5:] += rng.uniform(-3, 3, (3, 2))
        head = [0.01 + rng.uniform(-0.005, 0.005), 19.0 + rng.uniform(-0.5, 0.5),
                nx * 0.4 + rng.uniform(-3, 3), ny * 0.45 + rng.uniform(-3, 3)]
        out.append(np.concatenate([head, s.ravel()]))
    return np.array(out)


def extreme_case(shape, psf_shape, ps_method='lanczos3'):
    """The field and model of one RASTER_FORMS shape: a random field with bad pixels (test_gpu_random.edge_case),
    zero-point 25, Sky + a Lanczos point source + three Sersic slots, every parameter free under Uniform priors wide
    enough for every value of `extreme_specs`.  `test_gpu_random.build(case, backend, max_walkers)` builds it."""
    import test_gpu_random as tgr
    ny, nx = shape
    slots = extreme_slots(ny, nx)
    comps = [dict(type='sky', adu=0.01), dict(type='ps', xy=(nx * 0.4 + 0.25, ny * 0.45 - 0.2), mag=19.0, method=ps_method)]
    for s in slots:
        comps.append(dict(type='sersic', angle=s[0], index=s[1], mag=s[2], reff=s[3], reff_b=s[4], xy=(s[5], s[6]),
                          angle_degrees=True))
    case = tgr.edge_case(77000 + ny * 7 + nx, shape, psf_shape, comps, n_walkers=3)
    case['mask'] = None
    case['zp'] = EXTREME_ZP
    wide_xy = (np.array([-2e19, -2e19]), np.array([2e19, 2e19]))
    priors = [dict(adu=(np.asarray(-1.0), np.asarray(1.0))),
              dict(mag=(np.asarray(0.0), np.asarray(70.0)), xy=wide_xy)]
    for _ in range(3):
        priors.append(dict(angle=(np.asarray(-1e3), np.asarray(2e6)), index=(np.asarray(0.05), np.asarray(20.0)),
                           mag=(np.asarray(0.0), np.asarray(70.0)), reff=(np.asarray(0.01), np.asarray(5000.0)),
                           reff_b=(np.asarray(0.01), np.asarray(5000.0)), xy=wide_xy))
    case['priors'] = priors
    case['layout'] = [('sky',), ('ps', ps_method)] + [('sersic', True)] * 3
    case['has_psf_index'] = False
    for key in ('theta', 'outside'):
        case.pop(key, None)
    return case


def extreme_field(case):
    return orc.make_field(case['sci'], case['ivm'], case['psfs'], case['pivms'], mask=case['mask'], mag_zp=case['zp'])


_EXTREME_REFS = {}


def extreme_references(tag):
    """Everything the device is held to on one RASTER_FORMS shape, computed once per process and left unchanged:
    dict(case, field, theta, info, ll [n] (the fp64 oracle's, -inf where not finite), images (the oracle's, per
    walker), exact (long-double raw models), e_orc [n] (the oracle's largest relative pixel error against them),
    n_rel [n] (pixels in that check), bound [n] (per-pixel bound of the device), ll_bound [n])."""
    if tag in _EXTREME_REFS:
        return _EXTREME_REFS[tag]
    import fuzz_shapes
    _, shape, psf_shape = [f for f in RASTER_FORMS if f[0] == tag][0][:3]
    case = extreme_case(shape, psf_shape)
    field = extreme_field(case)
    theta, info = extreme_walkers(*shape)
    n = len(theta)
    ll, images, exact = np.empty(n), [], []
    e_orc, n_rel, bound, ll_bound = np.empty(n), np.empty(n, dtype=int), np.empty(n), np.empty(n)
    memo = {}
    for i, t in enumerate(theta):
        comps, psf = comps_from_theta(EXTREME_LAYOUT, t)
        want, imgs = orc.evaluate(field, comps, psf, raw_dtype=np.float64, want_ps_sub=True)
        ll[i] = want if np.isfinite(want) else -np.inf
        images.append(imgs)
        ex = longdouble_raw_model(field, comps, memo)
        exact.append(ex)
        e_orc[i], n_rel[i], _ = pixel_errors(imgs['raw_model'], ex)
        bound[i] = max(RASTER_PIXEL_BOUND, RASTER_ORACLE_FACTOR * e_orc[i])
        if np.isfinite(ll[i]):
            ll_bound[i] = 1e-5 * abs(ll[i]) if 'near_pixel' in info[i]['flags'] else fuzz_shapes.fuzz_bound(field, imgs, ll[i])
        else:
            ll_bound[i] = 0.0
    refs = dict(case=case, field=field, shape=shape, theta=theta, info=info, ll=ll, images=images, exact=exact,
                e_orc=e_orc, n_rel=n_rel, bound=bound, ll_bound=ll_bound)
    _EXTREME_REFS[tag] = refs
    return refs


def check_raster_form_coverage():
    """RASTER_FORMS covers {log2 + exp2, G = 1, G = 2, G = 4, one row per wave} x {plain, WRAP where the variant
    exists: the grouped forms have none, k_rows_fwd / k_rows3_fwd run G = 1 on embedded images} and the hipFFT back
    end; the power-table rows are the ones whose two table sources test_extremes_do_not_depend_on_the_batch runs."""
    from psfmc_amd import engine
    fused = {(f[4], f[5]) for f in RASTER_FORMS if f[3] == 'fused'}
    assert fused == {('logexp', False), ('g1', False), ('g2', False), ('g4', False), ('rows3', False),
                     ('logexp', True), ('g1', True), ('rows3', True)}, fused
    assert [f[4] for f in RASTER_FORMS if f[3] == 'hipfft'] == ['ocml']
    assert len({f[0] for f in RASTER_FORMS}) == len(RASTER_FORMS)
    for tag, shape, psf_shape, backend, kind, wrap, want in RASTER_FORMS:
        assert shape[0] == 64 and shape[1] <= 1152, tag
        if backend != 'fused':
            continue
        assert wrap != engine.fused_supports(*shape), tag
        assert engine.fused_supports(shape[0], shape[1], psf_shape), tag
        group = {'logexp': 0, 'g1': 1, 'g2': 2, 'g4': 4, 'rows3': 1}[kind]
        assert want == dict(pow_tabs=int(kind != 'logexp'), rows3_fwd=int(kind == 'rows3'), raster_group=group), tag
        side = shape[1] if not wrap else engine.embedding_side(shape[1], psf_shape[1])
        assert (side <= 256) == (kind == 'logexp') and (side > 1024) == (kind == 'rows3'), (tag, side)
    # the smallest and the largest log2 + exp2 row, and both table sources on every power-table form
    assert {f[1][1] for f in RASTER_FORMS if f[4] == 'logexp' and not f[5]} == {64, 256}
    assert {f[4] for f in RASTER_FORMS if f[6] and f[6]['pow_tabs']} == {'g1', 'g2', 'g4', 'rows3'}


def scale_walkers(ny, nx):
    """(name, point-source shift method, theta) of the three scale cases: a bright (mag 14) n = 6 Sersic centred 40 px
    outside a corner, and a mag 12 point source 10 px outside the image with either shift method (the Lanczos window
    holds zeros only; the bilinear weights 1 - |d| are taken at the unclipped position like the reference's), each
    beside an ordinary faint Sersic whose raw peak is of order 1; no sky."""
    faint = np.array([30.0, 1.0, 21.6, 4.0, 2.5, nx * 0.25 + 0.3, ny * 0.31 + 0.4])
    dark = extreme_dark_slot(ny, nx)
    bright = np.array([140.0, 6.0, 14.0, 3.0, 2.0, nx - 1 + 28.4, ny - 1 + 28.2])
    far_ps, near_ps = [0.0, 26.0, -50.3, ny * 0.45 - 0.2], [0.0, 12.0, -10.3, ny * 0.4 + 0.2]
    return [('sersic-off-corner', 'lanczos3', np.concatenate([far_ps, faint, bright, dark])),
            ('ps-off-lanczos', 'lanczos3', np.concatenate([near_ps, faint, dark, dark])),
            ('ps-off-bilinear', 'bilinear', np.concatenate([near_ps, faint, dark, dark]))]


def longdouble_loglike(field, raw, psf_index):
    """(weight map, log-likelihood, sum of the magnitudes of its terms) of a raw model with BOTH convolutions in
    numpy `longdouble` (`longdouble_weight_map` and models.py:213-236 in the same arithmetic)."""
    ld = np.longdouble
    ivm = longdouble_weight_map(field, raw, psf_index)
    k = int(np.rint(psf_index))
    kernel = np.fft.irfft2(np.asarray(field.psf_spec[k]).astype(np.clongdouble), s=raw.shape)
    spec = np.fft.rfft2(kernel.astype(ld))
    conv = np.fft.ifftshift(np.fft.irfft2(np.fft.rfft2(np.asarray(raw, dtype=ld)) * spec, s=raw.shape))
    good = ~field.bad_px
    with np.errstate(all='ignore'):
        chi = (np.asarray(field.sci, dtype=ld) - conv)[good] ** 2 * ivm[good]
        norm = np.log(ld(0.5) / ld(np.pi) * ivm[good])
    return ivm, -0.5 * (np.sum(chi) - np.sum(norm)), 0.5 * float(np.abs(chi).sum() + np.abs(norm).sum())
