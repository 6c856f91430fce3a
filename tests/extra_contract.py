"""The contract of the extra-image models (pixel-integrated Sersic, boxy / disky isophotes, azimuthal Fourier modes,
tilted sky, spiral arms, the radial laws `Moffat` and `Ferrer`) on ANY field:
`test_gpu_general_components.contract_raw` / `contract_evaluate` generalised to a
`test_gpu_random.random_case`-style field -- several PSFs with a free index, a mask, NaN `sci` pixels, non-positive
and NaN `ivm` pixels -- plus the fields, models and vectors the tests of these models on such fields share
(tests/test_extra_image_contract.py pins this module on the CPU, tests/test_gpu_extra_image_fields.py and
tests/test_gpu_law_fields.py hold the kernels to it).

The raw model comes from the components' own numpy definitions (`Sky.add_to_array`, `Sersic.add_to_array`) and the
oracle's point source; it is convolved with the spectra of the walker's PSF, k = rint(PSF_Index), and the likelihood
is taken over `~field.bad_px`.  An index outside [0, n_psf) is -inf before anything is evaluated
(`helpers.oracle_loglike`)."""
import functools

import numpy as np

import psfmc_oracle as orc
from psfmc_amd import MultiComponentModel
from psfmc_amd.ModelComponents import Configuration, Ferrer, Moffat, PointSource, Sersic, Sky
from psfmc_amd.ModelComponents.PSFSelector import PSFSelector
from psfmc_amd.distributions import Normal, Uniform

MAG_ZP = 25.0
PSF_SHAPE = (15, 13)
FREE = object()
ABSENT = object()
KEYWORDS = ('integrate', 'boxiness', 'fourier', 'spiral', 'law', 'fixed', 'truncation', 'bending')
THREE = {1: (FREE, FREE), 3: (FREE, 25.0), 4: (FREE, FREE)}          # one constant phase among free ones
MODES_1_4 = {1: (FREE, FREE), 4: (FREE, FREE)}

# the spiral of the kinds below: r_out and the winding free, the rest constants (angles in degrees)
ARMS = dict(r_in=2.0, r_out=FREE, winding=FREE, inclination=35.0, sky_angle=20.0)
LAWS = {'moffat': Moffat, 'ferrer': Ferrer}

# the model kinds: per Sersic its keywords, and the sky's slope.  I, G, F, M: the extra-image keywords; S, R, X: a
# spiral, the two radial laws, and everything in one model
KINDS = {
    'I': dict(sersics=[dict(integrate=True), {}], slope=ABSENT),
    'G': dict(sersics=[dict(boxiness=FREE), {}], slope=FREE),
    'F': dict(sersics=[dict(boxiness=FREE, fourier=THREE), {}], slope=ABSENT),
    'M': dict(sersics=[dict(boxiness=FREE, fourier=MODES_1_4), dict(integrate=True), {}], slope=FREE),
    'S': dict(sersics=[dict(boxiness=FREE, spiral=ARMS), {}], slope=ABSENT),
    'R': dict(sersics=[dict(law='moffat', boxiness=FREE), dict(law='ferrer', boxiness=FREE)], slope=FREE),
    'X': dict(sersics=[dict(law='ferrer', boxiness=FREE, spiral=ARMS, fourier=MODES_1_4), dict(integrate=True),
                       dict(law='moffat')], slope=FREE),
}
LAW_KINDS = ('S', 'R', 'X')


def moved(kind):
    """The kind with every Sersic's keywords -- `spiral` and `law` among them -- moved to the next one (what a wrong
    flag row would evaluate)."""
    spec = KINDS[kind] if isinstance(kind, str) else kind
    s = spec['sersics']
    return dict(spec, sersics=[dict(s[k - 1]) for k in range(len(s))])


# -- fields ----------------------------------------------------------------------------------------------------
def field_case(shape, seed, n_psf=2, psf_shape=PSF_SHAPE, box_at=None):
    """`random_case`'s field of this shape and seed with n_psf PSFs forced as `test_gpu_random.edge_case` makes them
    (each wider than the one before), the zeropoint fixed, and the features the tests claim PLANTED where the draw
    did not bring them: a mask, a NaN `sci` pixel, a zero, a negative and a NaN `ivm` pixel; with `box_at` = (x, y)
    one NaN `sci` and one zero `ivm` pixel inside the 7x7 box around floor((x, y) + 1/2)."""
    import test_gpu_random as tgr
    ny, nx = shape
    case = tgr.random_case(seed, shape)
    rng = np.random.RandomState(seed + 1)
    py, px = psf_shape
    yy, xx = np.mgrid[0:py, 0:px].astype(float)
    case['psfs'], case['pivms'] = [], []
    for k in range(n_psf):
        core = (1 + ((xx - px // 2) ** 2 + (yy - py // 2 + 0.1) ** 2) / (2.0 + 0.6 * k) ** 2) ** -2.5 * 300
        var = 0.01 + core / 40.0
        case['psfs'].append((core + rng.normal(size=core.shape) * np.sqrt(var)).astype(np.float32))
        case['pivms'].append((1.0 / var).astype(np.float32))
    case['zp'] = MAG_ZP
    case['shape'] = (ny, nx)
    for key in ('comps', 'psf_index'):
        case.pop(key, None)
    sci, ivm = case['sci'], case['ivm']
    if case['mask'] is None:
        case['mask'] = np.zeros((ny, nx), dtype=np.uint8)
        case['mask'][ny // 3:ny // 3 + 3, nx // 4:nx // 4 + 4] = 1
    sci[ny - 5, 3] = np.nan
    ivm[4, nx - 7], ivm[ny // 2 + 9, 5], ivm[ny - 3, nx // 2] = 0.0, -1.0, np.nan
    if box_at is not None:
        bx, by = int(np.floor(box_at[0] + 0.5)), int(np.floor(box_at[1] + 0.5))
        sci[min(max(by - 1, 0), ny - 1), min(max(bx + 2, 0), nx - 1)] = np.nan
        ivm[min(max(by + 2, 0), ny - 1), min(max(bx - 1, 0), nx - 1)] = 0.0
    return case


def oracle_field(case):
    return orc.make_field(case['sci'], case['ivm'], case['psfs'], case['pivms'], mask=case['mask'], mag_zp=case['zp'])


def field_features(case, field, box_at=None):
    """What a case claims about its field, asserted: a mask, >= 1 NaN `sci` pixel, >= 1 non-positive or NaN `ivm`
    pixel, and with `box_at` >= 1 bad pixel within the 7x7 box of the integrated component."""
    ny, nx = case['shape']
    assert case['mask'] is not None and np.any(case['mask']) and not np.all(case['mask'])
    assert np.isnan(case['sci']).sum() >= 1
    with np.errstate(invalid='ignore'):
        assert (np.isnan(case['ivm']) | (case['ivm'] <= 0)).sum() >= 1
    assert np.all(field.bad_px[np.isnan(case['sci'])]) and np.all(field.bad_px[case['mask'] != 0])
    assert 0 < field.bad_px.sum() < field.bad_px.size // 4
    if box_at is not None:
        bx, by = int(np.floor(box_at[0] + 0.5)), int(np.floor(box_at[1] + 0.5))
        box = field.bad_px[max(by - 3, 0):min(by + 4, ny), max(bx - 3, 0):min(bx + 4, nx)]
        assert box.size and box.any(), 'no bad pixel in the 7x7 box of the integrated component'


# -- models ----------------------------------------------------------------------------------------------------
def make_model(case, sersics, slope=ABSENT, backend='fused', max_walkers=8, lean=False, extent=None):
    """Configuration (the case's PSFs, mask and zeropoint) + Sky (`slope`: FREE, two values or ABSENT) + PointSource +
    one Sersic per entry of `sersics`, a dict with any of `integrate`, `boxiness` (FREE or a value), `fourier`
    ({m: (amplitude, phase)}, FREE or values), `spiral` ({key: FREE or a value}, `Sersic`'s keys), `truncation`
    ({side: (lo, hi)}, FREE or values), `bending` ({m: a_m}, FREE or values) and `law`: 'moffat'
    or 'ferrer' -- a `Moffat` / `Ferrer` with its own argument names in the Sersic's place -- or (law, {argument: a
    constant}) for constants among the law's own arguments; `fixed`: {argument: a constant} among a plain Sersic's
    own (`xy`, `mag`, `reff`, `reff_b`, `index`).  FREE: the test's prior, a fresh object per model; those of
    the spiral's and the laws' arguments are tests/test_gpu_radial_laws.py build's, wider than the support.
    `PSF_Index` is free (and last) when the case has several PSFs.  lean: the point source's position, the Sersics'
    angle and every boxiness given as FREE are constants (a 24-walker ensemble is allowed with one Sersic).  extent:
    the image side the priors of the laws' radii are scaled to (joint fits: shared priors are equal)."""
    ny, nx = case['shape']
    big = 4.0 * (extent or max(ny, nx))
    c = np.array((nx / 2 + 0.5, ny / 2 + 0.5))
    wide = lambda: Uniform(loc=c - 2.0 * max(ny, nx), scale=4.0 * max(ny, nx) * np.ones(2))
    psfs, pivms = case['psfs'], case['pivms']
    comps = [Configuration(case['sci'], case['ivm'], psfs if len(psfs) > 1 else psfs[0],
                           pivms if len(pivms) > 1 else pivms[0], mask_file=case['mask'], mag_zeropoint=case['zp'])]
    sky_kw = {}
    if slope is not ABSENT:
        sky_kw['slope'] = Normal(loc=(0, 0), scale=(1e-3, 1e-3)) if slope is FREE else slope
    comps.append(Sky(adu=Normal(loc=0.0, scale=0.1), **sky_kw))
    comps.append(PointSource(xy=(nx / 2 + 1.3, ny / 2 - 0.8) if lean else wide(), mag=Uniform(loc=16.0, scale=8.0)))
    for spec in sersics:
        assert set(spec) <= set(KEYWORDS), spec
        kw = {}
        if spec.get('integrate'):
            kw['integrate'] = True
        if 'boxiness' in spec:
            box = spec['boxiness']
            kw['boxiness'] = (0.6 if lean else Uniform(loc=-1.5, scale=4.0)) if box is FREE else box
        if 'fourier' in spec:
            kw['fourier'] = {m: (Uniform(loc=-1.0, scale=2.0) if a is FREE else a,
                                 Uniform(loc=-720.0, scale=1440.0) if p is FREE else p)
                             for m, (a, p) in spec['fourier'].items()}
        if 'spiral' in spec:
            kw['spiral'] = {k: (Uniform(loc=-720.0, scale=1440.0) if k == 'winding' else Uniform(loc=-5.0, scale=205.0))
                            if v is FREE else v for k, v in spec['spiral'].items()}
        if 'truncation' in spec:
            kw['truncation'] = {k: tuple(Uniform(loc=-5.0, scale=95.0) if v is FREE else v for v in pair)
                                for k, pair in spec['truncation'].items()}
        if 'bending' in spec:
            kw['bending'] = {m: Uniform(loc=-3.0, scale=6.0) if a is FREE else a for m, a in spec['bending'].items()}
        kw.update(xy=wide(), mag=Uniform(loc=15.0, scale=10.0), angle=30.0 if lean else Uniform(loc=-360, scale=720),
                  angle_degrees=True)
        if 'law' in spec:
            assert 'fixed' not in spec, spec                             # (a law's constants come with the law)
            law, consts = (spec['law'], {}) if isinstance(spec['law'], str) else spec['law']
            radius = lambda: Uniform(loc=0.5, scale=big - 0.5)
            if law == 'moffat':
                kw.update(fwhm=radius(), fwhm_b=radius(), beta=Uniform(loc=-4.0, scale=13.0))
            else:
                kw.update(r_out=radius(), r_out_b=radius(), alpha=Uniform(loc=-1.0, scale=8.0),
                          beta=Uniform(loc=-4.0, scale=13.0))
            assert set(consts) <= set(kw), consts
            kw.update(consts)
            comps.append(LAWS[law](**kw))
            continue
        kw.update(reff=Uniform(loc=0.5, scale=40.0), reff_b=Uniform(loc=0.5, scale=40.0), index=Uniform(loc=0.2, scale=8.0))
        assert set(spec.get('fixed', {})) <= {'xy', 'mag', 'reff', 'reff_b', 'index'}, spec
        kw.update(spec.get('fixed', {}))
        comps.append(Sersic(**kw))
    return MultiComponentModel(comps, backend=backend, max_walkers=max_walkers)


def theta_of(model, sky, ps, sersics, psf=0.0):
    """One parameter vector from values BY NAME (whatever the model's packing order): `sky`, `ps` and each of `sersics`
    map a component's attribute names (`adu`, `slope`, `mag`, `xy`, `angle`, `boxiness`, `f1_amp`, ...) to values;
    entries of attributes that are constants in this model, or absent from it, are ignored.  A `Moffat` or `Ferrer`
    takes a Sersic's entry (it is one); its `alpha` / `beta` are the entry's `moffat_beta`, `ferrer_alpha`,
    `ferrer_beta` (the two laws' `beta` mean different things)."""
    groups = {Sky: [sky], PointSource: [ps], Sersic: list(sersics), PSFSelector: [dict(psf_index=psf)]}
    seen = {k: 0 for k in groups}
    out = []
    for comp in model.components:
        group = Sersic if isinstance(comp, Sersic) else type(comp)
        vals = groups[group][seen[group]]
        seen[group] += 1
        law = getattr(comp, 'radial_law', None)
        for name, width in zip(comp.free_names(), comp.stochastic_lens()):
            v = np.ravel(np.asarray(vals['%s_%s' % (law, name) if law and name in comp.LAW_ATTRS else name],
                                    dtype=np.float64))
            assert v.size == width, (type(comp).__name__, name)
            out.extend(v)
    assert len(out) == model.num_params
    return np.array(out, dtype=np.float64)


def psf_index_of(model, theta):
    """The walker's PSF_Index as given (not rounded); 0 for a model with one PSF."""
    return float(theta[-1]) if model.param_names and model.param_names[-1] == 'PSF_Index' else 0.0


# -- the contract ----------------------------------------------------------------------------------------------
def contract_raw(model, theta, only_ps=False):
    """Raw model of one vector: the components' own host definitions (`add_to_array`) and the oracle's point source."""
    model.param_values = np.asarray(theta, dtype=np.float64)
    shape = model.config.obs_data.shape
    raw = np.zeros(shape)
    coords = orc.array_coords(shape)
    for comp in model.components:
        if isinstance(comp, PointSource):
            orc.add_point_source(raw, np.ravel(comp.xy), float(np.ravel(comp.mag)[0]), model.config.mag_zeropoint, coords,
                                 comp.shift_method)
        elif isinstance(comp, (Sky, Sersic)) and not only_ps:
            comp.add_to_array(raw, model.config.mag_zeropoint)
    return raw


def contract_evaluate(model, field, theta):
    """(log-likelihood, the five images) of one vector; (-inf, None) for a PSF index outside [0, n_psf)."""
    k = np.rint(psf_index_of(model, theta))
    if not 0 <= k < len(field.psf_spec):
        return -np.inf, None
    k = int(k)
    raw = contract_raw(model, theta)
    with np.errstate(all='ignore'):
        conv = orc.convolve(raw, field.psf_spec[k])
        resid = field.sci - conv
        ivm = 1 / (orc.convolve(raw ** 2, field.var_spec[k]) + field.obs_var)
        ps = contract_raw(model, theta, only_ps=True)
        images = {'raw_model': raw, 'convolved_model': conv, 'residual': resid, 'composite_ivm': ivm,
                  'point_source_subtracted': field.sci - orc.convolve(ps, field.psf_spec[k])}
        good = ~field.bad_px
        ll = -0.5 * np.sum(resid[good] ** 2 * ivm[good] - np.log(0.5 / np.pi * ivm[good]))
    return (ll if np.isfinite(ll) else -np.inf), images


def raw_error(got, want, tag):
    """Finite at every pixel (the bad ones included); relative error on every pixel above 1e-12 of the peak."""
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)), tag
    big = np.abs(want) > 1e-12 * np.abs(want).max()
    return float(np.max(np.abs(got[big] - want[big]) / np.abs(want[big])))


def rel(got, want):
    return abs(got - want) / abs(want)


# |1 - x| of every compared pixel of a Ferrer component is at least this (asserted on the host from the definition
# before the device is asked): 1 - x cancels at the edge, where a pixel's absolute error is alpha (1 - x)^(alpha - 1) dx;
# with dx ~ 1e-15 this stays below 1e-12 of Sigma_0 for alpha >= 0.5, and at alpha = 0 no pixel changes sides
EDGE_MARGIN = 1e-6


def ferrer_x(model, comp):
    """x = rho^(2 - beta) of a Ferrer component on the image's pixels at the model's current values (0 where
    u = v = 0): the law is Sigma_0 (1 - x)^alpha where x < 1 and exactly 0 elsewhere."""
    get = lambda k: getattr(comp, k)
    row = comp.derived_row(model.config.mag_zeropoint)
    box = float(np.ravel(comp.boxiness)[0]) if comp.has_boxiness else 0.0
    amps, phases = comp._fourier_values(get) if comp.has_fourier else ((), ())
    modes = list(zip(comp.fourier_modes, amps, phases))
    spiral = comp._spiral_values(get) if comp.has_spiral else None
    pars = comp._radial_values(get)
    rho2, centre = Sersic.radial_rho2(row, box, modes, spiral, model.config.obs_data.shape)
    with np.errstate(all='ignore'):
        x = np.where(centre, 0.0, rho2 ** (0.5 * (2.0 - pars[1])))
    return x, Sersic.radial_central('ferrer', row, pars, box, modes, spiral)


def ferrer_state(model):
    """(smallest Sigma_0, smallest |1 - x| over the image's pixels) of the model's Ferrer components at the model's
    current values, from the definition alone; (0, inf) without one."""
    sigma0, margin = [], np.inf
    for comp in model.components:
        if isinstance(comp, Ferrer):
            x, central = ferrer_x(model, comp)
            sigma0.append(central)
            margin = min(margin, float(np.min(np.abs(1.0 - x))))
    return (min(sigma0) if sigma0 else 0.0), margin


def law_error(got, want, sigma0, tag):
    """A Moffat, a Sersic, the sky and the point source relative to the pixel, a Ferrer relative to its Sigma_0: the
    absolute error over max(|pixel|, Sigma_0), on every pixel where that is above 1e-12 of the peak (`raw_error`'s
    pixels; with a Ferrer in the model no pixel is left out)."""
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)), tag
    scale = np.maximum(np.abs(want), sigma0)
    big = scale > 1e-12 * np.abs(want).max()
    assert sigma0 == 0.0 or np.all(big), tag
    err = float(np.max(np.abs(got - want)[big] / scale[big]))
    print('%s: raw model max error %.2e (Sigma_0 of the Ferrer %.3e)' % (tag, err, sigma0))
    return err


def has_ferrer(model):
    return any(isinstance(c, Ferrer) for c in model.components)


def contract_with_state(model, field, theta):
    """`contract_evaluate`'s (log-likelihood, images) and `ferrer_state`'s (Sigma_0, margin) of one vector."""
    out = contract_evaluate(model, field, theta)
    model.param_values = np.asarray(theta, dtype=np.float64)         # (an index outside the support evaluates nothing)
    return out + ferrer_state(model)


def judge_raw(model, got, want, sigma0, tag):
    """The raw model's error as the model is judged: by `law_error` where it has a Ferrer (whose value next to the
    cut-off is far below the peak and exactly 0 beyond it), else by `raw_error`."""
    return law_error(got, want, sigma0, tag) if has_ferrer(model) else raw_error(got, want, tag)


# -- the shared scene -------------------------------------------------------------------------------------------
def scene(shape, i=0):
    """(sky, ps, sersics) values of walker i on a (ny, nx) field, every keyword's value included (a model takes the
    ones it has): three Sersics about the field's centre, none on a pixel centre.  The magnitudes keep the raw model's
    peak near 20 counts (400 times the noise): the variance channel's rounding error grows with the SQUARED peak
    (tests/test_oracle_precision.py), and at a peak of 125 counts two fp64 evaluations of the same plain model whose
    raw images differ by one ulp (`Sersic.reference_image` against the oracle's `add_sersic`) already sit 3e-13 of
    the largest weight apart -- above the 1e-13 this module is pinned to the oracle with."""
    ny, nx = shape
    cx, cy = nx // 2, ny // 2
    d = 0.137 * i
    sky = dict(adu=0.02 + 0.003 * i, slope=(0.02 / nx * (1 - i % 3), 0.02 / ny * (0.5 - 0.25 * i)))
    ps = dict(mag=21.5 + 0.1 * i, xy=(nx / 2 + 1.3 + d, ny / 2 - 0.8 - d))
    four = dict(f1_amp=0.2 - 0.03 * i, f1_phase=30.0 + 20 * i, f3_amp=-0.15 + 0.02 * i, f4_amp=0.1 + 0.02 * i,
                f4_phase=-100.0 + 35 * i)
    sersics = [dict(angle=30.0 + 12 * i, index=1.5 + 0.2 * i, mag=20.4 + 0.1 * i, reff=6.0 - 0.3 * i, reff_b=4.0 - 0.2 * i,
                    xy=(cx - 6.36 + d, cy + 3.31 - d), boxiness=0.7 - 0.3 * i, **four),
               dict(angle=100.0 - 9 * i, index=2.5 - 0.2 * i, mag=20.9 - 0.1 * i, reff=4.0 + 0.2 * i, reff_b=2.5 + 0.1 * i,
                    xy=(cx + 5.27 - d, cy - 2.64 + d), boxiness=-0.5 + 0.2 * i,
                    **{k: -0.5 * v if k.endswith('amp') else v + 45.0 for k, v in four.items()}),
               dict(angle=-20.0 + 7 * i, index=1.0 + 0.1 * i, mag=21.3, reff=5.0, reff_b=4.5 - 0.2 * i,
                    xy=(cx + 1.62 + d, cy + 8.41), boxiness=1.2 - 0.1 * i,
                    **{k: 0.5 * v if k.endswith('amp') else v - 70.0 for k, v in four.items()})]
    # the spiral's and the radial laws' values (further names only: the ones above are what they always were).  The
    # laws' radii stay well inside the shortest image (64 rows) so that a Ferrer's rho = 1 contour lies inside it, and
    # with a Moffat or a Ferrer of these widths at the Sersics' magnitudes the peak stays at 20 counts (S, R and X
    # at every shape: 19.9 ... 20.0 for walker 0, 15.5 for walker 3; tests/test_extra_image_contract.py prints it)
    for k, s in enumerate(sersics):
        g = (1.0, -0.6, 0.8)[k]
        s.update(spiral_r_in=2.0 + 0.3 * k + 0.1 * i, spiral_r_out=9.0 + k + 0.5 * i, spiral_wind=g * (150.0 - 40.0 * i),
                 spiral_alpha=0.5 * k + 0.1 * i, spiral_incl=g * (35.0 - 3.0 * i), spiral_sky=20.0 - 30.0 * k + 5.0 * i,
                 fwhm=5.0 + 0.5 * k + 0.2 * i, fwhm_b=3.5 - 0.4 * k + 0.1 * i, moffat_beta=2.5 - 0.6 * k + 0.3 * i,
                 r_out=13.0 - 1.5 * k + 0.7 * i, r_out_b=7.0 - 0.5 * k + 0.3 * i, ferrer_alpha=0.5 + 0.25 * k + 0.5 * i,
                 ferrer_beta=1.2 - 0.3 * k - 0.4 * i)
    return sky, ps, sersics


def integrated_centre(kind, shape):
    """Centre (walker 0) of the kind's first integrated Sersic, or None."""
    flags = [bool(s.get('integrate')) for s in KINDS[kind]['sersics']]
    return tuple(scene(shape)[2][flags.index(True)]['xy']) if any(flags) else None


# The six PSF_Index values of the several-PSF batches: every PSF, 0.4 and 1.5 (rint: 0 and -- round-half-even -- 2, a
# PSF of three and outside the support of two), and one index outside the support
def psf_indices(n_psf):
    return [0.0, 1.0, 0.4, 1.5, 2.0, 3.0] if n_psf == 3 else [0.0, 1.0, 0.4, 1.5, 0.6, -1.0]


# (shape, number of PSFs) of the fused cases; the hipFFT cases are two of them
FUSED_SHAPES = [((64, 128), 2), ((128, 64), 3), ((70, 96), 2), ((96, 70), 3), ((96, 150), 2), ((64, 320), 2),
                ((64, 1152), 2)]
HIPFFT_CASES = [('M', (64, 128)), ('F', (64, 128)), ('M', (70, 96)), ('F', (70, 96))]
N_PSF = dict(FUSED_SHAPES)
CASES = [('fused', kind, shape) for shape, _ in FUSED_SHAPES for kind in 'IGFM'] + \
        [('hipfft', kind, shape) for kind, shape in HIPFFT_CASES]


# the spiral and radial-law kinds: every fused shape, and hipFFT's rectangular shapes
LAW_HIPFFT_CASES = [('X', (64, 128)), ('R', (64, 128)), ('X', (70, 96)), ('S', (70, 96))]
LAW_CASES = [('fused', kind, shape) for shape, _ in FUSED_SHAPES for kind in LAW_KINDS] + \
            [('hipfft', kind, shape) for kind, shape in LAW_HIPFFT_CASES]


def ferrer_centre(kind, shape):
    """Centre (walker 0) of the kind's first Ferrer, or None."""
    laws = [s.get('law') == 'ferrer' for s in KINDS[kind]['sersics']]
    return tuple(scene(shape)[2][laws.index(True)]['xy']) if any(laws) else None


def case_id(v):
    return '%dx%d' % v if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def several_psf_case(kind, shape):
    """(case, oracle field) of one (kind, shape): the field's seed is the shape's, the planted box pixels the kind's."""
    case = field_case(shape, 500 + 7 * shape[0] + shape[1], N_PSF[shape], box_at=integrated_centre(kind, shape))
    return case, oracle_field(case)


@functools.lru_cache(maxsize=None)
def law_case(kind, shape):
    """(case, oracle field) of one (kind, shape) of `LAW_CASES`: `several_psf_case`'s field, and for a kind with a
    Ferrer one NaN `sci` and one zero `ivm` pixel planted a few pixels from its centre -- inside its support, while
    the ones `field_case` plants near the image's corners lie outside."""
    case = field_case(shape, 500 + 7 * shape[0] + shape[1], N_PSF[shape], box_at=integrated_centre(kind, shape))
    at = ferrer_centre(kind, shape)
    if at is not None:
        fx, fy = int(np.floor(at[0] + 0.5)), int(np.floor(at[1] + 0.5))
        case['sci'][fy - 2, fx + 3] = np.nan
        case['ivm'][fy + 3, fx - 2] = 0.0
    return case, oracle_field(case)


def several_psf_thetas(model, shape):
    """The six distinct walkers of a (kind, shape) case for this model, PSF_Index (where free) as `psf_indices`."""
    n_psf = len(model.config.psf_selector.psf_data)
    return np.array([theta_of(model, *scene(shape, i), psf=p) for i, p in enumerate(psf_indices(n_psf))])
