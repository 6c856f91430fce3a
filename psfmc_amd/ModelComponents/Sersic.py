import numpy as np
from scipy.special import gamma, gammaincinv, gammaln

from .ComponentBase import ComponentBase, StochasticProperty


# Constants of the pixel-integrated profile (`integrate=True`); fixed per build, the same on the device
# (csrc/psfmc_integrated.h).  DESIGN.md section "Pixel-integrated Sersic profile" says how they were chosen.
INTEG_HALF_BOX = 3        # H: midpoint grids in the (2H+1)^2 pixels around the pixel nearest the centre
INTEG_GRID_NEAR = 8       # s x s samples per pixel at Chebyshev distance <= INTEG_NEAR_RING ...
INTEG_NEAR_RING = 1
INTEG_GRID_FAR = 4        # ... and further out in the box
INTEG_SPLIT = 4           # s0: a cell that holds the centre is split s0 x s0
INTEG_LEVELS = 8          # L: the sub-cell(s) holding the centre are split again, L times
INTEG_SUB = 4             # midpoint grid of every sub-cell that is not split (even: see integrated_image)
# The pixel-averaged mode of the general components (`pixel_mean=True`, `Sersic.general_mean_image`) uses the
# constants above unchanged and one of its own; the same on the device (csrc/psfmc_general_mean.h).
MEAN_EDGE_GRID = 8        # midpoint grid of a Ferrer pixel that the truncation edge crosses


class Sersic(ComponentBase):
    """Elliptical Sersic profile (reference: ModelComponents/Sersic.py:16-45).
    `reff` / `reff_b` are the semi-major / semi-minor effective radii, `angle`
    the position angle (CCW of up; radians unless `angle_degrees`).

    The default profile is the reference's: the profile at the pixel centre times a one-dimensional
    centroid correction, which is NaN in the pixel whose centre is the component's centre (0/0), so that
    such a walker's log-posterior is -inf.  `integrate=True` asks for the PIXEL-INTEGRATED profile instead
    (`Sersic.integrated_image`; not the reference's): finite everywhere, an on-pixel centre included, and
    several times closer to GALFIT's rendering in the core.

    `boxiness=c` (a number or a prior; GALFIT's C0, not the reference's) generalises the isophotes to
    superellipses |u|^(c+2) + |v|^(c+2) = const: boxy for c > 0, disky for c < 0, the plain ellipse at c = 0
    (`Sersic.general_image`); `mag` stays the total magnitude.  c <= -2 or a non-finite c is outside the support
    (log-prior -inf, like reff_b > reff).  None (the default) means absent: the component, its parameters and its
    kernels are the plain profile's.  `boxiness` together with `integrate=True` is out of scope (the
    pixel-integrated profile's second-order term and core refinement are derived for ellipses) and raises
    ValueError.

    `fourier={m: (amplitude, phase), ...}` (numbers or priors, m in 1 ... 6; GALFIT's F1 ... F6, not the reference's)
    bends the isophote radius by azimuthal modes, r = r0 (1 + sum_m a_m cos(m (theta + phi_m)))
    (`Sersic.fourier_image`): m = 1 is lopsidedness, m = 3 and above pick up tails and arms; `mag` stays the total
    magnitude.  The parameters are the attributes `f<m>_amp` and `f<m>_phase` (the phase in radians, or in degrees with
    `angle_degrees`).  Amplitudes and phases must be finite and sum_m |a_m| < 1 (log-prior -inf otherwise).  A
    component with `fourier` but without `boxiness` has c = 0; `fourier` with `integrate=True` raises ValueError.

    `spiral={'r_in': .., 'r_out': .., 'winding': .., 'alpha': .., 'inclination': .., 'sky_angle': ..}` (numbers or
    priors; the first three keys are required, the others are fixed at 0.0 when absent; GALFIT-style coordinate
    rotation, not GALFIT's formula and not the reference's) winds the component's coordinates in a disk plane that is
    inclined to the sky, so that a bar turns into arms: the position angle grows by `winding` between `r_in` and
    `r_out` along a tanh ramp times the power law (r / r_out)^alpha (`Sersic.spiral_image`); `mag` stays the total
    magnitude.  The parameters are the attributes `spiral_r_in`, `spiral_r_out`, `spiral_wind`, `spiral_alpha`,
    `spiral_incl`, `spiral_sky` (the three angles in radians, or in degrees with `angle_degrees`).  Support: all six
    finite, r_in >= 0, r_out > r_in, alpha >= 0, |inclination| < pi/2 (log-prior -inf otherwise).  A component with
    `spiral` alone is a general one with c = 0 and no modes; `spiral` with `integrate=True` raises ValueError.

    `pixel_mean=True` (only together with `boxiness`, `fourier` or `spiral`; not the reference's) renders the general
    component as the MEAN OF ITS LAW OVER EACH PIXEL instead of the law at the pixel centre times the centroid term
    (`Sersic.general_mean_image`): finite where the centre is a pixel centre, and several times to a hundred times
    closer to the true pixel mean in the core.  It adds no parameter.  On a plain Sersic it raises ValueError (use
    `integrate=True` there), and so does `pixel_mean=True` together with `integrate=True`.

    `truncation={'inner': (lo, hi), 'outer': (lo, hi)}` (either key or both; numbers or priors; GALFIT's truncation
    function in spirit, not its parametrisation and not the reference's) multiplies the component by a tanh ramp that
    rises from 0.018 at `lo` to 0.982 at `hi` (inner) and by one that falls from 0.982 at `lo` to 0.018 at `hi` (outer),
    radii in pixels ALONG THE COMPONENT'S MAJOR AXIS (`Sersic.truncation_weight`, `Sersic.truncated_image`): a ring, a
    lens, a disc or a pair of arms that starts outside the bar, a disc that stops.  The truncation follows the
    component's own isophotes -- boxy, bent by the modes and wound with them; it has no centre or axis ratio of its
    own.  The parameters are the attributes `trunc_in_lo`, `trunc_in_hi`, `trunc_out_lo`, `trunc_out_hi`.  Support:
    the values of a side finite with 0 <= lo < hi (log-prior -inf otherwise); the two sides may overlap.  `mag` is the
    total magnitude of the UNTRUNCATED component (GALFIT's flux parameter of a truncated component is not its total
    either); `Sersic.truncation_flux_fraction` gives the fraction of it that survives.  The ramps are soft by
    construction, so `pixel_mean=True` averages the product with its scheme unchanged and adds no refinement at the
    radii.  A component with `truncation` alone is a general one with c = 0 and no modes; `truncation` with
    `integrate=True` raises ValueError (use `pixel_mean=True`).

    `bending={m: a_m, ...}` (m = 1 ... 4; numbers or priors; GALFIT's bending modes, not the reference's) displaces the
    component's ridge across its major axis by a polynomial of the coordinate along it (`Sersic.bend`,
    `Sersic.bent_image`): with (u, v) the coordinates in units of the semi-major and semi-minor radius r_a, r_b (after
    the spiral's winding where there is one), v' = v + (r_a / r_b) sum_m a_m u^m, and everything downstream reads
    (u, v') -- in pixels along and across the major axis y' = y + r_a sum_m a_m (x / r_a)^m, so that the ridge lies at
    Y = -r_a sum_m a_m (X / r_a)^m: a banana (m = 2), an S-shaped tidal pair (m = 3), a sheared envelope (m = 1).  The
    parameters are the attributes `bend1` ... `bend4`; an absent mode is the constant 0 and adds none.  The shear has
    unit Jacobian and f(0) = 0, so `mag` stays the total magnitude and the centre the centre; boxiness, modes, spiral,
    radial law and truncation act on the bent coordinates.  Support: every amplitude finite (log-prior -inf otherwise);
    the shear is a bijection for any value.  m = 1 on a plain ellipse is another ellipse -- degenerate with `angle` and
    the axis ratio; it is allowed, not refused (fix it or give it a narrow prior).  `pixel_mean=True` averages the bent
    law with its scheme unchanged.  A component with `bending` alone is a general one with c = 0; `bending` with
    `integrate=True` raises ValueError (use `pixel_mean=True`)."""
    device_kind = 'sersic'
    # the radial law: None for the Sersic law, else a key of RADIAL_KINDS (the subclasses `Moffat` and `Ferrer`)
    radial_law = None
    RADIAL_KINDS = {None: 0, 'moffat': 1, 'ferrer': 2}      # psfmc_set_radial_layout's kind bytes
    RADIAL_PARAMS = 2                                       # entries per Sersic slot: (beta, unused) or (alpha, beta)
    # the attributes behind the slots angle, index, mag, reff, reff_b of psfmc_set_layout (a subclass renames the radii)
    SLOT_ATTRS = ('angle', 'index', 'mag', 'reff', 'reff_b')
    FOURIER_MODES = (1, 2, 3, 4, 5, 6)
    FOURIER_POINTS = 128      # midpoint rule of the area ratio Q (`fourier_area_ratio`); fixed, the same on the device
    # the keys of `spiral` in the order of psfmc_set_spiral_layout's entries, their attributes and FITS abbreviations
    SPIRAL_KEYS = ('r_in', 'r_out', 'winding', 'alpha', 'inclination', 'sky_angle')
    SPIRAL_REQUIRED = ('r_in', 'r_out', 'winding')
    SPIRAL_ATTRS = ('spiral_r_in', 'spiral_r_out', 'spiral_wind', 'spiral_alpha', 'spiral_incl', 'spiral_sky')
    SPIRAL_ANGLES = ('spiral_wind', 'spiral_incl', 'spiral_sky')
    # the sides of `truncation` (psfmc_set_truncation_layout's flag bits 0 and 1) and the attributes in the order of
    # its entries; TRUNC_ABSENT: what an absent side's entries hold (inside the support, never read)
    TRUNC_KEYS = ('inner', 'outer')
    TRUNC_ATTRS = ('trunc_in_lo', 'trunc_in_hi', 'trunc_out_lo', 'trunc_out_hi')
    TRUNC_PARAMS = 4
    TRUNC_ABSENT = (0.0, 1.0, 0.0, 1.0)
    # the modes of `bending` (psfmc_set_bending_layout's mask bit m - 1; PSFMC_BEND_MODES) and their attributes
    BEND_MODES = (1, 2, 3, 4)
    BEND_ATTRS = tuple('bend%d' % m for m in BEND_MODES)
    _fits_abbrs = ([('trunc_in_lo', 'TIL'), ('trunc_in_hi', 'TIH'), ('trunc_out_lo', 'TOL'), ('trunc_out_hi', 'TOH'),
                    ('Sersic', 'SER'), ('spiral_r_in', 'SRI'), ('spiral_r_out', 'SRO'), ('spiral_wind', 'SWD'),
                    ('spiral_alpha', 'SAL'), ('spiral_incl', 'SIN'), ('spiral_sky', 'SPA'),
                    ('reff_b', 'REB'), ('reff', 'RE'),
                    ('index', 'N'), ('angle', 'ANG'), ('boxiness', 'BOX')] +
                   [('f%d_amp' % m, 'F%dA' % m) for m in FOURIER_MODES] +
                   [('f%d_phase' % m, 'F%dP' % m) for m in FOURIER_MODES] +
                   [('bend%d' % m, 'BD%d' % m) for m in BEND_MODES])

    xy = StochasticProperty()
    mag = StochasticProperty()
    reff = StochasticProperty()
    reff_b = StochasticProperty()
    index = StochasticProperty()
    angle = StochasticProperty()
    boxiness = StochasticProperty()
    f1_amp = StochasticProperty()
    f1_phase = StochasticProperty()
    f2_amp = StochasticProperty()
    f2_phase = StochasticProperty()
    f3_amp = StochasticProperty()
    f3_phase = StochasticProperty()
    f4_amp = StochasticProperty()
    f4_phase = StochasticProperty()
    f5_amp = StochasticProperty()
    f5_phase = StochasticProperty()
    f6_amp = StochasticProperty()
    f6_phase = StochasticProperty()
    spiral_r_in = StochasticProperty()
    spiral_r_out = StochasticProperty()
    spiral_wind = StochasticProperty()
    spiral_alpha = StochasticProperty()
    spiral_incl = StochasticProperty()
    spiral_sky = StochasticProperty()
    trunc_in_lo = StochasticProperty()
    trunc_in_hi = StochasticProperty()
    trunc_out_lo = StochasticProperty()
    trunc_out_hi = StochasticProperty()
    bend1 = StochasticProperty()
    bend2 = StochasticProperty()
    bend3 = StochasticProperty()
    bend4 = StochasticProperty()

    def __init__(self, xy=None, mag=None, reff=None, reff_b=None, index=None,
                 angle=None, angle_degrees=False, integrate=False, boxiness=None, fourier=None, spiral=None,
                 pixel_mean=False, truncation=None, bending=None):
        super(Sersic, self).__init__()
        self.xy = xy
        self.mag = mag
        self.reff = reff
        self.reff_b = reff_b
        self.index = index
        self.angle = angle
        self.angle_degrees = angle_degrees
        self.integrate = bool(integrate)
        self._init_shape(boxiness, fourier, spiral, pixel_mean, truncation, bending)

    def _init_shape(self, boxiness, fourier, spiral, pixel_mean=False, truncation=None, bending=None):
        """The isophote-shape keywords `boxiness`, `fourier` and `spiral`, the rendering keyword `pixel_mean`,
        `truncation` and `bending` (shared with the radial-law subclasses)."""
        self.pixel_mean = bool(pixel_mean)
        if self.pixel_mean and self.integrate:
            raise ValueError('Sersic: pixel_mean=True together with integrate=True is not supported (integrate=True '
                             'is the plain profile\'s pixel integral, pixel_mean=True a general component\'s)')
        self.truncation_sides = ()
        if truncation is not None:
            if self.integrate:
                raise ValueError('Sersic: truncation together with integrate=True is not supported (the '
                                 'pixel-integrated profile is the plain component\'s; use pixel_mean=True)')
            truncation = dict(truncation)
            unknown = [k for k in truncation if k not in Sersic.TRUNC_KEYS]
            if unknown:
                raise ValueError('Sersic: truncation has no key {!r} (keys: {})'.format(
                    unknown[0], ', '.join(Sersic.TRUNC_KEYS)))
            if not truncation:
                raise ValueError('Sersic: truncation needs the key \'inner\' or \'outer\'')
            for side, key in enumerate(Sersic.TRUNC_KEYS):
                if key not in truncation:
                    continue
                entry = truncation[key]
                try:
                    if isinstance(entry, (str, bytes, dict)) or hasattr(entry, 'value'):
                        raise TypeError
                    lo, hi = entry
                except (TypeError, ValueError):
                    raise ValueError('Sersic: truncation {!r} needs a pair (lo, hi)'.format(key))
                setattr(self, Sersic.TRUNC_ATTRS[2 * side], lo)
                setattr(self, Sersic.TRUNC_ATTRS[2 * side + 1], hi)
            self.truncation_sides = tuple(k for k in Sersic.TRUNC_KEYS if k in truncation)
        self.has_truncation = bool(self.truncation_sides)
        self.bending_modes = ()
        if bending is not None:
            if self.integrate:
                raise ValueError('Sersic: bending together with integrate=True is not supported (the '
                                 'pixel-integrated profile is defined for elliptical isophotes; use pixel_mean=True)')
            modes = []
            # (a mapping, or pairs (m, a_m): pairs can name a mode twice)
            for m, amp in (bending.items() if hasattr(bending, 'items') else list(bending)):
                try:
                    whole = not isinstance(m, bool) and int(m) == m and int(m) in Sersic.BEND_MODES
                except (TypeError, ValueError):
                    whole = False
                if not whole:
                    raise ValueError('Sersic: bending mode numbers are integers in 1 ... 4, got {!r}'.format(m))
                if int(m) in modes:
                    raise ValueError('Sersic: bending mode {} given twice'.format(int(m)))
                modes.append(int(m))
                setattr(self, 'bend%d' % int(m), amp)
            self.bending_modes = tuple(sorted(modes))
        self.has_bending = bool(self.bending_modes)
        # (asked of what was parsed: an empty `bending` names no mode and makes no general component)
        if (self.pixel_mean and self.radial_law is None and boxiness is None and fourier is None and spiral is None
                and not self.has_truncation and not self.has_bending):
            raise ValueError('Sersic: pixel_mean=True needs boxiness, fourier or spiral; the plain profile has '
                             'integrate=True')
        self.has_boxiness = boxiness is not None
        if self.has_boxiness:
            if self.integrate:
                raise ValueError('Sersic: boxiness together with integrate=True is not supported (the '
                                 'pixel-integrated profile is defined for elliptical isophotes; use pixel_mean=True)')
            self.boxiness = boxiness
        self.fourier_modes = ()
        if fourier is not None:
            if self.integrate:
                raise ValueError('Sersic: fourier together with integrate=True is not supported (the '
                                 'pixel-integrated profile is defined for elliptical isophotes; use pixel_mean=True)')
            modes = []
            for m, entry in dict(fourier).items():
                if isinstance(m, bool) or int(m) != m or int(m) not in Sersic.FOURIER_MODES:
                    raise ValueError('Sersic: fourier mode numbers are integers in 1 ... 6, got {!r}'.format(m))
                try:
                    amp, phase = entry
                except (TypeError, ValueError):
                    raise ValueError('Sersic: fourier mode {} needs (amplitude, phase)'.format(m))
                if int(m) in modes:
                    raise ValueError('Sersic: fourier mode {} given twice'.format(int(m)))
                modes.append(int(m))
                setattr(self, 'f%d_amp' % int(m), amp)
                setattr(self, 'f%d_phase' % int(m), phase)
            self.fourier_modes = tuple(sorted(modes))
        self.has_fourier = bool(self.fourier_modes)
        self.has_spiral = spiral is not None
        if self.has_spiral:
            if self.integrate:
                raise ValueError('Sersic: spiral together with integrate=True is not supported (the '
                                 'pixel-integrated profile is defined for elliptical isophotes; use pixel_mean=True)')
            spiral = dict(spiral)
            unknown = [k for k in spiral if k not in Sersic.SPIRAL_KEYS]
            if unknown:
                raise ValueError('Sersic: spiral has no key {!r} (keys: {})'.format(
                    unknown[0], ', '.join(Sersic.SPIRAL_KEYS)))
            missing = [k for k in Sersic.SPIRAL_REQUIRED if k not in spiral]
            if missing:
                raise ValueError('Sersic: spiral needs the key {!r}'.format(missing[0]))
            for key, attr in zip(Sersic.SPIRAL_KEYS, Sersic.SPIRAL_ATTRS):
                setattr(self, attr, spiral.get(key, 0.0))

    @property
    def is_general(self):
        """Does the component run the general kernels (a `boxiness`, `fourier`, `spiral`, `truncation` or `bending`
        keyword)?"""
        return self.has_boxiness or self.has_fourier or self.has_spiral or self.has_truncation or self.has_bending

    @property
    def bending_mask(self):
        """psfmc_set_bending_layout's mask of the slot: bit m - 1 set where the component has bending mode m; 0: none."""
        return sum(1 << (m - 1) for m in self.bending_modes)

    @property
    def truncation_flags(self):
        """psfmc_set_truncation_layout's flag of the slot: bit 0 an inner, bit 1 an outer truncation; 0: none."""
        return sum(1 << Sersic.TRUNC_KEYS.index(k) for k in self.truncation_sides)

    def header_flags(self, count):
        """FITS header keys this component adds to a database beside its parameters' own: `<count>SERINT = T`
        when it is the pixel-integrated profile, `<count>SERBOX = T` when it has a boxiness, `<count>SERFOU` = the
        comma-separated mode numbers when it has Fourier modes, `<count>SERSPI = T` when it has a spiral,
        `<count>SERLAW = 'moffat' | 'ferrer'` when its radial law is not the Sersic law (`Moffat`, `Ferrer`),
        `<count>SERAVG = T` when it is rendered as the mean over each pixel (`pixel_mean=True`), `<count>SERTRU =
        'inner' | 'outer' | 'inner,outer'` when it is truncated, `<count>SERBND` = the comma-separated mode numbers
        when it has bending modes, nothing otherwise."""
        out = {'{:d}SERINT'.format(count): True} if self.integrate else {}
        if self.has_boxiness:
            out['{:d}SERBOX'.format(count)] = True
        if self.has_fourier:
            out['{:d}SERFOU'.format(count)] = ','.join(str(m) for m in self.fourier_modes)
        if self.has_spiral:
            out['{:d}SERSPI'.format(count)] = True
        if self.radial_law:
            out['{:d}SERLAW'.format(count)] = self.radial_law
        if self.pixel_mean:
            out['{:d}SERAVG'.format(count)] = True
        if self.has_truncation:
            out['{:d}SERTRU'.format(count)] = ','.join(self.truncation_sides)
        if self.has_bending:
            out['{:d}SERBND'.format(count)] = ','.join(str(m) for m in self.bending_modes)
        return out

    @staticmethod
    def _bending_ok(amps):
        """The support of the bending modes, amps [..., n_modes]: every amplitude finite (the shear is a bijection for
        any value)."""
        return np.all(np.isfinite(np.asarray(amps, dtype=np.float64)), axis=-1)

    def _bending_values(self, vals, n_w=None):
        """The amplitudes of the modes present, in mode order: [n_modes] (n_w None: current values) or
        [n_w, n_modes]."""
        shape = (len(self.bending_modes),) if n_w is None else (n_w, len(self.bending_modes))
        get = (lambda k: np.reshape(vals[k], shape[:-1])) if n_w is not None else (lambda k: float(np.ravel(vals(k))[0]))
        return np.stack([get('bend%d' % m) for m in self.bending_modes], axis=-1).reshape(shape).astype(np.float64)

    def bending_list(self):
        """The current values as the definition functions take them: [(m, a_m), ...] in mode order, or None for a
        component without the keyword."""
        if not self.has_bending:
            return None
        return list(zip(self.bending_modes, (float(a) for a in self._bending_values(lambda k: getattr(self, k)))))

    @staticmethod
    def _truncation_ok(trunc, flags):
        """The support of the truncation, trunc [..., 4] = (in_lo, in_hi, out_lo, out_hi) and `flags` the sides present
        (bit 0 inner, bit 1 outer): the two values of a side present finite with 0 <= lo < hi; an absent side's
        entries are not looked at, and there is no condition between the sides."""
        t = np.asarray(trunc, dtype=np.float64)
        ok = np.ones(t.shape[:-1], dtype=bool)
        with np.errstate(invalid='ignore'):
            for side in range(2):
                if (flags >> side) & 1:
                    lo, hi = t[..., 2 * side], t[..., 2 * side + 1]
                    ok = ok & np.isfinite(lo) & np.isfinite(hi) & (lo >= 0) & (hi > lo)
        return ok

    def _truncation_values(self, vals, n_w=None):
        """psfmc_set_truncation_layout's entries (in_lo, in_hi, out_lo, out_hi), TRUNC_ABSENT for an absent side: [4]
        (n_w None: current values) or [n_w, 4]."""
        get = (lambda k: np.reshape(vals[k], (n_w,))) if n_w is not None else (lambda k: float(np.ravel(vals(k))[0]))
        fill = (lambda v: np.full(n_w, v)) if n_w is not None else float
        cols = [np.asarray(get(a), dtype=np.float64) if (self.truncation_flags >> (j // 2)) & 1 else fill(absent)
                for j, (a, absent) in enumerate(zip(Sersic.TRUNC_ATTRS, Sersic.TRUNC_ABSENT))]
        return np.stack(cols, axis=-1)

    def truncation_tuple(self):
        """The current values as the definition functions take them: (in_lo, in_hi, out_lo, out_hi) with None for
        an absent side, or None for a component without the keyword."""
        if not self.has_truncation:
            return None
        t = self._truncation_values(lambda k: getattr(self, k))
        return tuple(float(t[j]) if (self.truncation_flags >> (j // 2)) & 1 else None for j in range(4))

    @staticmethod
    def _spiral_ok(spiral):
        """The support of the spiral, spiral [..., 6] = (r_in, r_out, winding, alpha, inclination, sky_angle) with
        the angles in radians: every value finite, r_in >= 0, r_out > r_in, alpha >= 0, |inclination| < pi/2."""
        s = np.asarray(spiral, dtype=np.float64)
        with np.errstate(invalid='ignore'):
            return (np.all(np.isfinite(s), axis=-1) & (s[..., 0] >= 0) & (s[..., 1] > s[..., 0]) & (s[..., 3] >= 0) &
                    (np.abs(s[..., 4]) < 0.5 * np.pi))

    def _spiral_values(self, vals, n_w=None):
        """(r_in, r_out, winding, alpha, inclination, sky_angle), the angles in radians: [6] (n_w None: current
        values) or [n_w, 6]."""
        get = (lambda k: np.reshape(vals[k], (n_w,))) if n_w is not None else (lambda k: float(np.ravel(vals(k))[0]))
        cols = [np.asarray(get(a), dtype=np.float64) for a in Sersic.SPIRAL_ATTRS]
        if self.angle_degrees:
            cols = [np.deg2rad(c) if a in Sersic.SPIRAL_ANGLES else c for a, c in zip(Sersic.SPIRAL_ATTRS, cols)]
        return np.stack(cols, axis=-1)

    @staticmethod
    def _fourier_ok(amps, phases):
        """The support of the modes, amps / phases [..., n_modes]: every value finite and sum |a_m| < 1, so that
        1 + eps > 0 at every angle."""
        amps, phases = np.asarray(amps, dtype=np.float64), np.asarray(phases, dtype=np.float64)
        with np.errstate(invalid='ignore'):
            return (np.all(np.isfinite(amps), axis=-1) & np.all(np.isfinite(phases), axis=-1) &
                    (np.sum(np.abs(amps), axis=-1) < 1))

    def _fourier_values(self, vals, n_w=None):
        """(amps, phases in radians), each [n_modes] (n_w None: current values) or [n_w, n_modes]."""
        shape = (len(self.fourier_modes),) if n_w is None else (n_w, len(self.fourier_modes))
        get = (lambda k: np.reshape(vals[k], shape[:-1])) if n_w is not None else (lambda k: float(np.ravel(vals(k))[0]))
        amps = np.stack([get('f%d_amp' % m) for m in self.fourier_modes], axis=-1).reshape(shape)
        phases = np.stack([get('f%d_phase' % m) for m in self.fourier_modes], axis=-1).reshape(shape)
        return amps, (np.deg2rad(phases) if self.angle_degrees else phases)

    @staticmethod
    def _boxiness_ok(c):
        """The support of the boxiness: finite and above -2 (e = c + 2 > 0)."""
        c = np.asarray(c, dtype=np.float64)
        with np.errstate(invalid='ignore'):
            return np.isfinite(c) & (c > -2)

    # axis-ratio constraint: reff_b <= reff (Sersic.py:41-45); the boxiness has its support
    def log_priors(self):
        logp = super(Sersic, self).log_priors()
        if self.has_boxiness and not np.all(Sersic._boxiness_ok(self.boxiness)):
            return -np.inf
        if self.has_fourier and not Sersic._fourier_ok(*self._fourier_values(lambda k: getattr(self, k))):
            return -np.inf
        if self.has_spiral and not Sersic._spiral_ok(self._spiral_values(lambda k: getattr(self, k))):
            return -np.inf
        if self.has_truncation and not Sersic._truncation_ok(self._truncation_values(lambda k: getattr(self, k)),
                                                              self.truncation_flags):
            return -np.inf
        if self.has_bending and not Sersic._bending_ok(self._bending_values(lambda k: getattr(self, k))):
            return -np.inf
        return logp + (-np.inf if self.reff_b > self.reff else 0)

    def log_priors_batch(self, block, resolved=None):
        logp = super(Sersic, self).log_priors_batch(block)
        vals = self.values_batch(block, resolved)
        logp = np.where(vals['reff_b'] > vals['reff'], -np.inf, logp)
        if self.has_boxiness:
            logp = np.where(Sersic._boxiness_ok(np.reshape(vals['boxiness'], (len(logp),))), logp, -np.inf)
        if self.has_fourier:
            logp = np.where(Sersic._fourier_ok(*self._fourier_values(vals, len(logp))), logp, -np.inf)
        if self.has_spiral:
            logp = np.where(Sersic._spiral_ok(self._spiral_values(vals, len(logp))), logp, -np.inf)
        if self.has_truncation:
            logp = np.where(Sersic._truncation_ok(self._truncation_values(vals, len(logp)), self.truncation_flags),
                            logp, -np.inf)
        if self.has_bending:
            logp = np.where(Sersic._bending_ok(self._bending_values(vals, len(logp))), logp, -np.inf)
        return logp

    @staticmethod
    def kappa(index):
        """b_n of Ciotti & Bertin (1999): gammaincinv(2n, 1/2) (Sersic.py:47-53)."""
        return gammaincinv(2 * index, 0.5)

    @staticmethod
    def sb_eff(flux_tot, index, reff, reff_b, kappa=None):
        """Surface brightness at the effective radius (Sersic.py:55-71)."""
        if kappa is None:
            kappa = Sersic.kappa(index)
        return flux_tot / (np.pi * reff * reff_b * 2 * index *
                           np.exp(kappa + np.log(kappa) * -2 * index) *
                           gamma(2 * index))

    # -- host meaning of the profile ---------------------------------------------------------------
    def derived_row(self, mag_zp):
        """The nine scalars the rasterisers work from (include/psfmc_hip.h, Sersic block of a row) for this
        component's current values: x0, y0, the rows of the inverse ellipse matrix, kappa, 1/(2n), Sigma_e."""
        angle = np.deg2rad(self.angle) if self.angle_degrees else self.angle
        sin_t, cos_t = np.sin(angle + 0.5 * np.pi), np.cos(angle + 0.5 * np.pi)
        kappa = Sersic.kappa(self.index)
        flux = 10 ** (-0.4 * (self.mag - mag_zp))
        xy = np.ravel(self.xy)
        return np.array([xy[0], xy[1], cos_t / self.reff, sin_t / self.reff, -sin_t / self.reff_b,
                         cos_t / self.reff_b, kappa, 0.5 / self.index,
                         Sersic.sb_eff(flux, self.index, self.reff, self.reff_b, kappa)], dtype=np.float64)

    def add_to_array(self, arr, mag_zp):
        """Add this component (current values) to `arr` on the host: the reference's formula, or the
        pixel-integrated profile with `integrate=True`.  The GPU rasterisers compute the same."""
        row = self.derived_row(mag_zp)
        if self.has_truncation or self.has_bending:
            amps, phases = self._fourier_values(lambda k: getattr(self, k)) if self.has_fourier else ((), ())
            args = (self.radial_law, row, self._radial_values(lambda k: getattr(self, k)) if self.radial_law else None,
                    float(np.ravel(self.boxiness)[0]) if self.has_boxiness else 0.0,
                    list(zip(self.fourier_modes, amps, phases)),
                    self._spiral_values(lambda k: getattr(self, k)) if self.has_spiral else None)
            if self.pixel_mean:
                arr += Sersic.general_mean_image(*args, shape=arr.shape, truncation=self.truncation_tuple(),
                                                 bending=self.bending_list())
            else:
                arr += Sersic.bent_image(*args, truncation=self.truncation_tuple(), bending=self.bending_list(),
                                         shape=arr.shape)
            return arr
        if self.pixel_mean:
            amps, phases = self._fourier_values(lambda k: getattr(self, k)) if self.has_fourier else ((), ())
            arr += Sersic.general_mean_image(
                self.radial_law, row, self._radial_values(lambda k: getattr(self, k)) if self.radial_law else None,
                float(np.ravel(self.boxiness)[0]) if self.has_boxiness else 0.0,
                list(zip(self.fourier_modes, amps, phases)),
                self._spiral_values(lambda k: getattr(self, k)) if self.has_spiral else None, arr.shape)
            return arr
        if self.radial_law:
            amps, phases = self._fourier_values(lambda k: getattr(self, k)) if self.has_fourier else ((), ())
            arr += Sersic.radial_image(self.radial_law, row, self._radial_values(lambda k: getattr(self, k)),
                                       float(np.ravel(self.boxiness)[0]) if self.has_boxiness else 0.0,
                                       list(zip(self.fourier_modes, amps, phases)),
                                       self._spiral_values(lambda k: getattr(self, k)) if self.has_spiral else None,
                                       arr.shape)
            return arr
        if self.has_spiral:
            amps, phases = self._fourier_values(lambda k: getattr(self, k)) if self.has_fourier else ((), ())
            arr += Sersic.spiral_image(row, float(np.ravel(self.boxiness)[0]) if self.has_boxiness else 0.0,
                                       list(zip(self.fourier_modes, amps, phases)),
                                       self._spiral_values(lambda k: getattr(self, k)), arr.shape)
            return arr
        if self.has_fourier:
            amps, phases = self._fourier_values(lambda k: getattr(self, k))
            arr += Sersic.fourier_image(row, float(np.ravel(self.boxiness)[0]) if self.has_boxiness else 0.0,
                                        list(zip(self.fourier_modes, amps, phases)), arr.shape)
            return arr
        if self.has_boxiness:
            arr += Sersic.general_image(row, float(np.ravel(self.boxiness)[0]), arr.shape)
            return arr
        arr += (Sersic.integrated_image(row, arr.shape) if self.integrate
                else Sersic.reference_image(row, arr.shape))
        return arr

    @staticmethod
    def superellipse_area_ratio(boxiness):
        """A(c) = 4 Gamma(1 + 1/e)^2 / (pi Gamma(1 + 2/e)), e = c + 2: the area of the superellipse
        |u|^e + |v|^e = 1 over the unit circle's (GALFIT's R(C0) is its reciprocal); A(0) = 1."""
        e = np.asarray(boxiness, dtype=np.float64) + 2.0
        return 4.0 / np.pi * np.exp(2.0 * gammaln(1.0 + 1.0 / e) - gammaln(1.0 + 2.0 / e))

    @staticmethod
    def general_image(row, boxiness, shape, bending=None):
        """The profile with boxy / disky isophotes on a `shape` image, from a derived row (`derived_row`: the plain
        component's) and c = `boxiness`.  This numpy text is the DEFINITION the device kernels
        (csrc/psfmc_general.h) are held to.  With e = c + 2,

            u = m00 dx + m01 dy,  v = m10 dx + m11 dy,  rho^2 = (|u|^e + |v|^e)^(2/e)

        and then the reference's formula unchanged: q = rho^2 / (dx^2 + dy^2), L = ln rho^2, g = -2 kappa p
        exp(L (p - 1/2)), value = sb exp(-kappa expm1(L p)) (1 + g (q/12 g)), with sb = Sigma_e / A(c)
        (`superellipse_area_ratio`), which keeps `mag` the total magnitude.  At c = 0 it is the reference's
        profile in different bits; where the centre is a pixel centre it is NaN like that one."""
        x0, y0, m00, m01, m10, m11, kappa, p, sbeff = row
        e = float(boxiness) + 2.0
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
        dx, dy = xx - x0, yy - y0
        u = m00 * dx + m01 * dy
        v = m10 * dx + m11 * dy
        if bending:                                   # (`bend`; None or empty: the step is left out)
            v = Sersic.bend(row, u, v, bending)
        with np.errstate(all='ignore'):
            rho2 = (np.abs(u) ** e + np.abs(v) ** e) ** (2.0 / e)
            q = rho2 / (dx ** 2 + dy ** 2)
            L = np.log(rho2)
            sb = sbeff / Sersic.superellipse_area_ratio(boxiness)
            g = -2 * kappa * p * np.exp(L * (p - 0.5))
            return sb * np.exp(-kappa * np.expm1(L * p)) * (1 + g * (q / 12 * g))

    @staticmethod
    def _fourier_eps(cos_t, sin_t, modes):
        """eps = sum_m a_m (cos(m t) cos(m phi_m) - sin(m t) sin(m phi_m)): cos(m t), sin(m t) from
        (cos t + i sin t)^m by repeated multiplication (no atan2)."""
        eps = np.zeros(np.shape(cos_t))
        todo = {int(m): (float(a), float(phi)) for m, a, phi in modes}
        if len(todo) != len(list(modes)) or any(m < 1 or m > 6 for m in todo):
            raise ValueError('fourier modes are distinct integers in 1 ... 6')
        cm, sm = cos_t, sin_t
        for m in range(1, max(todo) + 1 if todo else 1):
            if m > 1:
                cm, sm = cm * cos_t - sm * sin_t, sm * cos_t + cm * sin_t
            if m in todo:
                a, phi = todo[m]
                eps = eps + a * (cm * np.cos(m * phi) - sm * np.sin(m * phi))
        return eps

    @staticmethod
    def fourier_area_ratio(boxiness, modes, points=FOURIER_POINTS):
        """Q: the area inside the perturbed isophote over the unperturbed one's, DEFINED as the midpoint sum
            t_k = 2 pi (k + 1/2) / points,  w_k = (|cos t_k|^e + |sin t_k|^e)^(-2/e),
            Q = sum_k w_k (1 + eps(t_k))^-2 / sum_k w_k
        (the flux inside an isophote is proportional to the integral of [h(t) (1 + eps(t))]^-2 over the angle, with
        h = rho_0 / r = w^(-1/2); for one mode at c = 0 the integral is (1 - a^2)^(-3/2))."""
        e = float(boxiness) + 2.0
        t = 2.0 * np.pi * (np.arange(points) + 0.5) / points
        c, s = np.cos(t), np.sin(t)
        w = (np.abs(c) ** e + np.abs(s) ** e) ** (-2.0 / e)
        return np.sum(w * (1.0 + Sersic._fourier_eps(c, s, modes)) ** -2) / np.sum(w)

    @staticmethod
    def fourier_image(row, boxiness, modes, shape, bending=None):
        """The profile with azimuthal Fourier modes on the isophote radius on a `shape` image, from a derived row
        (`derived_row`: the plain component's), c = `boxiness` (0.0 for a component without the keyword) and
        `modes`, a list of (m, a_m, phi_m) with m distinct integers in 1 ... 6 and phi_m in radians.  This numpy
        text is the DEFINITION the device kernels (csrc/psfmc_general.h) are held to.  With e = c + 2,

            u = m00 dx + m01 dy,  v = m10 dx + m11 dy,  r = hypot(u, v),  cos t = u / r,  sin t = v / r
            eps = sum_m a_m (cos(m t) cos(m phi_m) - sin(m t) sin(m phi_m))                 (`_fourier_eps`)
            rho^2 = (|u|^e + |v|^e)^(2/e) (1 + eps)^2

        (GALFIT's r = r0 (1 + sum_m a_m cos(m (theta + phi_m))) with theta the angle in the component's (u, v) frame),
        and then `general_image` unchanged with sb = Sigma_e / (A(c) Q), Q = `fourier_area_ratio`, which keeps
        `mag` the total magnitude.  Zero amplitudes give `general_image`; where the centre is a pixel centre the
        value is NaN like that one's.  Support: finite values and sum_m |a_m| < 1 (1 + eps > 0 at every angle)."""
        x0, y0, m00, m01, m10, m11, kappa, p, sbeff = row
        modes = [(int(m), float(a), float(phi)) for m, a, phi in modes]
        e = float(boxiness) + 2.0
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
        dx, dy = xx - x0, yy - y0
        u = m00 * dx + m01 * dy
        v = m10 * dx + m11 * dy
        if bending:                                   # (`bend`; None or empty: the step is left out)
            v = Sersic.bend(row, u, v, bending)
        with np.errstate(all='ignore'):
            r = np.hypot(u, v)
            eps = Sersic._fourier_eps(u / r, v / r, modes)
            rho2 = (np.abs(u) ** e + np.abs(v) ** e) ** (2.0 / e) * (1.0 + eps) ** 2
            q = rho2 / (dx ** 2 + dy ** 2)
            L = np.log(rho2)
            sb = sbeff / (Sersic.superellipse_area_ratio(boxiness) * Sersic.fourier_area_ratio(boxiness, modes))
            g = -2 * kappa * p * np.exp(L * (p - 0.5))
            return sb * np.exp(-kappa * np.expm1(L * p)) * (1 + g * (q / 12 * g))

    @staticmethod
    def spiral_image(row, boxiness, modes, spiral, shape, bending=None):
        """The profile with its coordinates wound into arms on a `shape` image, from a derived row (`derived_row`:
        the plain component's), c = `boxiness` (0.0 without the keyword), `modes` as for `fourier_image` (may be
        empty) and `spiral` = (r_in, r_out, winding, alpha, inclination, sky_angle), angles in radians.  This numpy
        text is the DEFINITION the device kernels (csrc/psfmc_general.h) are held to.  GALFIT-style coordinate
        rotation, not GALFIT's formula:

            dx = x - x0,  dy = y - y0                                                         (pixel plane)
            X = cos(sky) dx + sin(sky) dy,  Y = (-sin(sky) dx + cos(sky) dy) / cos(incl)      (disk plane)
            r = hypot(X, Y)
            T = (1 + tanh(2 (2 r - r_in - r_out) / (r_out - r_in))) / 2         (0.018 at r_in, 0.982 at r_out)
            P = (r / r_out)^alpha for r > 0;  at r = 0: 1 if alpha == 0 else 0
            t = winding T P
            X' = cos(t) X + sin(t) Y,  Y' = -sin(t) X + cos(t) Y         (the pattern at radius r is turned by +t)
            u = m00 X' + m01 Y',  v = m10 X' + m11 Y'

        and from u, v on `fourier_image` unchanged -- eps from u, v, rho^2 = (|u|^e + |v|^e)^(2/e) (1 + eps)^2, the
        reference's formula with q = rho^2 / (dx^2 + dy^2) taken in the PIXEL plane -- with sb = Sigma_e / (A(c) Q
        cos(incl)).  The rotation (r, phi) -> (r, phi + t(r)) has unit Jacobian and the deprojection the constant
        Jacobian 1 / cos(incl), so every isophote's pixel-plane area is cos(incl) times its disk-plane area and
        `mag` stays the total magnitude in closed form.  winding = inclination = sky_angle = 0 gives `fourier_image`
        (`general_image` without modes) bit for bit; where the centre is a pixel centre the value is NaN like
        theirs.  Support: `_spiral_ok`."""
        x0, y0, m00, m01, m10, m11, kappa, p, sbeff = row
        modes = [(int(m), float(a), float(phi)) for m, a, phi in modes]
        r_in, r_out, winding, alpha, incl, sky = [float(s) for s in spiral]
        e = float(boxiness) + 2.0
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
        dx, dy = xx - x0, yy - y0
        cs, sn, ci = np.cos(sky), np.sin(sky), np.cos(incl)
        with np.errstate(all='ignore'):
            X = cs * dx + sn * dy
            Y = (-sn * dx + cs * dy) / ci
            r = np.hypot(X, Y)
            T = 0.5 * (1.0 + np.tanh(2.0 * (2.0 * r - r_in - r_out) / (r_out - r_in)))
            P = np.where(r > 0, (r / r_out) ** alpha, 1.0 if alpha == 0 else 0.0)
            t = winding * T * P
            ct, st = np.cos(t), np.sin(t)
            Xr = ct * X + st * Y
            Yr = -st * X + ct * Y
            u = m00 * Xr + m01 * Yr
            v = m10 * Xr + m11 * Yr
            if bending:                               # (`bend`; None or empty: the step is left out)
                v = Sersic.bend(row, u, v, bending)
            rho2 = (np.abs(u) ** e + np.abs(v) ** e) ** (2.0 / e)
            area = Sersic.superellipse_area_ratio(boxiness)
            if modes:
                ruv = np.hypot(u, v)
                rho2 = rho2 * (1.0 + Sersic._fourier_eps(u / ruv, v / ruv, modes)) ** 2
                area = area * Sersic.fourier_area_ratio(boxiness, modes)
            q = rho2 / (dx ** 2 + dy ** 2)
            L = np.log(rho2)
            sb = sbeff / area / ci
            g = -2 * kappa * p * np.exp(L * (p - 0.5))
            return sb * np.exp(-kappa * np.expm1(L * p)) * (1 + g * (q / 12 * g))

    @staticmethod
    def _radial_ok(law, pars):
        """The support of a radial law's parameters, pars [..., 2]: 'moffat' (beta, unused) with beta finite and
        > 1; 'ferrer' (alpha, beta) with both finite, alpha >= 0 and beta < 2."""
        q = np.asarray(pars, dtype=np.float64)
        with np.errstate(invalid='ignore'):
            if law == 'moffat':
                return np.isfinite(q[..., 0]) & (q[..., 0] > 1)
            if law == 'ferrer':
                return np.isfinite(q[..., 0]) & np.isfinite(q[..., 1]) & (q[..., 0] >= 0) & (q[..., 1] < 2)
        raise ValueError('radial law {!r}: one of moffat, ferrer'.format(law))

    @staticmethod
    def radial_central(law, row, pars, boxiness=0.0, modes=(), spiral=None):
        """Sigma_0 of `radial_image`: the value at u = v = 0."""
        kappa, sbeff = row[6], row[8]
        # F / (pi r_a r_b) from the index-1 row: Sigma_e 2 n e^kappa kappa^(-2n) Gamma(2n) at n = 1
        norm = sbeff * 2.0 * np.exp(kappa) / (kappa * kappa)
        area = Sersic.superellipse_area_ratio(boxiness)
        if len(modes):
            area = area * Sersic.fourier_area_ratio(boxiness, modes)
        if spiral is not None:
            area = area * np.cos(float(spiral[4]))
        if law == 'moffat':
            beta = float(pars[0])
            g = 4.0 * np.expm1(np.log(2.0) / beta)
            return norm * g * (beta - 1.0) / area
        if law == 'ferrer':
            alpha, beta = float(pars[0]), float(pars[1])
            k = 2.0 - beta
            lnb = gammaln(2.0 / k) + gammaln(alpha + 1.0) - gammaln(2.0 / k + alpha + 1.0)
            return norm / (area * (2.0 / k) * np.exp(lnb))
        raise ValueError('radial law {!r}: one of moffat, ferrer'.format(law))

    @staticmethod
    def radial_image(law, row, pars, boxiness, modes, spiral, shape, bending=None):
        """A component whose RADIAL LAW is not the Sersic law (`Moffat`, `Ferrer`; GALFIT's component types, not the
        reference's) on a `shape` image.  This numpy text is the DEFINITION the device kernels
        (csrc/psfmc_general.h) are held to.  `row` is the derived row of the component's Sersic slot (index 1, the
        radii in the places of reff / reff_b), `pars` = (beta, unused) for 'moffat' and (alpha, beta) for 'ferrer',
        c = `boxiness` (0.0 without the keyword), `modes` as for `fourier_image` (may be empty), `spiral` as for
        `spiral_image` or None.  The coordinates are `spiral_image`'s up to

            rho^2 = (|u|^e + |v|^e)^(2/e) (1 + eps)^2,   e = c + 2

        in units of the semi-major radius; an absent keyword leaves its step out, which gives the bits of its
        neutral value.  With F the total flux, r_a, r_b the radii, N = A(c) Q cos(incl):

            moffat:  g = 4 (2^(1/beta) - 1),  I = Sigma_0 (1 + g rho^2)^-beta,
                     Sigma_0 = F g (beta - 1) / (pi r_a r_b N)        (half the peak at rho = 1/2: r_a is the FWHM)
            ferrer:  k = 2 - beta,  x = rho^k,  I = Sigma_0 (1 - x)^alpha for x < 1, exactly 0 otherwise,
                     Sigma_0 = F / (pi r_a r_b N (2/k) B(2/k, alpha + 1))

        so that `mag` is the total magnitude.  The value is the law at the pixel centre: there is NO centroid term
        (the reference's belongs to the Sersic law, and Ferrer's log-slope diverges at the edge).  Where u = v = 0
        the value is Sigma_0, with or without modes and spiral: an on-pixel centre is finite, unlike the Sersic
        law's NaN.  Support: `_radial_ok`."""
        modes = [(int(m), float(a), float(phi)) for m, a, phi in modes]
        sigma0 = Sersic.radial_central(law, row, pars, boxiness, modes, spiral)
        rho2, centre = Sersic.radial_rho2(row, boxiness, modes, spiral, shape, bending)
        with np.errstate(all='ignore'):
            if law == 'moffat':
                beta = float(pars[0])
                g = 4.0 * np.expm1(np.log(2.0) / beta)
                img = sigma0 * (1.0 + g * rho2) ** -beta
            else:
                alpha, k = float(pars[0]), 2.0 - float(pars[1])
                x = rho2 ** (0.5 * k)
                img = np.where(x < 1.0, sigma0 * np.abs(1.0 - x) ** alpha, 0.0)
            return np.where(centre, sigma0, img)

    @staticmethod
    def radial_rho2(row, boxiness, modes, spiral, shape, bending=None):
        """(rho^2, centre) of `radial_image` on a `shape` image: the squared generalised radius in units of the
        semi-major radius (NaN or 0 where u = v = 0) and the mask of the pixels where u = v = 0.  `bending` (a list of
        (m, a_m); None or empty: absent, the bits of the function without the argument) bends v ahead of everything that
        reads it (`bend`)."""
        x0, y0, m00, m01, m10, m11 = row[:6]
        modes = [(int(m), float(a), float(phi)) for m, a, phi in modes]
        e = float(boxiness) + 2.0
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
        dx, dy = xx - x0, yy - y0
        with np.errstate(all='ignore'):
            if spiral is not None:
                r_in, r_out, winding, alpha_s, incl, sky = [float(s) for s in spiral]
                cs, sn, ci = np.cos(sky), np.sin(sky), np.cos(incl)
                X = cs * dx + sn * dy
                Y = (-sn * dx + cs * dy) / ci
                r = np.hypot(X, Y)
                T = 0.5 * (1.0 + np.tanh(2.0 * (2.0 * r - r_in - r_out) / (r_out - r_in)))
                P = np.where(r > 0, (r / r_out) ** alpha_s, 1.0 if alpha_s == 0 else 0.0)
                t = winding * T * P
                ct, st = np.cos(t), np.sin(t)
                dx, dy = ct * X + st * Y, -st * X + ct * Y
            u = m00 * dx + m01 * dy
            v = m10 * dx + m11 * dy
            if bending:
                v = Sersic.bend(row, u, v, bending)
            rho2 = (np.abs(u) ** e + np.abs(v) ** e) ** (2.0 / e)
            if modes:
                ruv = np.hypot(u, v)
                rho2 = rho2 * (1.0 + Sersic._fourier_eps(u / ruv, v / ruv, modes)) ** 2
            return rho2, (u == 0) & (v == 0)

    # -- bending modes (`bending=...`) -----------------------------------------------------------------------------
    @staticmethod
    def bend(row, u, v, bending):
        """v' of a bent component.  This numpy text is the DEFINITION the device kernels (csrc/psfmc_general.h,
        psfmc_general_mean.h) are held to.  `u`, `v`: the coordinates in units of the semi-major and semi-minor radius,
        exactly as the parent forms them (after the spiral's winding where there is one); `bending`: a list of
        (m, a_m) with m distinct integers in 1 ... 4.

            r_a = 1 / hypot(m00, m01),  r_b = 1 / hypot(m10, m11)        the row's two radii in pixels
            v'  = v + (r_a / r_b) sum_m a_m u^m

        In pixels along (x = r_a u) and across (y = r_b v) the major axis: y' = y + r_a sum_m a_m (x / r_a)^m, GALFIT's
        bending modes with r_scale = r_a and a_m in units of r_a; the ridge v' = 0 lies at y = -r_a sum_m a_m
        (x / r_a)^m.  A shear: unit Jacobian, a bijection for every finite amplitude, and f(0) = 0 keeps the centre.
        Everything downstream reads (u, v'): |u|^e + |v'|^e, the angle of the Fourier eps, the u = v = 0 centre mask,
        rho of the laws and of the truncation ramps.  The Sersic law's centroid term keeps q = rho^2 / (dx^2 + dy^2)
        in the pixel plane, as under the spiral.  Support: `_bending_ok`."""
        todo = {int(m): float(a) for m, a in bending}
        if len(todo) != len(list(bending)) or any(m not in Sersic.BEND_MODES for m in todo):
            raise ValueError('bending modes are distinct integers in 1 ... 4')
        ratio = (1.0 / np.hypot(row[2], row[3])) / (1.0 / np.hypot(row[4], row[5]))
        f, um = np.zeros(np.shape(u)), u
        for m in range(1, max(todo) + 1 if todo else 1):       # u^m by repeated multiplication (no pow)
            if m > 1:
                um = um * u
            if m in todo:
                f = f + todo[m] * um
        return v + ratio * f

    @staticmethod
    def bent_image(law, row, pars, boxiness, modes, spiral, truncation, bending, shape):
        """A general component with bending modes on a `shape` image: `truncated_image`'s value -- the Sersic law
        times the reference's centroid term (`law` None; NaN where the centre is a pixel centre) or `radial_image`'s
        law ('moffat' / 'ferrer'; Sigma_0 at u = v' = 0), times the truncation's factors where `truncation` is given --
        with v' of `bend` in the place of v: rho^2 and the centre mask are `radial_rho2(..., bending)`'s, the centroid
        term's q = rho^2 / (dx^2 + dy^2) stays in the pixel plane, and sb = Sigma_e / (A(c) Q cos(incl)), Sigma_0 and
        `mag` are the parent's (unit Jacobian).  `bending` None or empty gives `truncated_image`'s bits; all-zero
        amplitudes give its values."""
        return Sersic.truncated_image(law, row, pars, boxiness, modes, spiral, truncation, shape, bending)

    # -- truncation (`truncation=...`) ----------------------------------------------------------------------------
    @staticmethod
    def truncation_weight(row, rho2, centre, truncation):
        """The factors of a truncated component, (inner, outer), None for an absent side.  This numpy text is the
        DEFINITION the device kernels (csrc/psfmc_general.h, psfmc_general_mean.h) are held to.  `rho2`, `centre`: the
        squared generalised radius in units of the semi-major radius and the mask of u = v = 0, exactly as
        `radial_rho2` / `general_point` form them (boxiness, (1 + eps)^2 and winding included); `truncation` =
        (in_lo, in_hi, out_lo, out_hi) in pixels along the major axis, None for the values of an absent side.

            r_major = 1 / hypot(m00, m01)            the row's semi-major radius in pixels (reff, fwhm, r_out)
            s     = r_major sqrt(rho2)               the generalised radius in pixels; 0 where u = v = 0
            a(lo, hi) = 2 (2 s - lo - hi) / (hi - lo)          (the spiral ramp's argument)
            inner = 1 / (1 + exp(-2 a(in_lo,  in_hi )))        0.018 at in_lo,  0.982 at in_hi
            outer = 1 / (1 + exp(+2 a(out_lo, out_hi)))        0.982 at out_lo, 0.018 at out_hi

        These are (1 + tanh a) / 2 and (1 - tanh a) / 2 WRITTEN WITHOUT THEIR CANCELLATION: tanh saturates to -+1 at
        |a| = 19, so the tanh forms are exactly 0 from there on, while the factor is e^(-2 |a|) -- 1e-17 at |a| = 19.6,
        1e-280 at |a| = 322 -- and a component seen only through a ramp's tail (an inner ramp beyond the image, a ramp
        a thousandth of a pixel wide) would be 0 in the definition and e^(-2 |a|) times its parent on the device.  An
        exponent that overflows gives 1 / inf = 0.  The truncation follows the component's own isophotes; it has no
        centre or axis ratio of its own.  Support: `_truncation_ok`."""
        in_lo, in_hi, out_lo, out_hi = truncation
        if (in_lo is None) != (in_hi is None) or (out_lo is None) != (out_hi is None):
            raise ValueError('truncation: a side is (lo, hi) or (None, None)')
        r_major = 1.0 / np.hypot(row[2], row[3])
        with np.errstate(all='ignore'):
            s = r_major * np.sqrt(np.where(centre, 0.0, rho2))
            arg = lambda lo, hi: 2.0 * (2.0 * s - float(lo) - float(hi)) / (float(hi) - float(lo))
            inner = None if in_lo is None else 1.0 / (1.0 + np.exp(-2.0 * arg(in_lo, in_hi)))
            outer = None if out_lo is None else 1.0 / (1.0 + np.exp(2.0 * arg(out_lo, out_hi)))
        return inner, outer

    @staticmethod
    def _truncate(value, row, rho2, centre, truncation):
        """value * inner * outer; an absent side's factor is left out (not multiplied by 1.0), and `truncation`
        None returns `value` itself."""
        if truncation is None:
            return value
        for factor in Sersic.truncation_weight(row, rho2, centre, truncation):
            if factor is not None:
                value = value * factor
        return value

    @staticmethod
    def truncated_image(law, row, pars, boxiness, modes, spiral, truncation, shape, bending=None):
        """A general component with an inner and / or outer truncation on a `shape` image: its PARENT VALUE -- what
        the component renders without the keyword: `general_image`, `fourier_image` or `spiral_image` for the Sersic
        law (`law` None; the law times the reference's centroid term, NaN where the centre is a pixel centre),
        `radial_image` for 'moffat' / 'ferrer' (Sigma_0 at u = v = 0) -- times `truncation_weight`'s factors at the
        pixel centre, with rho^2 from `radial_rho2` (the parent's own, modes and winding included).  `truncation`
        None gives the parent's bits.  `mag` stays the total magnitude of the UNTRUNCATED parent
        (`truncation_flux_fraction`).  No refinement is added at the truncation radii: the ramps are soft by
        construction (`pixel_mean=True`, `general_mean_image`, averages the product over each pixel)."""
        modes = [(int(m), float(a), float(phi)) for m, a, phi in modes]
        bending = bending or None                     # (`bend`: the parent and its radius with v' in the place of v)
        if law is not None:
            parent = Sersic.radial_image(law, row, pars, boxiness, modes, spiral, shape, bending)
        elif spiral is not None:
            parent = Sersic.spiral_image(row, boxiness, modes, spiral, shape, bending)
        elif modes:
            parent = Sersic.fourier_image(row, boxiness, modes, shape, bending)
        else:
            parent = Sersic.general_image(row, boxiness, shape, bending)
        if truncation is None:
            return parent
        rho2, centre = Sersic.radial_rho2(row, boxiness, modes, spiral, shape, bending)
        with np.errstate(all='ignore'):
            return Sersic._truncate(parent, row, rho2, centre, truncation)

    @staticmethod
    def truncation_flux_fraction(law, index_or_pars, r_major, truncation):
        """The fraction of the untruncated component's flux that survives the truncation:

            int law(rho) W(r_major rho) rho drho / int law(rho) rho drho

        over the law's own range (scipy.integrate.quad, split at the ramps' radii), W = inner * outer of
        `truncation_weight` at s = r_major rho.  `law` None: the Sersic law exp(-kappa rho^(1/n)) with n =
        `index_or_pars`; 'moffat': `index_or_pars` = (beta,); 'ferrer': (alpha, beta).  Valid with any boxiness, modes,
        spiral and inclination, because every isophote's area is proportional to rho^2.  For reporting (the
        truncated component's total magnitude is mag - 2.5 log10 of it); no kernel uses it."""
        from scipy.integrate import quad
        in_lo, in_hi, out_lo, out_hi = truncation
        r_major = float(r_major)
        if law is None:
            n = float(index_or_pars)
            kap = Sersic.kappa(n)
            f, top = (lambda r: np.exp(-kap * (r ** (1.0 / n) - 1.0))), np.inf
        elif law == 'moffat':
            beta = float(np.ravel(index_or_pars)[0])
            g = 4.0 * np.expm1(np.log(2.0) / beta)
            f, top = (lambda r: (1.0 + g * r * r) ** -beta), np.inf
        elif law == 'ferrer':
            alpha, k = float(index_or_pars[0]), 2.0 - float(index_or_pars[1])
            f, top = (lambda r: max(1.0 - r ** k, 0.0) ** alpha), 1.0
        else:
            raise ValueError('radial law {!r}: one of None, moffat, ferrer'.format(law))

        def weight(r):
            w, s = 1.0, r_major * r
            with np.errstate(over='ignore'):                 # (the factors as `truncation_weight` writes them)
                if in_lo is not None:
                    w *= 1.0 / (1.0 + np.exp(-4.0 * (2.0 * s - in_lo - in_hi) / (in_hi - in_lo)))
                if out_lo is not None:
                    w *= 1.0 / (1.0 + np.exp(4.0 * (2.0 * s - out_lo - out_hi) / (out_hi - out_lo)))
            return w
        cuts = sorted(set(v / r_major for v in truncation if v is not None and 0.0 < v / r_major < top))
        edges = [0.0] + cuts + [top]
        whole = lambda fn: sum(quad(fn, a, b, epsabs=0.0, epsrel=1e-12, limit=200)[0]
                               for a, b in zip(edges[:-1], edges[1:]))
        import warnings
        with warnings.catch_warnings():        # (1e-12 is at the rounding level of some pieces: quad says so, and is right)
            warnings.simplefilter('ignore')
            return whole(lambda r: f(r) * weight(r) * r) / whole(lambda r: f(r) * r)

    @staticmethod
    def _plain(row, x, y):
        """Sigma_e exp(-kappa (rho^(1/n) - 1)) at the points (x, y); at rho = 0 its finite peak Sigma_e e^kappa.
        Returns (f, u, v, q = rho^2, t = q^p)."""
        x0, y0, m00, m01, m10, m11, kappa, p, sbeff = row
        dx, dy = x - x0, y - y0
        u = m00 * dx + m01 * dy
        v = m10 * dx + m11 * dy
        q = u * u + v * v
        with np.errstate(all='ignore'):
            t = np.where(q > 0, np.exp(np.log(q) * p), 0.0)
            return sbeff * np.exp(-kappa * (t - 1)), u, v, q, t

    @staticmethod
    def reference_image(row, shape):
        """The reference's profile (Sersic.py:98-153) from a derived row: NaN where the centre is a pixel centre."""
        x0, y0, m00, m01, m10, m11, kappa, p, sbeff = row
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
        f, _, _, q, t = Sersic._plain(row, xx, yy)
        with np.errstate(all='ignore'):
            g = -2 * kappa * p * t / np.sqrt(q)
            return f * (1 + g * (q / ((xx - x0) ** 2 + (yy - y0) ** 2) / 12 * g))

    @staticmethod
    def integrated_image(row, shape, half_box=INTEG_HALF_BOX, grid=None, split=INTEG_SPLIT, levels=INTEG_LEVELS,
                         sub=INTEG_SUB):
        """The pixel-integrated profile of one component on a `shape` image, from its derived row.  This numpy
        text is the DEFINITION the device kernels are held to.

        1. Every pixel: f (1 + lap f / (24 f)) with f the plain profile at the pixel centre -- the full
           two-dimensional second-order term of the mean over the pixel.
        2. The (2H+1)^2 pixels around (px, py) = floor(centre + 1/2), clipped to the image: the mean of f over an
           s x s midpoint grid, s = `grid(d)` of the Chebyshev distance d from (px, py).
        3. Every pixel whose closed square holds the centre (one, two on an edge, four on a corner): on the
           global grid of pitch h_l = split^-l (l = 0: the pixels), the cells that hold the centre in their closed
           square are split `split` x `split`; a sub-cell that is itself such a cell of level l + 1 is left to
           that level (l < levels), every other one adds (h_l / split)^2 times the mean of f over its `sub` x `sub`
           midpoint grid.  At the last level every sub-cell is sampled.  `sub` is even, so a sample never falls on
           its cell's centre, edges or corners; should the centre coincide with a sample all the same, f there is
           its finite peak Sigma_e e^kappa (`_plain`).  "Holds" is decided on g = (centre + 1/2) split^l: cell
           floor(g) always, cell floor(g) - 1 as well where g is an integer."""
        if grid is None:
            grid = lambda d: INTEG_GRID_NEAR if d <= INTEG_NEAR_RING else INTEG_GRID_FAR
        if sub % 2:
            raise ValueError('sub must be even')
        ny, nx = shape
        x0, y0, m00, m01, m10, m11, kappa, p, sbeff = row
        yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
        f, u, v, q, t = Sersic._plain(row, xx, yy)
        ie2, ib2 = m00 * m00 + m01 * m01, m10 * m10 + m11 * m11          # 1 / r_e^2, 1 / r_b^2
        with np.errstate(all='ignore'):
            tt = kappa * p * t / q
            lap = (tt * tt - tt * (p - 1) / q) * 4 * (u * u * ie2 + v * v * ib2) - 2 * tt * (ie2 + ib2)
            img = f * (1 + lap / 24)
        gx, gy = x0 + 0.5, y0 + 0.5
        if not (np.isfinite(gx) and np.isfinite(gy)) or abs(gx) > 2.0 ** 30 or abs(gy) > 2.0 ** 30:
            return img                                                  # (no pixel of any image is near)
        px, py = int(np.floor(gx)), int(np.floor(gy))

        def held(g, scale):               # indices of the pitch-1/scale cells holding the centre along one axis
            a = np.floor(g * scale)
            return ([int(a) - 1] if g * scale == a else []) + [int(a)]
        for j in range(max(py - half_box, 0), min(py + half_box + 1, ny)):
            for i in range(max(px - half_box, 0), min(px + half_box + 1, nx)):
                if i in held(gx, 1.0) and j in held(gy, 1.0):
                    img[j, i] = 0.0                                     # part 3 below
                    continue
                s = grid(max(abs(i - px), abs(j - py)))
                o = (np.arange(s) + 0.5) / s - 0.5
                sx, sy = np.meshgrid(i + o, j + o)
                img[j, i] = Sersic._plain(row, sx, sy)[0].mean()
        o = (np.arange(sub) + 0.5) / sub
        for l in range(levels + 1):
            scale = float(split) ** l
            cw = 1.0 / (scale * split)                                  # sub-cell pitch of this level
            nxt_x, nxt_y = held(gx, scale * split), held(gy, scale * split)
            for cy in held(gy, scale):
                for cx in held(gx, scale):
                    i, j = int(np.floor(cx / scale)), int(np.floor(cy / scale))      # the pixel of this cell
                    if not (0 <= i < nx and 0 <= j < ny):
                        continue
                    for b in range(split):
                        for a in range(split):
                            ix, iy = cx * split + a, cy * split + b
                            if l < levels and ix in nxt_x and iy in nxt_y:
                                continue
                            sx, sy = np.meshgrid(ix * cw - 0.5 + o * cw, iy * cw - 0.5 + o * cw)
                            img[j, i] += cw * cw * Sersic._plain(row, sx, sy)[0].mean()
        return img

    # -- the pixel-averaged mode of the general components (`pixel_mean=True`) ------------------------------------
    @staticmethod
    def _general_point_x(law, row, pars, boxiness, modes, spiral, x, y, truncation=None, bending=None):
        """(`general_point`'s value, Ferrer's x = rho^(2 - beta) with 0 at u = v = 0 -- None for the other laws)."""
        trunc = lambda val: Sersic._truncate(val, row, rho2, centre, truncation)
        x0, y0, m00, m01, m10, m11, kappa, p, sbeff = row
        modes = [(int(m), float(a), float(phi)) for m, a, phi in modes]
        if law not in Sersic.RADIAL_KINDS:
            raise ValueError('radial law {!r}: one of None, moffat, ferrer'.format(law))
        e = float(boxiness) + 2.0
        dx, dy = np.asarray(x, dtype=np.float64) - x0, np.asarray(y, dtype=np.float64) - y0
        ci = 1.0
        with np.errstate(all='ignore'):
            if spiral is not None:
                r_in, r_out, winding, alpha_s, incl, sky = [float(s) for s in spiral]
                cs, sn, ci = np.cos(sky), np.sin(sky), np.cos(incl)
                X = cs * dx + sn * dy
                Y = (-sn * dx + cs * dy) / ci
                r = np.hypot(X, Y)
                T = 0.5 * (1.0 + np.tanh(2.0 * (2.0 * r - r_in - r_out) / (r_out - r_in)))
                P = np.where(r > 0, (r / r_out) ** alpha_s, 1.0 if alpha_s == 0 else 0.0)
                t = winding * T * P
                ct, st = np.cos(t), np.sin(t)
                dx, dy = ct * X + st * Y, -st * X + ct * Y
            u = m00 * dx + m01 * dy
            v = m10 * dx + m11 * dy
            if bending:
                v = Sersic.bend(row, u, v, bending)
            rho2 = (np.abs(u) ** e + np.abs(v) ** e) ** (2.0 / e)
            if modes:
                ruv = np.hypot(u, v)
                rho2 = rho2 * (1.0 + Sersic._fourier_eps(u / ruv, v / ruv, modes)) ** 2
            centre = (u == 0) & (v == 0)
            if law is None:
                area = Sersic.superellipse_area_ratio(boxiness)
                if modes:
                    area = area * Sersic.fourier_area_ratio(boxiness, modes)
                sb = sbeff / area / ci if spiral is not None else sbeff / area
                return trunc(np.where(centre, sb * np.exp(kappa), sb * np.exp(-kappa * (rho2 ** p - 1.0)))), None
            sigma0 = Sersic.radial_central(law, row, pars, boxiness, modes, spiral)
            if law == 'moffat':
                beta = float(pars[0])
                g = 4.0 * np.expm1(np.log(2.0) / beta)
                return trunc(np.where(centre, sigma0, sigma0 * (1.0 + g * rho2) ** -beta)), None
            alpha, k = float(pars[0]), 2.0 - float(pars[1])
            xk = np.where(centre, 0.0, rho2 ** (0.5 * k))
            return trunc(np.where(xk < 1.0, sigma0 * np.abs(1.0 - xk) ** alpha, 0.0)), xk

    @staticmethod
    def general_point(law, row, pars, boxiness, modes, spiral, x, y, truncation=None, bending=None):
        """The law of a general component at ARBITRARY POINTS (x, y) (arrays of one shape, pixel coordinates): what
        `general_mean_image` averages.  `law` is None (the Sersic law), 'moffat' or 'ferrer'; `row`, `pars`
        (ignored for None), `boxiness`, `modes` and `spiral` as for `radial_image`.  The coordinate chain is
        `spiral_image`'s and `radial_rho2`'s -- an absent keyword leaves its step out -- up to
        rho^2 = (|u|^e + |v|^e)^(2/e) (1 + eps)^2, and then

            Sersic  sb exp(-kappa (rho^(2p) - 1)),  sb = Sigma_e / (A(c) Q cos(incl))
            Moffat, Ferrer  exactly as `radial_image`

        There is NO centroid term: the reference's is a correction for sampling the law at the pixel centre, and this
        is the law itself.  Where u = v = 0 the value is the finite peak, sb e^kappa or Sigma_0.  `truncation` (as for
        `truncation_weight`; None: absent, the bits of the function without the argument) multiplies the value by the
        inner and outer factors at the point, the peak by the factors at s = 0.  `bending` (a list of (m, a_m); None or
        empty: absent, the bits of the function without the argument) bends v ahead of everything that reads it
        (`bend`)."""
        return Sersic._general_point_x(law, row, pars, boxiness, modes, spiral, x, y, truncation, bending)[0]

    @staticmethod
    def general_mean_image(law, row, pars, boxiness, modes, spiral, shape, truncation=None, bending=None):
        """A general component rendered as the MEAN OF ITS LAW OVER EACH PIXEL on a `shape` image (`pixel_mean=True`;
        not the reference's).  This numpy text is the DEFINITION the device kernels (csrc/psfmc_general_mean.h) are
        held to.  With g = `general_point` and the constants INTEG_* of `integrated_image`:

        1. Every pixel: (2 g(centre) + the mean of g at the pixel's four corners) / 3 -- the second-order term of the
           mean over the pixel, which `integrated_image` part 1 takes from the closed Laplacian; the general forms
           have none, and neighbouring pixels share the corner samples.
        2. Ferrer only: a pixel of part 1 whose five samples do not all have x < 1, or all x >= 1 (the truncation
           edge crosses it), is the mean of g over a MEAN_EDGE_GRID x MEAN_EDGE_GRID midpoint grid instead.
        3. The (2H+1)^2 pixels around (px, py) = floor(centre + 1/2), clipped to the image: the mean of g over an
           s x s midpoint grid, s = INTEG_GRID_NEAR at Chebyshev distance <= INTEG_NEAR_RING from (px, py), else
           INTEG_GRID_FAR (`integrated_image` part 2 with g in place of the plain profile).
        4. Every pixel whose closed square holds the centre: `integrated_image` part 3 with g -- the same dyadic
           "holds" decisions, the same even sub-grids, so that no sample falls on the centre unless the centre
           coincides with one, where g is its finite peak.

        Parts 3 and 4 overwrite parts 1 and 2.  `mag` stays the total magnitude through the closed-form factors of
        `general_image`, `fourier_image`, `spiral_image` and `radial_image`.  With `truncation` every sample is
        `general_point(..., truncation)`, the product of the law and the truncation's factors: the scheme is applied
        to the product unchanged, and no refinement is added at the truncation radii (the ramps are soft).  With
        `bending` every sample is the bent law's (`general_point(..., bending)`); the scheme, its box around the centre
        (which the bending leaves in place) and Ferrer's edge pixels are unchanged, and none is added along the ridge."""
        ny, nx = shape
        x0, y0 = row[0], row[1]
        modes = [(int(m), float(a), float(phi)) for m, a, phi in modes]
        point = lambda x, y: Sersic._general_point_x(law, row, pars, boxiness, modes, spiral, x, y, truncation, bending)
        yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
        cyy, cxx = np.mgrid[0:ny + 1, 0:nx + 1].astype(np.float64) - 0.5
        mid, mid_x = point(xx, yy)
        cor, cor_x = point(cxx, cyy)
        img = (2.0 * mid + 0.25 * ((cor[:-1, :-1] + cor[:-1, 1:]) + (cor[1:, :-1] + cor[1:, 1:]))) / 3.0
        if law == 'ferrer':
            ins = [mid_x < 1.0, cor_x[:-1, :-1] < 1.0, cor_x[:-1, 1:] < 1.0, cor_x[1:, :-1] < 1.0, cor_x[1:, 1:] < 1.0]
            n_in = np.sum(ins, axis=0)
            o = (np.arange(MEAN_EDGE_GRID) + 0.5) / MEAN_EDGE_GRID - 0.5
            for j, i in zip(*np.nonzero((n_in > 0) & (n_in < 5))):
                sx, sy = np.meshgrid(i + o, j + o)
                img[j, i] = point(sx, sy)[0].mean()
        gx, gy = x0 + 0.5, y0 + 0.5
        if not (np.isfinite(gx) and np.isfinite(gy)) or abs(gx) > 2.0 ** 30 or abs(gy) > 2.0 ** 30:
            return img                                                  # (no pixel of any image is near)
        px, py = int(np.floor(gx)), int(np.floor(gy))
        grid = lambda d: INTEG_GRID_NEAR if d <= INTEG_NEAR_RING else INTEG_GRID_FAR
        split, levels, sub = INTEG_SPLIT, INTEG_LEVELS, INTEG_SUB

        def held(g, scale):               # indices of the pitch-1/scale cells holding the centre along one axis
            a = np.floor(g * scale)
            return ([int(a) - 1] if g * scale == a else []) + [int(a)]
        for j in range(max(py - INTEG_HALF_BOX, 0), min(py + INTEG_HALF_BOX + 1, ny)):
            for i in range(max(px - INTEG_HALF_BOX, 0), min(px + INTEG_HALF_BOX + 1, nx)):
                if i in held(gx, 1.0) and j in held(gy, 1.0):
                    img[j, i] = 0.0                                     # part 4 below
                    continue
                s = grid(max(abs(i - px), abs(j - py)))
                o = (np.arange(s) + 0.5) / s - 0.5
                sx, sy = np.meshgrid(i + o, j + o)
                img[j, i] = point(sx, sy)[0].mean()
        o = (np.arange(sub) + 0.5) / sub
        for l in range(levels + 1):
            scale = float(split) ** l
            cw = 1.0 / (scale * split)                                  # sub-cell pitch of this level
            nxt_x, nxt_y = held(gx, scale * split), held(gy, scale * split)
            for cy in held(gy, scale):
                for cx in held(gx, scale):
                    i, j = int(np.floor(cx / scale)), int(np.floor(cy / scale))      # the pixel of this cell
                    if not (0 <= i < nx and 0 <= j < ny):
                        continue
                    for b in range(split):
                        for a in range(split):
                            ix, iy = cx * split + a, cy * split + b
                            if l < levels and ix in nxt_x and iy in nxt_y:
                                continue
                            sx, sy = np.meshgrid(ix * cw - 0.5 + o * cw, iy * cw - 0.5 + o * cw)
                            img[j, i] += cw * cw * point(sx, sy)[0].mean()
        return img
