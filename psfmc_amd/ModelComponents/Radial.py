"""
Components whose RADIAL LAW is not the Sersic law: `Moffat` and `Ferrer` (GALFIT's component types and parameter
names; not the reference's).  Both are functions of the generalised radius alone, so they take `boxiness`, `fourier`,
`spiral`, `truncation` and `bending` exactly as `Sersic` does, occupy a Sersic slot of the model (index fixed at 1, the two radii in the
places of reff / reff_b) and always run the general kernels.  Definition: `Sersic.radial_image`.
"""
import numpy as np

from .ComponentBase import ComponentBase, StochasticProperty
from .Sersic import Sersic


class _RadialLaw(Sersic):
    """What `Moffat` and `Ferrer` share: the renamed radii, the law's parameters and their support."""
    RADII = ()                # the attributes in the places of reff, reff_b
    LAW_ATTRS = ()            # the law's parameters in the order of psfmc_set_radial_layout's entries (padded with 0)

    # the Sersic names of the radii read the renamed attributes (log_priors, derived_row)
    reff = property(lambda self: getattr(self, self.RADII[0]))
    reff_b = property(lambda self: getattr(self, self.RADII[1]))

    def _init_law(self, xy, mag, angle, angle_degrees, boxiness, fourier, spiral, pixel_mean=False, truncation=None,
                  bending=None):
        ComponentBase.__init__(self)
        self.xy = xy
        self.mag = mag
        self.index = 1.0          # the slot's Sersic constants (kappa, Sigma_e) are formed for n = 1
        self.angle = angle
        self.angle_degrees = angle_degrees
        self.integrate = False
        self._init_shape(boxiness, fourier, spiral, pixel_mean, truncation, bending)

    @property
    def is_general(self):
        """Always: the laws live in the general kernels (boxiness 0 when absent)."""
        return True

    def values_batch(self, block, resolved=None):
        out = super(_RadialLaw, self).values_batch(block, resolved)
        out['reff'], out['reff_b'] = out[self.RADII[0]], out[self.RADII[1]]
        return out

    def _radial_values(self, vals, n_w=None):
        """The law's RADIAL_PARAMS entries: [2] (n_w None: current values) or [n_w, 2]."""
        get = (lambda k: np.reshape(vals[k], (n_w,))) if n_w is not None else (lambda k: float(np.ravel(vals(k))[0]))
        cols = [np.asarray(get(a), dtype=np.float64) for a in self.LAW_ATTRS]
        cols += [np.zeros_like(cols[0])] * (Sersic.RADIAL_PARAMS - len(cols))
        return np.stack(cols, axis=-1)

    def log_priors(self):
        logp = super(_RadialLaw, self).log_priors()
        if not Sersic._radial_ok(self.radial_law, self._radial_values(lambda k: getattr(self, k))):
            return -np.inf
        return logp

    def log_priors_batch(self, block, resolved=None):
        logp = super(_RadialLaw, self).log_priors_batch(block, resolved)
        vals = self.values_batch(block, resolved)
        return np.where(Sersic._radial_ok(self.radial_law, self._radial_values(vals, len(logp))), logp, -np.inf)


# Sersic's abbreviations of the shape keywords; the spiral's and the truncation's go first (`spiral_r_out` and
# `spiral_alpha` hold the names `r_out` and `alpha`, and the abbreviations are applied in order)
_SPIRAL_ABBRS = [pair for pair in Sersic._fits_abbrs if pair[0].startswith(('spiral_', 'trunc_'))]
_SHAPE_ABBRS = [pair for pair in Sersic._fits_abbrs
                if pair[0] not in ('Sersic', 'reff_b', 'reff', 'index') and pair not in _SPIRAL_ABBRS]


class Moffat(_RadialLaw):
    """Elliptical Moffat profile, I = Sigma_0 (1 + g rho^2)^-beta with g = 4 (2^(1/beta) - 1): power-law wings, for
    the unresolved flux a PSF mismatch leaves round a point source or a seeing-limited compact bulge.  `fwhm` /
    `fwhm_b` are the FULL widths at half maximum along the major / minor axis (half the peak lies at rho = 1/2),
    `beta` the wing exponent, `mag` the total magnitude: Sigma_0 = F g (beta - 1) / (pi fwhm fwhm_b A(c) Q cos(incl)).
    Support: beta finite and > 1, fwhm_b <= fwhm (log-prior -inf otherwise).  `angle`, `angle_degrees`, `boxiness`,
    `fourier`, `spiral`, `truncation` and `bending` are `Sersic`'s (the truncation radii in pixels along the major
    axis; `mag` stays the untruncated total).  The value is the law at the pixel centre -- no centroid term, the
    reference's belongs to the Sersic law -- and an on-pixel centre is finite (Sigma_0).  There is no `integrate`;
    `pixel_mean=True` renders the mean of the law over each pixel instead (`Sersic.general_mean_image`), which is what
    a `fwhm` of a few pixels needs.  Definition: `Sersic.radial_image`."""
    radial_law = 'moffat'
    RADII = ('fwhm', 'fwhm_b')
    LAW_ATTRS = ('beta',)
    SLOT_ATTRS = ('angle', 'index', 'mag', 'fwhm', 'fwhm_b')
    _fits_abbrs = ([('Moffat', 'MOF')] + _SPIRAL_ABBRS + [('fwhm_b', 'FWB'), ('fwhm', 'FW'), ('beta', 'BET')] +
                   _SHAPE_ABBRS)

    fwhm = StochasticProperty()
    fwhm_b = StochasticProperty()
    beta = StochasticProperty()

    def __init__(self, xy=None, mag=None, fwhm=None, fwhm_b=None, beta=None, angle=None, angle_degrees=False,
                 boxiness=None, fourier=None, spiral=None, pixel_mean=False, truncation=None, bending=None):
        self._init_law(xy, mag, angle, angle_degrees, boxiness, fourier, spiral, pixel_mean, truncation, bending)
        self.fwhm = fwhm
        self.fwhm_b = fwhm_b
        self.beta = beta


class Ferrer(_RadialLaw):
    """Elliptical Ferrer profile, I = Sigma_0 (1 - rho^(2 - beta))^alpha inside rho = 1 and exactly 0 outside: a flat
    core and a sharp outer truncation, the bar (normally with a positive `boxiness`).  `r_out` / `r_out_b` are the
    truncation radii along the major / minor axis, `alpha` the sharpness of the truncation, `beta` the central
    slope, `mag` the total magnitude: Sigma_0 = F / (pi r_out r_out_b A(c) Q cos(incl) (2/k) B(2/k, alpha + 1)),
    k = 2 - beta.  Support: alpha, beta finite, alpha >= 0, beta < 2, r_out_b <= r_out (log-prior -inf otherwise).
    `angle`, `angle_degrees`, `boxiness`, `fourier`, `spiral`, `truncation` and `bending` are `Sersic`'s (the truncation radii
    in pixels along the major axis; `mag` stays the untruncated total).  The value is the law at the pixel
    centre -- no centroid term: the reference's belongs to the Sersic law, and this law's log-slope diverges at the
    edge -- and an on-pixel centre is finite (Sigma_0).  There is no `integrate`; `pixel_mean=True` renders the mean
    of the law over each pixel instead (`Sersic.general_mean_image`: the pixels the truncation edge crosses are
    sampled on an 8 x 8 grid).  Definition: `Sersic.radial_image`."""
    radial_law = 'ferrer'
    RADII = ('r_out', 'r_out_b')
    LAW_ATTRS = ('alpha', 'beta')
    SLOT_ATTRS = ('angle', 'index', 'mag', 'r_out', 'r_out_b')
    _fits_abbrs = ([('Ferrer', 'FER')] + _SPIRAL_ABBRS +
                   [('r_out_b', 'ROB'), ('r_out', 'RO'), ('alpha', 'ALP'), ('beta', 'BET')] + _SHAPE_ABBRS)

    r_out = StochasticProperty()
    r_out_b = StochasticProperty()
    alpha = StochasticProperty()
    beta = StochasticProperty()

    def __init__(self, xy=None, mag=None, r_out=None, r_out_b=None, alpha=None, beta=None, angle=None,
                 angle_degrees=False, boxiness=None, fourier=None, spiral=None, pixel_mean=False, truncation=None,
                 bending=None):
        self._init_law(xy, mag, angle, angle_degrees, boxiness, fourier, spiral, pixel_mean, truncation, bending)
        self.r_out = r_out
        self.r_out_b = r_out_b
        self.alpha = alpha
        self.beta = beta
