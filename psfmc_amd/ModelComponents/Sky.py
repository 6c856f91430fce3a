"""
Sky background component.

A spatially constant level, in the same units as the observed image (ADU per
pixel).  Being constant it passes through the PSF convolution unchanged except
for the PSF's normalisation, and it contributes `adu**2 * sum(psf variance)` to
the model variance; on the GPU it is simply the starting value of every
rasterised pixel (`raster_row` in csrc/psfmc_device.h).  Several Sky components
in one model add up.  Reference: psfMC/ModelComponents/Sky.py:14-16.
"""
import numpy as np

from .ComponentBase import ComponentBase, StochasticProperty


class Sky(ComponentBase):
    """`adu` alone is the reference's constant sky.  `slope=(sx, sy)` (not the reference's; GALFIT's sky
    gradient) tilts it: adu + sx (x - (nx-1)/2) + sy (y - (ny-1)/2) over the field's own image, so that `adu`
    stays the level at the image centre (`Sky.tilted_image`)."""
    #: understood by the device rasteriser as an additive constant
    device_kind = 'sky'
    _fits_abbrs = [('slope', 'SLP')]

    #: level in ADU: a number, or a prior (e.g. ``Normal(loc=0, scale=0.01)``)
    adu = StochasticProperty()
    #: gradient (d/dx, d/dy) in ADU per pixel per pixel: two numbers, a two-element prior, or None (absent:
    #: the component, its parameters and its kernels are the constant sky's)
    slope = StochasticProperty()

    def __init__(self, adu=None, slope=None):
        ComponentBase.__init__(self)
        if adu is None:
            raise ValueError('Sky needs a level `adu` (a value or a prior)')
        self.adu = adu
        self.has_slope = slope is not None
        if self.has_slope:
            if np.size(slope.value if hasattr(slope, 'value') else slope) != 2:
                raise ValueError('Sky slope needs two values (d/dx, d/dy)')
            self.slope = slope

    def header_flags(self, count):
        """FITS header keys this component adds to a database: `<count>SKYSLP = T` for a tilted sky."""
        return {'{:d}SKYSLP'.format(count): True} if self.has_slope else {}

    @staticmethod
    def tilted_image(adu, slope, shape):
        """adu + sx (x - (nx-1)/2) + sy (y - (ny-1)/2) on a `shape` = (ny, nx) image: the DEFINITION the device
        kernel (csrc/psfmc_general.h) is held to.  The level is the value at the image centre."""
        ny, nx = shape
        sx, sy = np.ravel(np.asarray(slope, dtype=np.float64))
        yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
        return adu + (sx * (xx - 0.5 * (nx - 1)) + sy * (yy - 0.5 * (ny - 1)))

    def add_to_array(self, arr, mag_zp=None):
        """Add this component (current values) to `arr` on the host."""
        if self.has_slope:
            arr += Sky.tilted_image(float(np.ravel(self.adu)[0]), self.slope, arr.shape)
        else:
            arr += float(np.ravel(self.adu)[0])
        return arr

    def __repr__(self):
        extra = ', slope={!r}'.format(self._priors.get('slope', self._constants.get('slope'))) if self.has_slope else ''
        return 'Sky(adu={!r}{})'.format(self._priors.get('adu', self._constants.get('adu')), extra)
