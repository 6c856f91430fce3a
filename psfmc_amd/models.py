"""
Composite model + the batched log-posterior -- the drop-in for
`psfMC.models.MultiComponentModel` (psfMC/models.py).

Host side (this file): model-file parsing, the parameter packing contract,
vectorised priors with the non-finite early-out, derivation of the per-walker
scalars the GPU needs (flux, Sersic b_n, surface brightness at r_e, inverse
ellipse matrix), NaN -> -inf mapping.  Device side (libpsfmc_hip): everything
from models.py:213 to :236 for all walkers of a batch at once.
"""
import copy

import numpy as np

from .ModelComponents import Configuration, PointSource, Sersic, Sky
from .ModelComponents.ComponentBase import ComponentBase, Tied
from .ModelComponents.PointSource import SHIFT_METHODS
from .ModelComponents.PSFSelector import PSFSelector
from .model_parser import component_list_from_file
from .utils import mag_to_flux
from . import engine

IMAGE_KINDS = engine.Context.IMAGE_KINDS


# scipy.stats name -> (include/psfmc_hip.h PSFMC_PRIOR_* code, number of shape arguments); the
# device takes the shapes, then loc and scale (randint: low and high with the location folded in)
_DEVICE_FAMILIES = {
    'uniform': (1, 0), 'norm': (2, 0), 'weibull_min': (3, 1), 'randint': (4, 2),
    'truncnorm': (5, 2), 'lognorm': (6, 1), 'halfnorm': (7, 0), 'expon': (8, 0), 'laplace': (9, 0),
    'cauchy': (10, 0), 'halfcauchy': (11, 0), 'logistic': (12, 0), 't': (13, 1), 'beta': (14, 2),
    'reciprocal': (15, 2), 'loguniform': (15, 2), 'weibull_max': (16, 1), 'invgamma': (17, 1),
}
# spiral entries (r_in, r_out, winding, alpha, inclination, sky angle) of a Sersic component without the keyword:
# inside the support, never read
_SPIRAL_ABSENT = (0.0, 1.0, 0.0, 0.0, 0.0, 0.0)
# The five blocks behind the aux entries, in table order (engine._BLOCKS; include/psfmc_hip.h psfmc_set_<name>_layout):
# the model property with the per-Sersic tags, and a Sersic slot's entries -- each the name of a parameter as declared,
# or the constant an absent one holds (neutral, or inside the support of what never reads it).  A block is registered,
# after the aux layout and in this order, only by a model with a tag set; a block in a walker's auxiliary row forces
# those before it.
_AUX_BLOCKS = (
    # per mode 1 ... 6 an amplitude and a phase
    ('fourier', 'sersic_fourier_masks', lambda c: [
        name if m in c.fourier_modes else 0.0 for m in Sersic.FOURIER_MODES for name in ('f%d_amp' % m, 'f%d_phase' % m)]),
    # r_in, r_out, winding, alpha, inclination, sky angle
    ('spiral', 'sersic_spiral_flags', lambda c: list(Sersic.SPIRAL_ATTRS if c.has_spiral else _SPIRAL_ABSENT)),
    # (beta, unused) of a `Moffat`, (alpha, beta) of a `Ferrer`
    ('radial', 'sersic_radial_kinds', lambda c: (
        list(c.LAW_ATTRS if c.radial_law else ()) + [0.0] * Sersic.RADIAL_PARAMS)[:Sersic.RADIAL_PARAMS]),
    # in_lo, in_hi, out_lo, out_hi; flag bit 0 the inner side, bit 1 the outer
    ('truncation', 'sersic_truncation_flags', lambda c: [
        attr if (getattr(c, 'truncation_flags', 0) >> (j // 2)) & 1 else absent
        for j, (attr, absent) in enumerate(zip(Sersic.TRUNC_ATTRS, Sersic.TRUNC_ABSENT))]),
    # a_1 ... a_4; mask bit m - 1 the mode m
    ('bending', 'sersic_bending_masks', lambda c: [
        attr if m in getattr(c, 'bending_modes', ()) else 0.0 for m, attr in zip(Sersic.BEND_MODES, Sersic.BEND_ATTRS)]),
)
_FIRST_NEW_FAMILY = 5           # psfmc_set_layout takes families 0-4; the rest go through psfmc_set_priors


def _device_params_ok(code, params):
    """What psfmc_set_priors accepts (psfmc_theta.h prior_params_ok): the parameters scipy accepts, finite
    (truncnorm's bounds may be infinite), for every element."""
    p = [np.asarray(v, dtype=np.float64) for v in params]
    fin = lambda v: np.isfinite(v)
    pos = lambda v: np.isfinite(v) & (v > 0)
    if code in (1, 2):
        ok = fin(p[0]) & pos(p[1])
    elif code in (3, 6, 13, 16, 17):
        ok = pos(p[0]) & fin(p[1]) & pos(p[2])
    elif code == 4:
        ok = fin(p[0]) & fin(p[1]) & (p[0] == np.rint(p[0])) & (p[1] == np.rint(p[1])) & (p[0] < p[1])
    elif code == 5:
        ok = (p[0] < p[1]) & fin(p[2]) & pos(p[3])
    elif code in (7, 8, 9, 10, 11, 12):
        ok = fin(p[0]) & pos(p[1])
    elif code == 14:
        ok = pos(p[0]) & pos(p[1]) & fin(p[2]) & pos(p[3])
    elif code == 15:
        ok = pos(p[0]) & fin(p[1]) & (p[1] > p[0]) & fin(p[2]) & pos(p[3])
    else:
        return False
    return bool(np.all(ok))


def _device_prior(prior, width):
    """(family, p0, p1, p2, p3) if the library evaluates this prior itself
    (include/psfmc_hip.h PSFMC_PRIOR_*: the scipy.stats arguments in order, each a scalar or one value
    per element of a vector parameter), else None: an unknown family, or parameters scipy rejects."""
    rv = getattr(prior, 'rv_frozen', None)
    if rv is None:
        return None
    try:
        shapes, loc, scale = rv.dist._parse_args(*rv.args, **rv.kwds)
    except Exception:
        return None
    name = rv.dist.name
    ok_size = all(np.size(v) in (1, width) for v in (loc, scale) + tuple(shapes))
    if not ok_size or name not in _DEVICE_FAMILIES:
        return None
    code, n_shapes = _DEVICE_FAMILIES[name]
    if len(shapes) != n_shapes:
        return None
    if code == 4:                   # randint: an integer location moves the bounds
        loc = np.asarray(loc, dtype=np.float64)
        if not np.all(np.isfinite(loc) & (loc == np.rint(loc))):
            return None
        params = (shapes[0] + loc, shapes[1] + loc)
    else:
        params = tuple(shapes) + (loc, scale)
    if not _device_params_ok(code, params):
        return None
    return (code,) + tuple(params) + (0.0,) * (4 - len(params))


def _tie_term(term, name_attr):
    """A tie's ratio or offset as a header records it: the column's name for a prior, else the number -- a float, or
    a tuple of floats for a vector constant."""
    if hasattr(term, 'value'):
        return getattr(term, name_attr)
    vals = tuple(float(v) for v in np.ravel(term))
    return vals[0] if len(vals) == 1 else vals


class MultiComponentModel(object):
    """A 2-D surface-brightness model made of components (Sky, PointSource,
    Sersic) plus one Configuration, given as a model file or a list
    (reference: models.py:9-61).

    device / backend / max_walkers configure the GPU context, which is created
    on first use.  backend: 'fused' (hand-written FFT kernels; sides from
    `engine.FUSED_SIDES`: the powers of two 64...1024 and the even 5-smooth sides in
    between), 'hipfft' (any even size) or 'auto' (fused whenever the shape allows).
    storage: 'f64' (default) or 'f32' -- keep the intermediate half-spectra of the fused path as
    complex64 while all arithmetic stays fp64: half the memory traffic, log-posteriors good to
    ~1e-7 relative (the class of the reference's own float32 raw model, models.py:249) instead
    of ~1e-15; power-of-two sides only.
    """

    def __init__(self, components, device=0, backend='auto', max_walkers=4096, storage='f64'):
        np.seterr(divide='ignore')
        if isinstance(components, str):
            try:
                components = component_list_from_file(components)
            except IOError as err:
                raise IOError('Unable to open model file {}. Does it exist? ({})'
                              .format(components, err))
        components = list(components)
        configs = [c for c in components if isinstance(c, Configuration)]
        if not configs:
            raise ValueError('Unable to find the Configuration component, '
                             'required for setting up input images.')
        config = configs[-1]
        components.remove(config)
        components.append(config.psf_selector)      # always last (models.py:37-38)
        for count, comp in enumerate(components):
            comp.update_stochastic_names(count=count)
            if not isinstance(comp, PSFSelector) and comp.device_kind is None:
                raise NotImplementedError(
                    'component {} has no GPU rasteriser; supported: Sky, '
                    'PointSource, Sersic, Moffat, Ferrer'.format(type(comp).__name__))

        self.config = config
        self.components = components
        self.raw_model_components = [c for c in components
                                     if c.device_kind is not None]
        self.psf_comps = [c for c in components if isinstance(c, PointSource)]
        self.obs_header = config.obs_header

        # column ranges of each component in the emcee vector
        self._spans, pos = [], 0
        for comp in components:
            n = comp.num_stochastics()
            self._spans.append(slice(pos, pos + n))
            pos += n
        self._num_params = pos
        self._param_vector = np.zeros(pos)
        self._ties = self._collect_ties(components)

        self._sky = [c for c in components if isinstance(c, Sky)]
        self._ps = self.psf_comps
        self._sersic = [c for c in components if isinstance(c, Sersic)]
        if backend == 'auto':
            ny, nx = config.obs_data.shape
            psf_shape = np.shape(config.psf_selector.psf_data[0])
            backend = 'fused' if engine.fused_supports(ny, nx, psf_shape) else 'hipfft'
        if storage not in ('f64', 'f32'):
            raise ValueError("storage must be 'f64' or 'f32'")
        self._device, self._backend, self._storage = device, backend, storage
        self._max_walkers = int(max_walkers)
        self._engine = None

        self.blob_images = False      # log_posterior() returns image blobs
        self.posterior_images = {}
        self.accumulated_samples = 0
        self._device_samples = 0
        self.reset_images()

    # -- ties ------------------------------------------------------------------
    @staticmethod
    def _collect_ties(components):
        """The model's ties in component and attribute order: [(component, attr, source component, source attr)],
        checked -- ValueError, naming the attribute, for a tie on or to the PSF index, a source that is itself tied or
        belongs to no component of this model, and widths that do not match."""
        owner = {}                                    # id(prior) -> (component, attr) of every free attribute
        for comp in components:
            for attr in comp.free_names():
                if id(comp._priors[attr]) in owner:
                    first = owner[id(comp._priors[attr])]
                    raise ValueError('{}.{}: the prior object is also given to {}.{}; one object is one parameter -- '
                                     'to make the two equal give Tied(<the prior>) to one of them, to keep them '
                                     'independent give each its own prior'.format(
                                         type(comp).__name__, attr, type(first[0]).__name__, first[1]))
                owner[id(comp._priors[attr])] = (comp, attr)
        ties = []
        for comp in components:
            kind = type(comp).__name__
            for attr in sorted(getattr(comp, '_ties', {})):
                tie, what = comp._ties[attr], '{}.{}'.format(kind, attr)
                if isinstance(comp, PSFSelector):
                    raise ValueError('{}: the PSF index cannot be tied'.format(what))
                if isinstance(tie.source, Tied):
                    raise ValueError('{}: the source of a Tied is itself tied; chains of ties are not supported '
                                     '(tie to its source)'.format(what))
                if not hasattr(tie.source, 'value') or id(tie.source) not in owner:
                    raise ValueError('{}: the source of the Tied is not a free parameter of a component of this '
                                     'model (give the same prior object to the source attribute)'.format(what))
                src_comp, src_attr = owner[id(tie.source)]
                if isinstance(src_comp, PSFSelector):
                    raise ValueError('{}: the PSF index cannot be the source of a Tied'.format(what))
                if src_attr.endswith(tuple('_' + t for t in comp.TIE_TERMS)) and src_attr not in src_comp._declared:
                    raise ValueError('{}: the source of the Tied is the ratio / offset of another tie'.format(what))
                width = comp.attr_width(attr)
                if tie.source.size != width:
                    raise ValueError('{}: a {}-element attribute tied to a source of {} element(s)'.format(
                        what, width, tie.source.size))
                for term in comp.TIE_TERMS:
                    val = getattr(tie, term)
                    if isinstance(val, Tied):
                        raise ValueError('{}: the {} of a Tied is a number or a prior'.format(what, term))
                    size = val.size if hasattr(val, 'value') else np.size(val)
                    if size not in (1, width):
                        raise ValueError('{}: the {} has {} elements; one, or the attribute\'s {}'.format(
                            what, term, size, width))
                    if not hasattr(val, 'value') and not np.all(np.isfinite(np.asarray(val, dtype=np.float64))):
                        raise ValueError('{}: the {} must be finite'.format(what, term))
                ties.append((comp, attr, src_comp, src_attr))
        if sum(c.attr_width(a) for c, a, _, _ in ties) > engine.MAX_TIES:
            raise ValueError('a model holds at most {} tied values'.format(engine.MAX_TIES))
        return ties

    def _tie_terms(self, comp, attr, free, n_w):
        """(ratio, offset) of a tie as arrays that broadcast against the source's [W] or [W, k] values."""
        tie, width, out = comp._ties[attr], comp.attr_width(attr), []
        for term in comp.TIE_TERMS:
            key = '{}_{}'.format(attr, term)
            if key in free:
                val = free[key]                       # [W], or [W, k]
                out.append(val[:, None] if width > 1 and val.ndim == 1 else val)
            else:
                out.append(np.asarray(getattr(tie, term), dtype=np.float64))
        return out

    def _resolved(self, theta):
        """{id(component): {attr: [W] or [W, k]}} of the tied attributes at theta [W, P]: the numpy definition,
        `ratio * source + offset`."""
        if not self._ties:
            return {}
        free = {id(c): c.free_values_batch(theta[:, s]) for c, s in zip(self.components, self._spans)}
        out = {}
        for comp, attr, src_comp, src_attr in self._ties:
            ratio, offset = self._tie_terms(comp, attr, free[id(comp)], theta.shape[0])
            out.setdefault(id(comp), {})[attr] = Tied.resolve(free[id(src_comp)][src_attr], ratio, offset)
        return out

    def _values(self, theta):
        """{id(component): its `values_batch`} at theta [W, P], tied attributes resolved."""
        res = self._resolved(theta)
        return {id(c): c.values_batch(theta[:, s], res.get(id(c))) for c, s in zip(self.components, self._spans)}

    def tied_values(self, theta):
        """{trace name of the tied attribute: [W] or [W, k]} at theta ([P] or [W, P]): ratio * source + offset."""
        res = self._resolved(self._theta(theta))
        return {comp._ties[attr].name: res[id(comp)][attr] for comp, attr, _, _ in self._ties}

    @property
    def tie_records(self):
        """The ties as a database header records them: [(tied fitsname, source fitsname, ratio, offset)], ratio and
        offset each the number (a float; a tuple of floats, one per element, for a vector constant) or the fitsname of
        its column."""
        out = []
        for comp, attr, src_comp, src_attr in self._ties:
            tie = comp._ties[attr]
            terms = [_tie_term(getattr(tie, t), 'fitsname') for t in comp.TIE_TERMS]
            out.append((tie.fitsname, src_comp._priors[src_attr].fitsname, terms[0], terms[1]))
        return out

    # -- engine --------------------------------------------------------------
    @property
    def engine(self):
        if self._engine is None:
            sel = self.config.psf_selector
            self._engine = engine.Context(
                self.config.obs_data, self.config.obs_var, self.config.bad_px,
                np.stack(sel.psf_data), np.stack(sel.psf_var),
                n_ps=len(self._ps), n_sersic=len(self._sersic),
                # small ensembles: room for the device sampler's whole-iteration launches (3 proposal sets of
                # half an ensemble each, psfmc_hip.hip stretch_run_impl)
                max_walkers=self._max_walkers + (self._max_walkers // 2 + 1 if self._max_walkers <= 512 else 0),
                device=self._device, backend=self._backend)
            if self._storage == 'f32':
                self._engine.set_option('storage_f32', 1)
            self._register_layout(self._engine)
        return self._engine

    def _register_layout(self, eng, columns=None, n_params=None):
        """Hand the parameter layout and the priors to the library so that raw
        emcee vectors can be evaluated without host arithmetic.  Priors of
        families the library does not know, and parameters scipy rejects, stay on the host
        (`_host_priors`).  Joint fits (`JointModel`): this model's column c is column columns[c] of
        n_params joint columns, and its prior table is left to the joint one (psfmc_set_joint_priors)."""
        # which Sersic components are the pixel-integrated profile: a property of the model, sent once like the
        # point sources' shift methods (nothing is sent, and nothing changes, for a model without the keyword)
        if any(self.sersic_integrate):
            eng.set_sersic_integrate(self.sersic_integrate)
        col_of = {}                                   # (component id, attr, element) -> column
        family = np.zeros(self.num_params, dtype=np.int32)
        params = np.zeros((self.num_params, engine.PRIOR_NPAR))
        self._host_priors = []                        # (prior, column slice)
        for comp, span in zip(self.components, self._spans):
            pos = span.start
            for name, width in zip(comp.free_names(), comp.stochastic_lens()):
                prior = comp._priors[name]
                desc = _device_prior(prior, width)
                if desc is None:
                    self._host_priors.append((prior, slice(pos, pos + width)))
                for j in range(width):
                    col_of[(id(comp), name, j)] = pos + j
                    if desc is not None:
                        family[pos + j] = desc[0]
                        params[pos + j] = [np.ravel(v)[j if np.size(v) > 1 else 0] for v in desc[1:]]
                pos += width
        slot_col, slot_const = [], []
        # the ties (psfmc_set_ties): one per tied element, named in the tables below by the entry -2 - t
        tie_of, tie_rows = {}, []                     # (component id, attr, element) -> t; (src, ratio, offset) terms
        for comp, attr, src_comp, src_attr in self._ties:
            tie = comp._ties[attr]
            for j in range(comp.attr_width(attr)):
                row = [col_of[(id(src_comp), src_attr, j)]]
                for term in comp.TIE_TERMS:
                    val, key = getattr(tie, term), '{}_{}'.format(attr, term)
                    if hasattr(val, 'value'):
                        row += [col_of[(id(comp), key, j if val.size > 1 else 0)], 0.0]
                    else:
                        row += [-1, float(np.ravel(val)[j if np.size(val) > 1 else 0])]
                tie_of[(id(comp), attr, j)] = len(tie_rows)
                tie_rows.append(row)

        def add(comp, name, elem=0):
            key = (id(comp), name, elem)
            if key in tie_of:
                slot_col.append(-2 - tie_of[key])
                slot_const.append(0.0)
            elif key in col_of:
                slot_col.append(col_of[key])
                slot_const.append(0.0)
            else:
                slot_col.append(-1)
                slot_const.append(float(np.ravel(comp._constants[name])[elem]))
        for c in self._sky:
            add(c, 'adu')
        for c in self._ps:
            add(c, 'mag'); add(c, 'xy', 0); add(c, 'xy', 1)
        for c in self._sersic:
            for name in c.SLOT_ATTRS:                 # angle, index, mag and the class's names of the two radii
                add(c, name)
            add(c, 'xy', 0); add(c, 'xy', 1)
        add(self.config.psf_selector, 'psf_index')
        # auxiliary parameters (Sky slope, Sersic boxiness): per Sky two values, per Sersic one, a component
        # without the keyword a neutral constant; registered after the layout, and only by a model with a keyword
        n_main = len(slot_col)
        for c in self._sky:
            if c.has_slope:
                add(c, 'slope', 0); add(c, 'slope', 1)
            else:
                slot_col += [-1, -1]; slot_const += [0.0, 0.0]
        for c in self._sersic:
            if c.has_boxiness:
                add(c, 'boxiness')
            else:
                slot_col.append(-1); slot_const.append(0.0)
        aux_col, aux_const = slot_col[n_main:], slot_const[n_main:]
        slot_col, slot_const = slot_col[:n_main], slot_const[:n_main]
        # the blocks behind them (_AUX_BLOCKS): a declared entry its column or constant, an absent one its constant
        blocks = []                                   # (name, tags, col, const)
        for name, tags, entries in _AUX_BLOCKS:
            n_before = len(slot_col)
            for c in self._sersic:
                for entry in entries(c):
                    if isinstance(entry, str):
                        add(c, entry)
                    else:
                        slot_col.append(-1); slot_const.append(entry)
            blocks.append((name, getattr(self, tags), slot_col[n_before:], slot_const[n_before:]))
            del slot_col[n_before:], slot_const[n_before:]
        if columns is not None:                       # (constants and ties keep their entries)
            aux_col = [int(columns[c]) if c >= 0 else c for c in aux_col]
            blocks = [(name, tags, [int(columns[c]) if c >= 0 else c for c in col], const)
                      for name, tags, col, const in blocks]
            tie_rows = [[int(columns[r[0]]), int(columns[r[1]]) if r[1] >= 0 else -1, r[2],
                         int(columns[r[3]]) if r[3] >= 0 else -1, r[4]] for r in tie_rows]
        # only a model with ties sends them (and one registered where a tied model stood clears them): every other
        # model makes the calls it always made
        if tie_rows or getattr(eng, 'has_ties', False):
            eng.set_ties(*([list(v) for v in zip(*tie_rows)] if tie_rows else [[]] * 5))

        def register_aux():
            if self.has_aux:
                eng.set_aux_layout(aux_col, aux_const, self.sky_slope_flags, self.sersic_general_flags)
            for name, tags, col, const in blocks:
                if any(tags):
                    getattr(eng, 'set_%s_layout' % name)(tags, col, const)
            # which general components are rendered as the mean over each pixel (`pixel_mean=True`): flags, no
            # entries; the last call, and only by a model with the keyword
            if any(self.sersic_general_mean):
                eng.set_general_mean(self.sersic_general_mean)
        if columns is not None:
            slot_col = [int(columns[c]) if c >= 0 else c for c in slot_col]
            zero = np.zeros(n_params)
            eng.set_layout(len(self._sky), n_params, slot_col, slot_const,
                           [SHIFT_METHODS[c.shift_method] for c in self._ps],
                           [int(bool(c.angle_degrees)) for c in self._sersic],
                           self.config.mag_zeropoint, np.zeros(n_params, dtype=np.int32), zero, zero, zero)
            register_aux()
            return
        # families 0-4 as psfmc_set_layout takes them, the newer ones as host columns there; the full
        # table follows only where a newer family exists (a model of families 1-4 makes the same calls
        # as before they did)
        new = family >= _FIRST_NEW_FAMILY
        base = np.where(new[:, None], 0.0, params)
        eng.set_layout(len(self._sky), self.num_params, slot_col, slot_const,
                       [SHIFT_METHODS[c.shift_method] for c in self._ps],
                       [int(bool(c.angle_degrees)) for c in self._sersic],
                       self.config.mag_zeropoint, np.where(new, 0, family), base[:, 0], base[:, 1], base[:, 2])
        if new.any():
            eng.set_priors(family, params)
        register_aux()

    @property
    def sky_slope_flags(self):
        """[n_sky] which Sky components (model-file order) were given a `slope`."""
        return [bool(getattr(c, 'has_slope', False)) for c in self._sky]

    @property
    def sersic_general_flags(self):
        """[n_sersic] which Sersic components (model-file order) run the general kernels: those given a `boxiness`
        or `fourier` modes (a component with modes alone is a general one at c = 0), a `spiral`, a `truncation` or
        `bending` modes, and every `Moffat` and `Ferrer`."""
        return [bool(getattr(c, 'is_general', False)) for c in self._sersic]

    @property
    def sersic_fourier_masks(self):
        """[n_sersic] bit m - 1 set where the Sersic component (model-file order) has Fourier mode m; 0: none."""
        return [sum(1 << (m - 1) for m in getattr(c, 'fourier_modes', ())) for c in self._sersic]

    @property
    def sersic_spiral_flags(self):
        """[n_sersic] which Sersic components (model-file order) were given a `spiral`."""
        return [bool(getattr(c, 'has_spiral', False)) for c in self._sersic]

    @property
    def sersic_radial_kinds(self):
        """[n_sersic] the radial law of each Sersic slot (model-file order): 0 Sersic, 1 Moffat, 2 Ferrer."""
        return [Sersic.RADIAL_KINDS[getattr(c, 'radial_law', None)] for c in self._sersic]

    @property
    def sersic_truncation_flags(self):
        """[n_sersic] the truncation of each Sersic slot (model-file order): bit 0 inner, bit 1 outer; 0: none."""
        return [int(getattr(c, 'truncation_flags', 0)) for c in self._sersic]

    @property
    def sersic_bending_masks(self):
        """[n_sersic] bit m - 1 set where the Sersic slot (model-file order) has bending mode m; 0: none."""
        return [int(getattr(c, 'bending_mask', 0)) for c in self._sersic]

    @property
    def sersic_general_mean(self):
        """[n_sersic] which Sersic slots (model-file order) were given `pixel_mean=True`."""
        return [bool(getattr(c, 'pixel_mean', False)) for c in self._sersic]

    @property
    def has_aux(self):
        """Does a component carry an auxiliary parameter (Sky `slope`, Sersic `boxiness`, `fourier`, `spiral`,
        `truncation` or `bending`, a `Moffat` or `Ferrer`)?"""
        return any(self.sky_slope_flags) or any(self.sersic_general_flags)

    def aux_rows(self, theta):
        """[W, P] emcee vectors -> [W, 2 n_sky + n_sersic] auxiliary vectors (include/psfmc_hip.h
        psfmc_set_aux_layout: per Sky its slope, per Sersic its boxiness; zeros for components without the
        keyword), or None for a model without the keywords: the companion of `derived_rows`.  A model with Fourier
        modes appends psfmc_set_fourier_layout's 12 n_sersic entries: per Sersic and mode 1 ... 6 the amplitude and
        the phase as declared (zeros for absent modes).  A model with a `spiral` carries those 12 n_sersic entries
        (zeros without modes) and behind them psfmc_set_spiral_layout's 6 n_sersic: per Sersic r_in, r_out, winding,
        alpha, inclination and sky angle as declared (constants inside the support for a component without it).  A
        model with a `Moffat` or `Ferrer` carries both blocks and behind them psfmc_set_radial_layout's 2 n_sersic:
        per Sersic slot (beta, 0) or (alpha, beta), zeros for a slot with the Sersic law.  A model with a `truncation`
        carries the three blocks and behind them psfmc_set_truncation_layout's 4 n_sersic: per Sersic slot in_lo,
        in_hi, out_lo, out_hi (constants inside the support for an absent side): 2 n_sky + 25 n_sersic in all.  A
        model with `bending` modes carries the four blocks and behind them psfmc_set_bending_layout's 4 n_sersic: per
        Sersic slot a_1 ... a_4 (zeros for absent modes): 2 n_sky + 29 n_sersic in all."""
        if not self.has_aux:
            return None
        theta = self._theta(theta)
        n_w = theta.shape[0]
        cols = []
        all_vals = self._values(theta)
        for c, s in zip(self.components, self._spans):
            if isinstance(c, Sky):
                sl = all_vals[id(c)]['slope'] if c.has_slope else np.zeros((n_w, 2))
                sl = np.reshape(sl, (n_w, 2))
                cols += [sl[:, 0], sl[:, 1]]
        for c, s in zip(self.components, self._spans):
            if isinstance(c, Sersic):
                cols.append(np.reshape(all_vals[id(c)]['boxiness'], (n_w,)) if c.has_boxiness
                            else np.zeros(n_w))
        present = [any(getattr(self, tags)) for _, tags, _ in _AUX_BLOCKS]
        for _, _, entries in _AUX_BLOCKS[:max([0] + [b + 1 for b, p in enumerate(present) if p])]:
            for c, s in zip(self.components, self._spans):
                if isinstance(c, Sersic):
                    ents = entries(c)
                    vals = all_vals[id(c)]
                    cols += [np.reshape(vals[e], (n_w,)) if isinstance(e, str) else np.full(n_w, e) for e in ents]
        return np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.float64) for c in cols], axis=1))

    @staticmethod
    def _aux_kw(aux, lo, hi):
        """Keyword for the engine's row-based calls: rows [lo, hi) of `aux_rows`' result, nothing for a model
        without the keywords (whose calls are what they always were)."""
        return {} if aux is None else {'aux': aux[lo:hi]}

    @property
    def sersic_integrate(self):
        """[n_sersic] which Sersic components (model-file order) were given `integrate=True`."""
        return [bool(getattr(c, 'integrate', False)) for c in self._sersic]

    def header_flags(self):
        """Header keys of the components that are not the reference's profile (`Sersic.header_flags`)."""
        out = {}
        for count, comp in enumerate(self.components):
            out.update(getattr(comp, 'header_flags', lambda n: {})(count))
        return out

    def device_group(self, devices, max_walkers=None):
        """A `engine.ContextGroup`: this model's field on several GPUs driven by this one
        process, layout and priors registered (psfmc_group_*).  Its `logpost_theta(theta)`
        splits the walkers over the devices.  The caller closes it."""
        sel = self.config.psf_selector
        grp = engine.ContextGroup(devices, self.config.obs_data, self.config.obs_var, self.config.bad_px,
                                  np.stack(sel.psf_data), np.stack(sel.psf_var), n_ps=len(self._ps),
                                  n_sersic=len(self._sersic), max_walkers=max_walkers or self._max_walkers,
                                  backend=self._backend)
        self._register_layout(grp)
        return grp

    def _host_prior_sum(self, theta):
        """log-prior of the priors the library leaves to the host, or None."""
        if not self._host_priors:
            return None
        total = np.zeros(theta.shape[0])
        with np.errstate(all='ignore'):
            for prior, cols in self._host_priors:
                total = total + prior.logp_batch(theta[:, cols])
        return total

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    # -- parameter vector -----------------------------------------------------
    @property
    def num_params(self):
        return self._num_params

    @property
    def param_names(self):
        return [n for c in self.components for n in c.stochastic_names()]

    @property
    def param_fits_abbrs(self):
        return [n for c in self.components
                for n in c.stochastic_names(name_attr='fitsname')]

    @property
    def param_lens(self):
        return [n for c in self.components for n in c.stochastic_lens()]

    @property
    def param_values(self):
        parts = np.split(self._param_vector, np.cumsum(self.param_lens)[:-1])
        return dict(zip(self.param_names, parts))

    @param_values.setter
    def param_values(self, vector):
        vector = np.asarray(vector, dtype=np.float64)
        self._param_vector = vector
        for comp, span in zip(self.components, self._spans):
            comp.set_stochastic_values(vector[span])

    def get_distribution(self, param_name):
        found = None
        for comp in self.components:
            try:
                found = comp.get_distribution(param_name)
            except KeyError:
                pass
        return found

    def init_params_from_priors(self, nwalkers):
        """Walker start positions drawn from the priors, re-drawing a component
        until its joint prior is finite (models.py:108-130)."""
        out = np.zeros((nwalkers, self.num_params))
        for w in range(nwalkers):
            for comp, span in zip(self.components, self._spans):
                while True:
                    vals = comp.set_stochastic_values('random')
                    if np.isfinite(comp.log_priors()):
                        break
                out[w, span] = vals
        return out

    # -- priors ---------------------------------------------------------------
    def log_priors(self):
        return np.sum([c.log_priors() for c in self.components])

    def log_priors_batch(self, theta):
        theta = self._theta(theta)
        total = np.zeros(theta.shape[0])
        with np.errstate(all='ignore'):
            res = self._resolved(theta)
            for comp, span in zip(self.components, self._spans):
                if id(comp) in res:
                    total = total + comp.log_priors_batch(theta[:, span], res[id(comp)])
                else:
                    total = total + comp.log_priors_batch(theta[:, span])
        return total

    # -- host -> device rows ---------------------------------------------------
    def _theta(self, theta):
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim == 1:
            theta = theta[None, :]
        if theta.ndim != 2 or theta.shape[1] != self.num_params:
            raise ValueError('expected [W, {}] parameter vectors, got {}'
                             .format(self.num_params, theta.shape))
        return theta

    def derived_rows(self, theta):
        """[W, P] emcee vectors -> [W, row_len] rows of include/psfmc_hip.h."""
        theta = self._theta(theta)
        n_w = theta.shape[0]
        zp = self.config.mag_zeropoint
        vals = self._values(theta)
        cols = [sum((vals[id(c)]['adu'] for c in self._sky), np.zeros(n_w))]
        with np.errstate(all='ignore'):
            for c in self._ps:
                v = vals[id(c)]
                cols += [mag_to_flux(v['mag'], zp), v['xy'][:, 0], v['xy'][:, 1],
                         np.full(n_w, float(SHIFT_METHODS[c.shift_method]))]
            for c in self._sersic:
                v = vals[id(c)]
                theta_rot = (np.deg2rad(v['angle']) if c.angle_degrees
                             else v['angle']) + 0.5 * np.pi
                sin_t, cos_t = np.sin(theta_rot), np.cos(theta_rot)
                kappa = Sersic.kappa(v['index'])
                cols += [v['xy'][:, 0], v['xy'][:, 1],
                         cos_t / v['reff'], sin_t / v['reff'],
                         -sin_t / v['reff_b'], cos_t / v['reff_b'],
                         kappa, 0.5 / v['index'],
                         Sersic.sb_eff(mag_to_flux(v['mag'], zp), v['index'],
                                       v['reff'], v['reff_b'], kappa)]
        sel = vals[id(self.config.psf_selector)]
        psf = sel.get('psf_index', np.zeros(n_w))
        cols.append(np.clip(psf, 0, len(self.config.psf_selector.psf_data) - 1))
        return np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.float64)
                                              for c in cols], axis=1))

    # -- the hot path -----------------------------------------------------------
    def log_likelihood_batch(self, theta, skip=None):
        """[W] Gaussian log-likelihoods from the GPU; non-finite -> -inf."""
        rows, aux = self.derived_rows(theta), self.aux_rows(theta)
        cap = self._max_walkers                  # larger batches go through in slices
        parts = [self.engine.loglike(rows[lo:lo + cap], None if skip is None else skip[lo:lo + cap],
                                     **self._aux_kw(aux, lo, lo + cap))
                 for lo in range(0, len(rows), cap)]
        ll = np.concatenate(parts) if parts else np.zeros(0)
        return np.where(np.isfinite(ll), ll, -np.inf)

    def log_posterior_batch(self, theta):
        """log-posterior of W parameter vectors in one GPU batch: priors with the
        non-finite early-out (models.py:208-211), Sersic constants and likelihood
        all on the device; only priors of families the library does not know are
        evaluated here with scipy and passed along per walker."""
        theta = self._theta(theta)
        eng = self.engine
        extra = self._host_prior_sum(theta)
        cap = self._max_walkers
        parts = [eng.logpost_theta(theta[lo:lo + cap], None if extra is None else extra[lo:lo + cap])
                 for lo in range(0, theta.shape[0], cap)]
        return np.concatenate(parts) if parts else np.zeros(0)

    def log_likelihood_and_prior_batch(self, theta):
        """(lnL [W], lnprior [W]) of W parameter vectors from ONE device evaluation, the two terms of
        `log_posterior_batch` apart (psfmc_eval_theta_split): lnL is -inf outside the priors and where it is
        not finite.  The tempered samplers work with these values (sampler.TemperedEnsembleSampler)."""
        theta = self._theta(theta)
        eng = self.engine
        extra = self._host_prior_sum(theta)
        cap = self._max_walkers
        parts = [eng.loglike_prior_theta(theta[lo:lo + cap], None if extra is None else extra[lo:lo + cap])
                 for lo in range(0, theta.shape[0], cap)]
        if not parts:
            return np.zeros(0), np.zeros(0)
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    def log_posterior_batch_host(self, theta):
        """The same through host-side priors and derived rows (scipy.stats /
        scipy.special exactly as the reference calls them); the device only runs the
        likelihood.  Kept as the cross-check of the raw-vector path."""
        theta = self._theta(theta)
        lnprior = self.log_priors_batch(theta)
        skip = ~np.isfinite(lnprior)
        out = np.full(theta.shape[0], -np.inf)
        if not skip.all():
            safe = np.where(skip[:, None], theta[np.argmin(skip)], theta)
            ll = self.log_likelihood_batch(safe, skip)
            ok = ~skip
            out[ok] = ll[ok] + lnprior[ok]
        return out

    @staticmethod
    def log_posterior(param_values, **kwargs):
        """Single-vector form with the reference's signature (models.py:193-243):
        `kwargs` must hold `model`.  Returns (lnprob, blobs)."""
        model = kwargs.pop('model')
        model.param_values = param_values
        lnp = model.log_posterior_batch(param_values)[0]
        blobs = {}
        if model.blob_images and np.isfinite(model.log_priors()):
            blobs = {k: v[0] for k, v in model.sample_images(param_values).items()}
        return float(lnp), blobs

    # -- images ---------------------------------------------------------------
    def sample_images(self, theta, kinds=None):
        """The per-sample images of models.py:222-226 for W vectors:
        dict kind -> [W, ny, nx]."""
        rows, aux = self.derived_rows(theta), self.aux_rows(theta)
        cap = self._max_walkers
        parts = [self.engine.images(rows[lo:lo + cap], kinds, **self._aux_kw(aux, lo, lo + cap))
                 for lo in range(0, max(len(rows), 1), cap)]
        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}

    # -- Fisher matrix and gradient -----------------------------------------------
    def fisher(self, theta, step=None, columns=None):
        """Fisher matrix and gradient of the log-likelihood at theta ([P] or [n, P]) from central-difference stencils
        of device images (psfmc_fisher_rows; the definition: `mode.fisher_from_stencil`).

        columns  the differentiated columns (default: every free column whose prior is not discrete -- the PSF index
                 and its like stay at the base value)
        step     [K] or [n, K] steps h_k (default: 1e-4 x the prior's standard deviation where that is finite and
                 positive, else 1e-4 x max(|theta_k|, 1))
        Returns dict(F [n, K, K], grad [n, K] (of lnL), loglike [n], columns [K], step [n, K]); without the leading
        axis for a [P] theta.  The images do not care about prior supports, so there is no edge handling; a base
        with a stencil image that is not finite on a good pixel gets NaN F and grad, which is not an error."""
        from . import mode
        if self._storage == 'f32':
            raise ValueError("fisher() needs storage='f64': differences of float32-stored images over a 1e-4 step "
                             "are rounding noise")
        single = np.ndim(theta) == 1
        theta = self._theta(theta)
        columns = mode.default_columns(self) if columns is None else np.asarray(columns, dtype=np.int64)
        if columns.ndim != 1 or len(columns) < 1 or columns.min() < 0 or columns.max() >= self.num_params:
            raise ValueError('columns must be a non-empty list of columns of the parameter vector')
        n, k = theta.shape[0], len(columns)
        if step is None:
            step = mode.default_steps(self, theta, columns)
        step = np.array(np.broadcast_to(np.asarray(step, dtype=np.float64), (n, k)))
        if not np.all(np.isfinite(step) & (step > 0)):
            raise ValueError('steps must be finite and positive')
        eng = self.engine
        per_call = eng.max_walkers // (2 * k + 1)
        if per_call < 1:
            raise ValueError('a stencil of {} columns is {} walkers; the model was built for max_walkers={}'.format(
                k, 2 * k + 1, eng.max_walkers))
        fisher, grad, ll = np.empty((n, k, k)), np.empty((n, k)), np.empty(n)
        for lo in range(0, n, per_call):
            hi = min(lo + per_call, n)
            vecs = mode.stencil(theta[lo:hi], step[lo:hi], columns).reshape(-1, self.num_params)
            rows, aux = self.derived_rows(vecs), self.aux_rows(vecs)
            fisher[lo:hi], grad[lo:hi], ll[lo:hi] = eng.fisher_rows(
                rows.reshape(hi - lo, 2 * k + 1, -1), 0.5 / step[lo:hi], **self._aux_kw(aux, 0, len(vecs)))
        bad = ~(np.isfinite(fisher).all(axis=(1, 2)) & np.isfinite(grad).all(axis=1))
        fisher[bad], grad[bad] = np.nan, np.nan
        ll = np.where(np.isfinite(ll), ll, -np.inf)
        out = dict(F=fisher, grad=grad, loglike=ll, columns=columns, step=step)
        return {key: (val[0] if single and key != 'columns' else val) for key, val in out.items()}

    def _one_image(self, kind):
        return self.sample_images(self._param_vector, (kind,))[kind][0]

    def raw_model(self):
        return self._one_image('raw_model')

    def convolved_model(self, raw_px=None):
        return self._one_image('convolved_model')

    def composite_ivm(self, raw_px=None):
        return self._one_image('composite_ivm')

    def residual(self, convolved_px=None, raw_px=None):
        return self._one_image('residual')

    def point_source_subtracted(self):
        return self._one_image('point_source_subtracted')

    def reset_images(self):
        shape = self.config.obs_data.shape
        self.accumulated_samples = 0
        self._device_samples = 0
        if self._engine is not None:
            self._engine.reset_accumulated()
        for kind in IMAGE_KINDS:
            self.posterior_images[kind] = np.ones(shape, dtype=np.float64)

    def accumulate_samples(self, theta):
        """Add the images of W parameter vectors to the posterior means ON THE
        DEVICE (no image leaves the GPU until `collect_posterior_images`)."""
        theta = self._theta(theta)
        eng = self.engine
        for lo in range(0, len(theta), self._max_walkers):
            # flux, kappa, Sigma_e, ellipse matrix on the device (host scipy cost 0.2 ms per sample)
            eng.accumulate_theta(theta[lo:lo + self._max_walkers])
        self._device_samples += len(theta)
        self.accumulated_samples += len(theta)

    def reduce_accumulated(self, ranks):
        """Walkers sharded over GPUs (`parallel.RankGroup`): add up the ranks' device-resident
        posterior sums, so that every rank holds the sums over ALL walkers.  One all-reduce of
        4 images at the end of sampling."""
        if ranks is None or ranks.single or self._engine is None:
            return
        sums, count = self._engine.accumulated_sums()
        total = ranks.all_reduce_sum_host(np.concatenate([sums.ravel(), [float(count)]]))
        n_all = int(round(total[-1]))
        self._engine.set_accumulated_sums(total[:-1].reshape(sums.shape), n_all)
        self._device_samples += n_all - count
        self.accumulated_samples += n_all - count

    def collect_posterior_images(self):
        """Merge the device-resident sums into `posterior_images` (sample-count
        weighted; the weight map in the variance domain) and return that dict."""
        if self._device_samples:
            dev, n_dev = self.engine.accumulated()
            n_host = self.accumulated_samples - self._device_samples
            post = self.posterior_images
            with np.errstate(all='ignore'):
                for kind in IMAGE_KINDS:
                    if n_host == 0:
                        post[kind] = dev[kind]
                    elif kind == 'composite_ivm':
                        post[kind] = (n_host + n_dev) / (n_host / post[kind] + n_dev / dev[kind])
                    else:
                        post[kind] = (n_host * post[kind] + n_dev * dev[kind]) / (n_host + n_dev)
            self.engine.reset_accumulated()
            self._device_samples = 0
            self._merged_device = True
        return self.posterior_images

    def accumulate_images(self, sample_images):
        """Running mean of the per-sample images; the weight map is averaged
        as a variance (models.py:74-97).  `sample_images`: list of dicts
        {kind: [ny, nx]} (emcee blobs) or one dict {kind: [W, ny, nx]}."""
        self.collect_posterior_images()
        if isinstance(sample_images, dict):
            n_w = len(next(iter(sample_images.values())))
            sample_images = [{k: v[i] for k, v in sample_images.items()}
                             for i in range(n_w)]
        post = self.posterior_images
        with np.errstate(all='ignore'):
            post['composite_ivm'] = 1 / post['composite_ivm']
            for imgs in sample_images:
                if not imgs:
                    continue
                self.accumulated_samples += 1
                n = self.accumulated_samples
                for kind, img in imgs.items():
                    step = 1 / img if kind == 'composite_ivm' else img
                    post[kind] = (post[kind] * (n - 1) + step) / n
            post['composite_ivm'] = 1 / post['composite_ivm']


class FieldSet(object):
    """Several fields of one model structure (the same component lists; their own data, image and PSF
    sizes, constants and priors) evaluated in shared GPU batches: `engine.FieldSetContext`.  Every
    field's images and posterior images have its own shape; the fields share one transform shape, which
    each of them pays for (a small field in a set with a large one costs a large field's walker).  The
    reference has no counterpart (one `MultiComponentModel` per model file and process,
    psfMC/fitting.py:13-113); this is for surveys of many small fields, where a batch per field would
    be dominated by its fixed cost (BASELINE config 5).

    models: MultiComponentModel objects (or model files) whose priors all have a device form."""

    def __init__(self, models, max_walkers=4096, device=0):
        # a model object handed in stays what it was (its own context, if it has one, included): the set works
        # on shallow copies that share the components and the data but route through the shared context
        self.models = [copy.copy(m) if isinstance(m, MultiComponentModel) else
                       MultiComponentModel(m, device=device, backend='fused', max_walkers=1) for m in models]
        first = self.models[0]
        for m in self.models:
            if (len(m._ps), len(m._sersic), len(m._sky), m.num_params) != \
                    (len(first._ps), len(first._sersic), len(first._sky), first.num_params):
                raise ValueError('the fields of a FieldSet need the same component lists and free parameters')
        fields = []
        for m in self.models:
            sel = m.config.psf_selector
            fields.append((m.config.obs_data, m.config.obs_var, m.config.bad_px, np.stack(sel.psf_data),
                           np.stack(sel.psf_var)))
        self.context = engine.FieldSetContext(fields, n_ps=len(first._ps), n_sersic=len(first._sersic),
                                              max_walkers=max_walkers, device=device)
        for f, m in enumerate(self.models):
            m._register_layout(self.context.layout_of(f))
            if m._host_priors:
                raise ValueError('field {}: a prior has no device form; a FieldSet evaluates priors on the '
                                 'GPU only'.format(f))
            # the model's images, posterior sums and log-posteriors go through ITS field of the shared
            # context (it never creates a context of its own)
            m._engine = self.context.view(f)
            m.posterior_images = dict(m.posterior_images)      # (a copy's own running means and vector)
            m._param_vector = m._param_vector.copy()
            m._max_walkers = int(max_walkers)
        self.num_params = first.num_params
        self.max_walkers = int(max_walkers)

    def log_posterior_batch(self, thetas):
        """thetas: one [W_f, num_params] array per field -> list of [W_f] log-posteriors."""
        return self.context.logpost_theta(thetas)

    def log_likelihood_and_prior_batch(self, thetas):
        """thetas: one [W_f, num_params] array per field -> list of (lnL [W_f], lnprior [W_f]), the two terms of
        `log_posterior_batch` apart from ONE device evaluation (psfmc_eval_theta_split_fields): what the
        tempered samplers work with.  A member model's own `log_likelihood_and_prior_batch` gives its field's."""
        return self.context.eval_split(thetas)

    def fisher(self, thetas, step=None, columns=None):
        """`MultiComponentModel.fisher` for every field at once: thetas one [n_f, P] (or [P]) array per field, None
        to leave a field out -> a list of the dicts `fs.models[f].fisher(thetas[f])` returns (None for a field left
        out), the same bits.  The stencils of all fields go to the device together (psfmc_fisher_rows_fields): one
        call per group of fields with the same number of differentiated columns, split only where `max_walkers` is
        too small for the group.

        step, columns  None, or one entry per field (an entry None: the defaults of that field's model,
                       `mode.default_steps` / `mode.default_columns`); `columns` may also be one list for all fields"""
        from . import mode
        n_f = len(self.models)
        if len(thetas) != n_f:
            raise ValueError('one parameter array per field')
        per_field = lambda arg: [None] * n_f if arg is None else list(arg)
        if columns is not None and len(columns) and columns[0] is not None and np.ndim(columns[0]) == 0:
            columns = [columns] * n_f
        steps, cols = per_field(step), per_field(columns)
        if len(steps) != n_f or len(cols) != n_f:
            raise ValueError('step / columns: one entry per field')
        jobs, outs = [], [None] * n_f
        for f, (m, theta) in enumerate(zip(self.models, thetas)):
            if theta is None:
                continue
            single = np.ndim(theta) == 1
            theta = m._theta(theta)
            col = mode.default_columns(m) if cols[f] is None else np.asarray(cols[f], dtype=np.int64)
            if col.ndim != 1 or len(col) < 1 or col.min() < 0 or col.max() >= m.num_params:
                raise ValueError('field {}: columns must be a non-empty list of columns of the parameter '
                                 'vector'.format(f))
            n, k = theta.shape[0], len(col)
            if 2 * k + 1 > self.max_walkers:
                raise ValueError('a stencil of {} columns is {} walkers; the set was built for max_walkers={}'.format(
                    k, 2 * k + 1, self.max_walkers))
            h = mode.default_steps(m, theta, col) if steps[f] is None else steps[f]
            h = np.array(np.broadcast_to(np.asarray(h, dtype=np.float64), (n, k)))
            if not np.all(np.isfinite(h) & (h > 0)):
                raise ValueError('steps must be finite and positive')
            vecs = mode.stencil(theta, h, col).reshape(-1, m.num_params)
            rows, aux = m.derived_rows(vecs), m.aux_rows(vecs)
            outs[f] = dict(F=np.empty((n, k, k)), grad=np.empty((n, k)), loglike=np.empty(n), columns=col, step=h)
            jobs.append(dict(f=f, k=k, n=n, single=single, rows=rows.reshape(n, 2 * k + 1, -1),
                             aux=None if aux is None else np.asarray(aux).reshape(n, 2 * k + 1, -1)))
        for k in sorted({j['k'] for j in jobs}):
            group = [j for j in jobs if j['k'] == k]
            for call in mode._pack_fields([(i, j['n']) for i, j in enumerate(group)], self.max_walkers // (2 * k + 1)):
                fields = np.concatenate([np.full(hi - lo, group[i]['f']) for i, lo, hi in call])
                rows = np.concatenate([group[i]['rows'][lo:hi] for i, lo, hi in call])
                inv2h = np.concatenate([0.5 / outs[group[i]['f']]['step'][lo:hi] for i, lo, hi in call])
                aux = _stack_aux([None if group[i]['aux'] is None else group[i]['aux'][lo:hi] for i, lo, hi in call],
                                 [hi - lo for _, lo, hi in call], 2 * k + 1)
                fisher, grad, ll = self.context.fisher_rows_fields(fields, rows, inv2h, aux=aux)
                at = 0
                for i, lo, hi in call:
                    out = outs[group[i]['f']]
                    out['F'][lo:hi], out['grad'][lo:hi] = fisher[at:at + hi - lo], grad[at:at + hi - lo]
                    out['loglike'][lo:hi] = ll[at:at + hi - lo]
                    at += hi - lo
        for j in jobs:
            outs[j['f']] = _fisher_result(outs[j['f']], j['single'])
        return outs

    def close(self):
        self.context.close()
        for m in self.models:
            m._engine = None               # (views of the context just closed)


def _stack_aux(parts, counts, n_st):
    """The auxiliary rows of a call whose stencils come from several models: parts[i] [counts[i], n_st, n_aux_i] or
    None -> [sum(counts) n_st, widest n_aux] with zeros where a model has no (or shorter) rows; None if none has."""
    if all(p is None for p in parts):
        return None
    width = max(p.shape[-1] for p in parts if p is not None)
    out = np.zeros((sum(counts), n_st, width))
    at = 0
    for p, n in zip(parts, counts):
        if p is not None:
            out[at:at + n, :, :p.shape[-1]] = p
        at += n
    return out.reshape(-1, width)


def _fisher_result(out, single):
    """A fisher() result as it is returned: NaN F and grad for a base where either has a non-finite entry, -inf
    for a non-finite log-likelihood, and no leading axis for a single vector."""
    fisher, grad = out['F'], out['grad']
    bad = ~(np.isfinite(fisher).all(axis=(1, 2)) & np.isfinite(grad).all(axis=1))
    fisher[bad], grad[bad] = np.nan, np.nan
    out['loglike'] = np.where(np.isfinite(out['loglike']), out['loglike'], -np.inf)
    return {key: (val[0] if single and key != 'columns' else val) for key, val in out.items()}



def _same_prior(a, b):
    """The same scipy family with the same args and kwds (vector arguments equal element by element)."""
    ra, rb = getattr(a, 'rv_frozen', None), getattr(b, 'rv_frozen', None)
    if ra is None or rb is None:
        return a is b
    if ra.dist.name != rb.dist.name or len(ra.args) != len(rb.args) or set(ra.kwds) != set(rb.kwds):
        return False
    same = lambda x, y: np.shape(x) == np.shape(y) and np.array_equal(np.asarray(x), np.asarray(y))
    return (all(same(x, y) for x, y in zip(ra.args, rb.args)) and
            all(same(ra.kwds[k], rb.kwds[k]) for k in ra.kwds))


class JointModel(object):
    """ONE model fitted jointly to several exposures of the same object (dithered frames, visits,
    filters): every field keeps its own data, PSFs, noise map, constants and zeropoint, and the
    log-posterior of a joint vector theta is

        ((ll_0(theta_0) + ll_1(theta_1)) + ... + ll_{F-1}(theta_{F-1})) + lnprior(theta)

    with theta_f field f's own vector taken from theta's columns.  The reference has no counterpart (one
    model file per process, psfMC/fitting.py:13-113).

    models     F >= 1 model files or `MultiComponentModel`s with the same component lists (so the same
               `param_names` / `param_lens`) and the same number of PSFs; image and PSF sizes may differ
    per_field  names of `param_names` that each field fits on its own: each becomes F column blocks
               `<name>_f<k>`.  Every other parameter is SHARED (one block, the same value in every field,
               and the same prior in every field).  A PSF index is always per field.

    Joint column order: field 0's `param_names` in order, a shared name once, a per-field name as its F
    blocks in field order.  Every joint column's prior counts once; the Sersic axis-ratio rule applies in
    every field.  Every prior needs a device form.  The linking is checked here without touching the GPU;
    the shared context (`engine.FieldSetContext`, fused back end, f64 storage) is made on first use.
    Capacity: a walker is F field records, so F x W <= max_walkers per batch."""

    def __init__(self, models, per_field=(), max_walkers=4096, device=0):
        models = list(models)
        if not models:
            raise ValueError('a joint fit needs at least one field')
        for m in models:
            if isinstance(m, MultiComponentModel) and (m._storage != 'f64' or m._backend != 'fused'):
                raise ValueError("a joint fit runs on the fused back end with storage='f64' (got backend={!r}, "
                                 "storage={!r})".format(m._backend, m._storage))
        # shallow copies (as FieldSet makes): a model handed in stays what it was
        self.field_models = [copy.copy(m) if isinstance(m, MultiComponentModel) else
                             MultiComponentModel(m, device=device, backend='fused', max_walkers=1) for m in models]
        first = self.field_models[0]
        names, lens = first.param_names, first.param_lens
        n_psf = len(first.config.psf_selector.psf_data)
        for f, m in enumerate(self.field_models):
            if (m.param_names != names or m.param_lens != lens or
                    (len(m._ps), len(m._sersic), len(m._sky)) != (len(first._ps), len(first._sersic), len(first._sky))):
                raise ValueError('field {}: the fields of a joint fit need the same component lists and free '
                                 'parameters ({} against field 0\'s {})'.format(f, m.param_names, names))
            if len(m.config.psf_selector.psf_data) != n_psf:
                raise ValueError('field {} has {} PSFs and field 0 has {}: every field needs the same number of '
                                 'PSFs'.format(f, len(m.config.psf_selector.psf_data), n_psf))
        per_field = set(per_field)
        # ties: a tied attribute has no column to fit per field (its source may be per field), and -- as a shared
        # parameter needs the same prior -- the ties are the same in every exposure
        tie_names = {comp._ties[attr].name for comp, attr, _, _ in first._ties}
        if per_field & tie_names:
            raise ValueError('per_field names {} are tied attributes: a tied attribute follows its source (name the '
                             'source in per_field)'.format(sorted(per_field & tie_names)))

        def tie_key(m):
            out = []
            for comp, attr, src_comp, src_attr in m._ties:
                tie = comp._ties[attr]
                terms = tuple(getattr(tie, t).name if hasattr(getattr(tie, t), 'value') else
                              tuple(float(v) for v in np.ravel(getattr(tie, t))) for t in comp.TIE_TERMS)
                out.append((tie.name, src_comp._priors[src_attr].name) + terms)
            return out
        for f, m in enumerate(self.field_models):
            if tie_key(m) != tie_key(first):
                raise ValueError('field {}: the ties of a joint fit are the same in every field (same source, same '
                                 'ratio and offset); got {} against field 0\'s {}'.format(f, tie_key(m), tie_key(first)))
        unknown = sorted(per_field - set(names))
        if unknown:
            raise ValueError('per_field names {} are not parameters of the model ({})'.format(unknown, names))
        psf_names = [n for c in first.components if isinstance(c, PSFSelector) for n in c.stochastic_names()]
        per_field |= set(psf_names)
        n_f = len(self.field_models)
        self.per_field = sorted(per_field)
        # each field's priors by parameter name, with their device forms
        priors = []
        for f, m in enumerate(self.field_models):
            by_name = {}
            for comp in m.components:
                for attr in comp.free_names():
                    prior = comp._priors[attr]
                    desc = _device_prior(prior, prior.size)
                    if desc is None:
                        raise ValueError('field {}: the prior of {} has no device form; a joint fit evaluates '
                                         'priors on the GPU only'.format(f, prior.name))
                    by_name[prior.name] = (prior, desc)
            priors.append(by_name)
        # joint columns
        own_start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int)
        self._columns = [np.zeros(first.num_params, dtype=np.int64) for _ in range(n_f)]
        self._blocks = []                          # (prior, joint slice, device description)
        j_names, j_lens, pos = [], [], 0
        for name, width, start in zip(names, lens, own_start):
            own = slice(start, start + width)
            if name in per_field:
                for f in range(n_f):
                    prior, desc = priors[f][name]
                    j_names.append('{}_f{}'.format(name, f))
                    j_lens.append(width)
                    self._columns[f][own] = np.arange(pos, pos + width)
                    self._blocks.append((prior, slice(pos, pos + width), desc))
                    pos += width
            else:
                prior, desc = priors[0][name]
                for f in range(1, n_f):
                    if not _same_prior(prior, priors[f][name][0]):
                        raise ValueError('shared parameter {}: field {} has the prior {!r}, field 0 has {!r}; a '
                                         'shared parameter needs the same prior in every field (or make it '
                                         'per_field)'.format(name, f, priors[f][name][0], prior))
                j_names.append(name)
                j_lens.append(width)
                for f in range(n_f):
                    self._columns[f][own] = np.arange(pos, pos + width)
                self._blocks.append((prior, slice(pos, pos + width), desc))
                pos += width
        self._param_names, self._param_lens, self._num_params = j_names, j_lens, pos
        self._family = np.zeros(pos, dtype=np.int32)
        self._prior_params = np.zeros((pos, engine.PRIOR_NPAR))
        for prior, cols, desc in self._blocks:
            width = cols.stop - cols.start
            self._family[cols] = desc[0]
            for j in range(width):
                self._prior_params[cols.start + j] = [np.ravel(v)[j if np.size(v) > 1 else 0] for v in desc[1:]]
        self._device, self._max_walkers = int(device), int(max_walkers)
        self._context = None
        self._host_priors = []             # (DeviceEnsembleSampler: every prior is on the device)

    # -- the shared context ------------------------------------------------------
    @property
    def engine(self):
        """A `engine.JointView` of the fields' shared context, created on first use."""
        if self._context is None:
            fields = []
            for m in self.field_models:
                sel = m.config.psf_selector
                fields.append((m.config.obs_data, m.config.obs_var, m.config.bad_px, np.stack(sel.psf_data),
                               np.stack(sel.psf_var)))
            first = self.field_models[0]
            ctx = engine.FieldSetContext(fields, n_ps=len(first._ps), n_sersic=len(first._sersic),
                                         max_walkers=self._max_walkers, device=self._device)
            try:
                for f, m in enumerate(self.field_models):
                    m._register_layout(ctx.layout_of(f), columns=self._columns[f], n_params=self._num_params)
                ctx.set_joint_priors(self._family, self._prior_params)
            except Exception:
                ctx.close()
                raise
            for f, m in enumerate(self.field_models):
                # the field's images and posterior sums go through ITS field of the shared context
                m._engine = ctx.view(f, self._columns[f])
                m.posterior_images = dict(m.posterior_images)
                m._param_vector = m._param_vector.copy()
                m._max_walkers = self._max_walkers
            self._context = ctx
        return self._context.joint_view()

    @property
    def context(self):
        """The shared `engine.FieldSetContext` (created on first use)."""
        self.engine
        return self._context

    def close(self):
        if self._context is not None:
            self._context.close()
            self._context = None
            for m in self.field_models:
                m._engine = None           # (views of the context just closed)

    # -- parameter vector -----------------------------------------------------------
    @property
    def num_params(self):
        return self._num_params

    @property
    def param_names(self):
        return list(self._param_names)

    @property
    def param_lens(self):
        return list(self._param_lens)

    @property
    def param_fits_abbrs(self):
        return list(self._param_names)

    @property
    def obs_header(self):
        return self.field_models[0].obs_header

    def header_flags(self):
        """`MultiComponentModel.header_flags` over the fields: a key's value is T where every field has the flag
        (pixel-integrated, boxiness, sky slope) -- or, for a valued key (the Fourier mode numbers), the value the
        fields share -- else one letter per field ('TF': field 0 only)."""
        per = [m.header_flags() for m in self.field_models]
        out = {}
        for key in sorted(set().union(*per)):
            marks = ''.join('T' if key in p else 'F' for p in per)
            vals = [p[key] for p in per if key in p]
            same = vals[0] if all(v == vals[0] for v in vals) else True
            out[key] = same if 'F' not in marks else marks
        return out

    @property
    def tie_records(self):
        """`MultiComponentModel.tie_records` of the joint fit (the ties are the same in every field), by the names
        a joint database uses for its columns: [(tied name, source name, ratio, offset)]; a per-field source or
        term stands for its `<name>_f<k>` blocks."""
        first = self.field_models[0]
        out = []
        for comp, attr, src_comp, src_attr in first._ties:
            tie = comp._ties[attr]
            terms = [_tie_term(getattr(tie, t), 'name') for t in comp.TIE_TERMS]
            out.append((tie.name, src_comp._priors[src_attr].name, terms[0], terms[1]))
        return out

    def field_columns(self, f):
        """[P_f] joint column of each of field f's own columns."""
        return self._columns[f].copy()

    def _theta(self, theta):
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim == 1:
            theta = theta[None, :]
        if theta.ndim != 2 or theta.shape[1] != self.num_params:
            raise ValueError('expected [W, {}] joint parameter vectors, got {}'.format(self.num_params, theta.shape))
        return theta

    def field_theta(self, theta, f):
        """[W, P_joint] joint vectors -> [W, P_f] field f's own vectors."""
        return np.ascontiguousarray(self._theta(theta)[:, self._columns[f]])

    def init_params_from_priors(self, nwalkers):
        """Start positions: every joint column block drawn from its prior, redrawn until every field's
        component priors (the axis-ratio rule included) are finite."""
        out = np.zeros((nwalkers, self.num_params))
        for w in range(nwalkers):
            while True:
                for prior, cols, _ in self._blocks:
                    out[w, cols] = np.ravel(prior.random())
                if np.isfinite(self.log_priors_batch(out[w:w + 1])[0]):
                    break
        return out

    # -- priors and posterior ----------------------------------------------------------
    def log_priors_batch(self, theta):
        """[W] joint log-priors with scipy: each joint column's prior once, then every field's Sersic
        axis-ratio rule."""
        theta = self._theta(theta)
        total = np.zeros(theta.shape[0])
        with np.errstate(all='ignore'):
            for prior, cols, _ in self._blocks:
                total = total + prior.logp_batch(theta[:, cols])
            for f, m in enumerate(self.field_models):
                th = theta[:, self._columns[f]]
                resolved = m._resolved(th)                     # once per field ({} for a model without ties)
                for comp, span in zip(m.components, m._spans):
                    if isinstance(comp, Sersic):
                        v = comp.values_batch(th[:, span], resolved.get(id(comp)))
                        total = np.where(v['reff_b'] > v['reff'], -np.inf, total)
        return total

    def log_posterior_batch(self, theta):
        """[W] joint log-posteriors, everything on the device, in slices of max_walkers // F walkers."""
        theta = self._theta(theta)
        eng = self.engine
        cap = max(self._max_walkers // len(self.field_models), 1)
        parts = [eng.logpost_theta(theta[lo:lo + cap]) for lo in range(0, theta.shape[0], cap)]
        return np.concatenate(parts) if parts else np.zeros(0)

    def log_likelihood_and_prior_batch(self, theta):
        """(lnL [W], lnprior [W]) of W joint vectors, the two terms of `log_posterior_batch` apart
        (psfmc_eval_theta_joint_split), in the same slices: lnL is the fields' sum, -inf outside the priors and
        where it is not finite; lnprior the joint log-prior.  The tempered samplers work with these values."""
        theta = self._theta(theta)
        eng = self.engine
        cap = max(self._max_walkers // len(self.field_models), 1)
        parts = [eng.loglike_prior_theta(theta[lo:lo + cap]) for lo in range(0, theta.shape[0], cap)]
        if not parts:
            return np.zeros(0), np.zeros(0)
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    # -- Fisher matrix and gradient ---------------------------------------------------------
    def _check_columns(self, columns):
        """The differentiated joint columns as an array, or ValueError (no device is touched)."""
        from . import mode
        columns = mode.default_columns(self) if columns is None else np.asarray(columns, dtype=np.int64)
        if (columns.ndim != 1 or len(columns) < 1 or columns.min() < 0 or columns.max() >= self.num_params or
                len(set(columns.tolist())) != len(columns)):
            raise ValueError('columns must be a non-empty list of distinct joint columns in [0, {})'.format(
                self.num_params))
        return columns

    def fisher(self, theta, step=None, columns=None):
        """Fisher matrix and gradient of the JOINT log-likelihood (the fields' sum) at theta ([P_joint] or
        [n, P_joint]) over joint columns, from central-difference stencils of device images
        (psfmc_fisher_rows_joint; the definition: `mode.joint_fisher` of the fields' `mode.fisher_from_stencil`).

        columns  the differentiated joint columns (default: every joint column whose prior is not discrete -- every
                 exposure's PSF index stays at the base value)
        step     [K] or [n, K] steps h_k (default: `mode.default_steps`' rule on the joint blocks' priors); the
                 fields that share a column share its step
        Field f's stencil holds the base and the +- vectors of only the joint columns it reads, so a per-field
        column costs two images, not two per field.  Every field must read the same number of `columns` (the
        default's always do), at most 63; their total is limited only by memory.
        Returns dict(F [n, K, K], grad [n, K] (of lnL), loglike [n], columns [K], step [n, K]) in joint terms;
        without the leading axis for a [P_joint] theta.  NaN F and grad where an image is not finite on a good
        pixel, as `MultiComponentModel.fisher`.  `loglike` is `log_likelihood_and_prior_batch`'s lnL of theta, bit
        for bit (one more evaluation of the n base vectors, from raw vectors as the samplers evaluate them): -inf
        outside the priors, where F and grad -- the images do not care about supports -- are still the likelihood's."""
        from . import mode
        single = np.ndim(theta) == 1
        theta = self._theta(theta)
        columns = self._check_columns(columns)
        n, k = theta.shape[0], len(columns)
        if step is None:
            step = mode.default_steps(self, theta, columns)
        step = np.array(np.broadcast_to(np.asarray(step, dtype=np.float64), (n, k)))
        if not np.all(np.isfinite(step) & (step > 0)):
            raise ValueError('steps must be finite and positive')
        place = np.full(self.num_params, -1, dtype=np.int64)       # a joint column's place among `columns`
        place[columns] = np.arange(k)
        own = [np.flatnonzero(place[jc] >= 0) for jc in self._columns]          # the field's own differentiated columns
        col_of = [place[jc[o]] for jc, o in zip(self._columns, own)]
        k_f = len(own[0])
        if k_f < 1 or any(len(o) != k_f for o in own):
            raise ValueError('every field must read the same number (>= 1) of the differentiated columns; the '
                             'fields read {}'.format([len(o) for o in own]))
        n_f, n_st = len(self.field_models), 2 * k_f + 1
        eng = self.engine
        per_call = self._max_walkers // (n_f * n_st)
        if per_call < 1:
            raise ValueError('{} field stencils of {} walkers exceed max_walkers={}'.format(n_f, n_st,
                                                                                           self._max_walkers))
        out = dict(F=np.empty((n, k, k)), grad=np.empty((n, k)), loglike=np.empty(n), columns=columns, step=step)
        for lo in range(0, n, per_call):
            hi = min(lo + per_call, n)
            rows, inv2h, aux = [], [], []
            for f, m in enumerate(self.field_models):
                h = step[lo:hi][:, col_of[f]]
                vecs = mode.stencil(theta[lo:hi][:, self._columns[f]], h, own[f]).reshape(-1, m.num_params)
                rows.append(m.derived_rows(vecs).reshape(hi - lo, n_st, -1))
                a = m.aux_rows(vecs)
                aux.append(None if a is None else np.asarray(a).reshape(hi - lo, n_st, -1))
                inv2h.append(0.5 / h)
            aux_rows = None
            if any(a is not None for a in aux):
                width = max(a.shape[-1] for a in aux if a is not None)
                aux_rows = np.zeros((hi - lo, n_f, n_st, width))
                for f, a in enumerate(aux):
                    if a is not None:
                        aux_rows[:, f, :, :a.shape[-1]] = a
                aux_rows = aux_rows.reshape(-1, width)
            out['F'][lo:hi], out['grad'][lo:hi], _ = eng.fisher_rows(
                np.stack(col_of), np.stack(rows, axis=1), np.stack(inv2h, axis=1), k, aux=aux_rows)
        # (the entry's own lnlike is the sum of the fields' ROW-based log-likelihoods, whose rows the host derives: it
        # sits a rounding apart -- 2e-13 relative, DESIGN.md section 31 -- from the lnL the samplers see)
        out['loglike'] = self.log_likelihood_and_prior_batch(theta)[0]
        return _fisher_result(out, single)

    # -- posterior-image bookkeeping: the device sampler counts samples on the model, every field's sums
    # get each of them -------------------------------------------------------------------
    @property
    def accumulated_samples(self):
        return self.field_models[0].accumulated_samples

    @accumulated_samples.setter
    def accumulated_samples(self, n):
        step = n - self.field_models[0].accumulated_samples
        for m in self.field_models:
            m.accumulated_samples += step

    @property
    def _device_samples(self):
        return self.field_models[0]._device_samples

    @_device_samples.setter
    def _device_samples(self, n):
        step = n - self.field_models[0]._device_samples
        for m in self.field_models:
            m._device_samples += step

    def reset_images(self):
        for m in self.field_models:
            m.reset_images()

    def collect_posterior_images(self):
        """One dict kind -> image per field (`MultiComponentModel.collect_posterior_images`)."""
        return [m.collect_posterior_images() for m in self.field_models]
