"""
Component plugin base -- host glue (parameter containers; rasterisation itself
happens on the GPU).

Keeps the reference's contract (psfMC/ModelComponents/ComponentBase.py):
  * a constructor argument is either a constant or a prior (anything with a
    `.value`; :26-34);
  * free parameters are packed in alphabetical attribute order, each taking
    `size(value)` slots (`xy` -> 2; :45-74, :82-89) -- the emcee vector is the
    concatenation over components in model-file order (models.py:174-185);
  * trace names `<idx>_<Class>_<attr>` and abbreviated FITS names (:99-119);
  * the component log-prior is the sum of its priors' log-probabilities (:121-129).
On top of that every operation has a batch form working on walker columns
`[W, n]`, which is what `BatchLogPosterior` uses.

Not the reference's: an argument may also be a `Tied(source, ratio, offset)`, an
attribute that follows a free parameter of the same model.  A tie is kept apart from
priors and constants; a prior given as its ratio / offset is a free parameter of this
component under the name `<attr>_ratio` / `<attr>_offset`.
"""
import numpy as np


class Tied(object):
    """An attribute that is not independent: value = ratio * source + offset, element by element (GALFIT's
    constraints; not the reference's).  `source` is the prior OBJECT given to another attribute of this or of another
    component of the same model; `ratio` and `offset` are each a number (or one per element) or a prior, which then
    becomes a free parameter of the tied component.  The arithmetic is numpy's `ratio * source + offset`: two
    separately rounded fp64 operations, which the device reproduces to the bit.  A tied attribute has no prior
    term of its own; every support rule reads the resolved value.

        centre = Uniform(loc=(60, 60), scale=(8, 8))
        PointSource(xy=centre, ...)
        Sersic(xy=Tied(centre, offset=Normal(loc=(0, 0), scale=(0.5, 0.5))), ...)
    """

    def __init__(self, source, ratio=1.0, offset=0.0):
        self.source, self.ratio, self.offset = source, ratio, offset
        self.name = ''
        self.fitsname = ''

    @staticmethod
    def resolve(source, ratio, offset):
        """The definition: product, then sum, each rounded once."""
        return np.asarray(ratio, dtype=np.float64) * np.asarray(source, dtype=np.float64) + \
            np.asarray(offset, dtype=np.float64)

    @staticmethod
    def _current(term):
        return term.value if hasattr(term, 'value') else term

    @property
    def value(self):
        """The resolved value at the current values of the source and of a ratio / offset prior."""
        out = Tied.resolve(Tied._current(self.source), Tied._current(self.ratio), Tied._current(self.offset))
        return out.item() if out.size == 1 else out

    @property
    def size(self):
        return int(np.size(Tied._current(self.source)))

    def __repr__(self):
        return 'Tied({!r}, ratio={!r}, offset={!r})'.format(self.source, self.ratio, self.offset)


class StochasticProperty(object):
    """Descriptor declaring an attribute that may hold a prior or a constant
    (reference: ComponentBase.py:132-153).  `xy = StochasticProperty()` or
    `StochasticProperty('xy')`."""

    def __init__(self, key=None):
        self.key = key

    def __set_name__(self, owner, name):
        if self.key is None:
            self.key = name
        declared = list(getattr(owner, '_declared', ()))
        if self.key not in declared:
            declared.append(self.key)
        owner._declared = tuple(declared)

    def __get__(self, obj, owner=None):
        if obj is None:
            return self
        return obj.get_stochastic_val(self.key)

    def __set__(self, obj, value):
        obj.assign_stochastic(self.key, value)

    def __delete__(self, obj):
        raise NotImplementedError('Cannot delete stochastics')


class ComponentBase(object):
    _fits_abbrs = []
    _declared = ()
    #: rasteriser kind understood by the GPU path ('sky', 'ps', 'sersic') or None
    device_kind = None

    #: attributes that are vectors: their width (every other attribute is a scalar)
    _widths = {'xy': 2, 'slope': 2}
    TIE_TERMS = ('ratio', 'offset')

    def __init__(self):
        self._priors = {}
        self._constants = {}
        self._ties = {}

    # -- storage ----------------------------------------------------------
    def assign_stochastic(self, name, value):
        if name in getattr(self, '_ties', {}):               # (the attribute is given anew: its tie goes)
            del self._ties[name]
            for term in self.TIE_TERMS:
                self._priors.pop('{}_{}'.format(name, term), None)
        if isinstance(value, Tied):
            self.__dict__.setdefault('_ties', {})[name] = value
            self._priors.pop(name, None)
            self._constants.pop(name, None)
            for term in self.TIE_TERMS:
                if hasattr(getattr(value, term), 'value'):
                    self._priors['{}_{}'.format(name, term)] = getattr(value, term)
        elif hasattr(value, 'value'):
            self._constants.pop(name, None)
            self._priors[name] = value
        else:
            self._priors.pop(name, None)
            self._constants[name] = value

    def get_stochastic_val(self, name):
        if name in self._priors:
            return self._priors[name].value
        if name in self._ties:
            return self._ties[name].value
        return self._constants[name]

    def attr_width(self, name):
        return self._widths.get(name, 1)

    def get_distribution(self, stoch_name):
        hits = [p for p in self._priors.values() if p.name == stoch_name]
        if len(hits) != 1:
            raise KeyError('Could not find unique prior with name: {}'
                           .format(stoch_name))
        return hits[0]

    # -- packing contract --------------------------------------------------
    def free_names(self):
        return sorted(self._priors)

    def stochastic_lens(self):
        return [self._priors[k].size for k in self.free_names()]

    def num_stochastics(self):
        return int(sum(self.stochastic_lens()))

    def stochastic_names(self, name_attr='name'):
        return [getattr(self._priors[k], name_attr) for k in self.free_names()]

    def update_stochastic_names(self, count=None):
        kind = type(self).__name__
        named = list(self._priors.items()) + list(self._ties.items())
        for attr, prior in named:
            # a tie's ratio / offset prior: the attribute's names with `_ratio` / `_offset`, short form the
            # attribute's without its underscore and an R / O (at most 8 characters, as the attribute's own)
            base, term = attr, None
            for t in self.TIE_TERMS:
                if attr.endswith('_' + t) and attr[:-len(t) - 1] in self._ties:
                    base, term = attr[:-len(t) - 1], t
            long_name = '{}_{}'.format(kind, base)
            short = long_name
            for word, abbr in type(self)._fits_abbrs:
                short = short.replace(word, abbr)
            if term is not None:
                long_name = '{}_{}'.format(long_name, term)
                short = short.replace('_', '', 1) + term[0].upper()
            if count is not None:
                long_name = '{:d}_{}'.format(count, long_name)
                short = '{:d}{}'.format(count, short)
            prior.name = long_name
            prior.fitsname = short

    def set_stochastic_values(self, param_values='random'):
        """Vector of this component's free values, or 'random' / 'median' to
        take them from the priors.  Returns the vector that was set."""
        names = self.free_names()
        if isinstance(param_values, str):
            how = param_values
            parts = [np.ravel(getattr(self._priors[k], how)()) for k in names]
            param_values = (np.concatenate(parts) if parts
                            else np.zeros(0))
        pos = 0
        for k, width in zip(names, self.stochastic_lens()):
            self._priors[k].value = np.array(param_values[pos:pos + width])
            pos += width
        return param_values

    def log_priors(self):
        total = 0
        for prior in self._priors.values():
            total += np.sum(prior.logp(prior.value))
        return total

    # -- batch forms --------------------------------------------------------
    def _columns(self):
        pos, cols = 0, {}
        for k, width in zip(self.free_names(), self.stochastic_lens()):
            cols[k] = slice(pos, pos + width)
            pos += width
        return cols

    def free_values_batch(self, block):
        """[W, num_stochastics] walker columns -> {packed name: [W] or [W, k]} for every free parameter, the
        ratio / offset priors of the ties among them."""
        block = np.asarray(block, dtype=np.float64)
        return {k: self._priors[k].coerce(block[:, cols]) for k, cols in self._columns().items()}

    def values_batch(self, block, resolved=None):
        """[W, num_stochastics] walker columns -> {attr: [W] or [W, k]} for
        every declared attribute, constants broadcast.  resolved: {attr: values} of this component's tied
        attributes, which the model resolves (`MultiComponentModel.tied_values`: the source may belong to another
        component)."""
        block = np.asarray(block, dtype=np.float64)
        n_w = block.shape[0]
        cols = self._columns()
        out = {}
        for k in self._declared:
            if k in self._priors:
                out[k] = self._priors[k].coerce(block[:, cols[k]])
            elif k in self._ties:
                if resolved is None or k not in resolved:
                    raise ValueError('{}: the tied attribute {!r} is resolved by the model (values_batch needs '
                                     '`resolved`)'.format(type(self).__name__, k))
                out[k] = resolved[k]
            elif k in self._constants:
                const = np.asarray(self._constants[k], dtype=np.float64)
                out[k] = np.broadcast_to(const, (n_w,) + const.shape)
        return out

    def log_priors_batch(self, block, resolved=None):
        """[W, num_stochastics] -> [W] joint log-prior of this component (resolved: as for `values_batch`; the
        base class sums the free parameters' priors and does not need it)."""
        block = np.asarray(block, dtype=np.float64)
        total = np.zeros(block.shape[0])
        for k, cols in self._columns().items():
            total = total + self._priors[k].logp_batch(block[:, cols])
        return total
