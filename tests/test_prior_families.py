"""Which priors the library evaluates itself (`models._device_prior`, include/psfmc_hip.h PSFMC_PRIOR_*):
every family of the device table with scalar and per-element parameters, DiscreteUniform with a location,
and what stays on the host.  No GPU needed."""
import numpy as np
import pytest

from psfmc_amd import distributions as D
from psfmc_amd.models import _device_prior

# (prior, width, expected (code, p0, p1, p2, p3))
MAPPED = [
    (D.Uniform(loc=1.0, scale=2.0), 1, (1, 1.0, 2.0, 0.0, 0.0)),
    (D.Normal(loc=20.0, scale=0.5), 1, (2, 20.0, 0.5, 0.0, 0.0)),
    (D.WeibullMinimum(1.5, loc=0.1, scale=2.0), 1, (3, 1.5, 0.1, 2.0, 0.0)),
    (D.DiscreteUniform(0, 3), 1, (4, 0.0, 3.0, 0.0, 0.0)),
    (D.TruncatedNormal(-2.0, 3.0, loc=20.0, scale=0.5), 1, (5, -2.0, 3.0, 20.0, 0.5)),
    (D.LogNormal(0.4, scale=3.0), 1, (6, 0.4, 0.0, 3.0, 0.0)),
    (D.HalfNormal(loc=-0.1, scale=0.05), 1, (7, -0.1, 0.05, 0.0, 0.0)),
    (D.Exponential(scale=0.2), 1, (8, 0.0, 0.2, 0.0, 0.0)),
    (D.Laplace(loc=3.0, scale=0.7), 1, (9, 3.0, 0.7, 0.0, 0.0)),
    (D.Cauchy(loc=21.0, scale=0.3), 1, (10, 21.0, 0.3, 0.0, 0.0)),
    (D.HalfCauchy(loc=0.0, scale=2.0), 1, (11, 0.0, 2.0, 0.0, 0.0)),
    (D.Logistic(loc=-1.0, scale=4.0), 1, (12, -1.0, 4.0, 0.0, 0.0)),
    (D.T(3.0, loc=0.5, scale=2.0), 1, (13, 3.0, 0.5, 2.0, 0.0)),
    (D.Beta(0.5, 2.0, loc=0.3, scale=6.0), 1, (14, 0.5, 2.0, 0.3, 6.0)),
    (D.Reciprocal(0.5, 12.0), 1, (15, 0.5, 12.0, 0.0, 1.0)),
    (D.WeibullMaximum(2.0, loc=1.0, scale=0.5), 1, (16, 2.0, 1.0, 0.5, 0.0)),
    (D.InverseGamma(3.0, loc=0.0, scale=2.0), 1, (17, 3.0, 0.0, 2.0, 0.0)),
]


def _flat(desc):
    return [desc[0]] + [np.ravel(np.asarray(v, dtype=np.float64)).tolist() for v in desc[1:]]


@pytest.mark.parametrize('prior,width,want', MAPPED, ids=[type(m[0]).__name__ for m in MAPPED])
def test_device_families_map_to_their_code(prior, width, want):
    got = _device_prior(prior, width)
    assert got is not None
    assert _flat(got) == _flat(want)


def test_loguniform_is_reciprocal():
    import scipy.stats as st

    class LogUniform(D.ScipyPrior):
        rv_name = 'loguniform'
    prior = LogUniform(1e-2, 1e2, loc=0.5, scale=2.0)
    assert st.loguniform is not st.reciprocal
    assert _flat(_device_prior(prior, 1)) == [15, [1e-2], [1e2], [0.5], [2.0]]


def test_vector_priors_carry_per_element_parameters():
    got = _device_prior(D.TruncatedNormal(-3.0, 3.0, loc=[64.2, 63.1], scale=[0.5, 0.6]), 2)
    assert _flat(got) == [5, [-3.0], [3.0], [64.2, 63.1], [0.5, 0.6]]
    got = _device_prior(D.LogNormal([0.3, 0.5], loc=0.0, scale=[8.0, 5.0]), 2)
    assert _flat(got) == [6, [0.3, 0.5], [0.0], [8.0, 5.0], [0.0]]
    got = _device_prior(D.Beta([2.0, 0.5], 3.0, loc=[0.0, 1.0], scale=2.0), 2)
    assert _flat(got) == [14, [2.0, 0.5], [3.0], [0.0, 1.0], [2.0]]
    # a parameter of neither size 1 nor the vector's width stays on the host
    assert _device_prior(D.Laplace(loc=[1.0, 2.0, 3.0], scale=1.0), 2) is None


def test_discrete_uniform_folds_its_location():
    got = _device_prior(D.DiscreteUniform(0, 3, loc=2), 1)
    assert _flat(got) == [4, [2.0], [5.0], [0.0], [0.0]]
    got = _device_prior(D.DiscreteUniform(-1, 4, loc=[2, -3]), 2)
    assert _flat(got) == [4, [1.0, -4.0], [6.0, 1.0], [0.0], [0.0]]
    # a location that is not an integer stays on the host
    assert _device_prior(D.DiscreteUniform(0, 3, loc=0.5), 1) is None


@pytest.mark.parametrize('prior', [
    D.Gamma(2.0, scale=1.5),                  # a family with no device form
    D.Pareto(2.0),
    D.SkewNormal(1.0),
    D.Poisson(3.0),
], ids=lambda p: type(p).__name__)
def test_other_families_stay_on_the_host(prior):
    assert _device_prior(prior, 1) is None


def _frozen(cls, *args, **kwargs):
    """a prior built without drawing its first value (scipy would reject the parameters)"""
    prior = object.__new__(cls)
    prior.rv_frozen = getattr(__import__('scipy.stats', fromlist=['x']), cls.rv_name)(*args, **kwargs)
    return prior


@pytest.mark.parametrize('cls,args,kwargs', [
    (D.HalfNormal, (), {'scale': 0.0}),
    (D.Exponential, (), {'scale': -1.0}),
    (D.TruncatedNormal, (2.0, 1.0), {}),
    (D.TruncatedNormal, (1.0, 1.0), {}),
    (D.Reciprocal, (2.0, 1.0), {}),
    (D.Reciprocal, (-1.0, 1.0), {}),
    (D.LogNormal, (0.0,), {}),
    (D.Beta, (1.0, -2.0), {}),
    (D.T, (np.inf,), {}),
    (D.InverseGamma, (2.0,), {'loc': np.nan}),
    (D.WeibullMaximum, (2.0,), {'scale': np.inf}),
    (D.Cauchy, (), {'scale': [1.0, -1.0]}),
])
def test_parameters_scipy_rejects_stay_on_the_host(cls, args, kwargs):
    width = max(np.size(v) for v in list(args) + list(kwargs.values()) + [1])
    assert _device_prior(_frozen(cls, *args, **kwargs), width) is None
