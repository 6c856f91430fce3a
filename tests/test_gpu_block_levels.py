"""The seven forms a context's general launches take -- no block, modes only, a spiral only, modes and a spiral, a radial
law, a truncation, bending modes -- each registered on FIELD 1 ALONE of a two-field context (fused back end, 64 x 64, two Sersic
slots, 8 walkers per field), so that the per-field state is read at an index above 0 and the context carries exactly
the level's blocks.  Field 0 keeps a plain boxy Sersic.

Per level: field 1 against the contract of tests/extra_contract.py at the bounds the project holds these features to
(the raw model per pixel at `RAW_BOUND`, the log-posterior at 1e-9 |ll|); field 0 bit for bit against a context that
never saw a block; then field 1's aux layout is registered again, which drops its blocks while the context keeps their
buffers, and field 1 equals bit for bit the same layout in a context that never saw a block; last, posterior sums
of field 1 alone leave the counts (0, 8)."""
import numpy as np
import pytest

import extra_contract as xc
from test_gpu_general_components import RAW_BOUND
from psfmc_amd.models import FieldSet

pytestmark = pytest.mark.gpu

SHAPE, N_W = (64, 64), 8
MODES = {1: (0.2, 30.0), 3: (-0.15, 25.0)}
ARMS = dict(r_in=2.0, r_out=9.0, winding=150.0, inclination=35.0, sky_angle=20.0)
BOXY = [dict(boxiness=xc.FREE), {}]
# the first Sersic slot of field 1; every keyword's values are constants, so every level but the law has field 0's
# free parameters name for name, and the Moffat (beta free in the place of the index) as many
LEVELS = {
    'none': dict(boxiness=xc.FREE),
    'modes': dict(boxiness=xc.FREE, fourier=MODES),
    'spiral': dict(boxiness=xc.FREE, spiral=ARMS),
    'modes+spiral': dict(boxiness=xc.FREE, fourier=MODES, spiral=ARMS),
    'law': dict(boxiness=xc.FREE, law='moffat'),
    'truncation': dict(boxiness=xc.FREE, truncation={'outer': (9.0, 14.0)}),
    'bending': dict(boxiness=xc.FREE, bending={2: 0.2, 3: -0.1}),
}
BLOCK_CALLS = ('set_fourier_layout', 'set_spiral_layout', 'set_radial_layout', 'set_truncation_layout',
               'set_bending_layout')


class WithoutBlocks(object):
    """A field's layout calls passed on, the block registrations left out."""

    def __init__(self, layout):
        self._layout = layout

    def __getattr__(self, name):
        return (lambda *args: None) if name in BLOCK_CALLS else getattr(self._layout, name)


class AuxCall(object):
    """Keeps the arguments of a model's `set_aux_layout`; every other layout call is dropped."""
    args = None

    def set_aux_layout(self, *args):
        self.args = args

    def __getattr__(self, name):
        return lambda *args: None


@pytest.fixture(scope='module')
def cases():
    return [xc.field_case(SHAPE, seed, n_psf=1) for seed in (41, 42)]


def thetas(model):
    return np.array([xc.theta_of(model, *xc.scene(SHAPE, i)) for i in range(N_W)])


def field_set(cases, spec):
    return FieldSet([xc.make_model(cases[0], BOXY, max_walkers=1),
                     xc.make_model(cases[1], [spec, {}], max_walkers=1)], max_walkers=2 * N_W)


@pytest.mark.parametrize('level', list(LEVELS))
def test_a_level_on_field_1_alone(cases, level):
    fs = field_set(cases, LEVELS[level])
    model = fs.models[1]
    both = [thetas(fs.models[0]), thetas(model)]
    # the same two layouts in a context that never saw a block
    plain = field_set(cases, LEVELS['none'])
    model._register_layout(WithoutBlocks(plain.context.layout_of(1)))
    want0, want1 = plain.log_posterior_batch(both)
    plain.close()
    assert np.all(np.isfinite(want0)) and np.all(np.isfinite(want1))

    got0, got1 = fs.log_posterior_batch(both)
    raw = model.sample_images(both[1][:2], ('raw_model',))['raw_model']
    assert np.array_equal(got0, want0)                             # field 0, bit for bit
    assert (level == 'none') == bool(np.array_equal(got1, want1))  # (the level changes field 1)
    field = xc.oracle_field(cases[1])
    prior = model.log_priors_batch(both[1])
    for i, t in enumerate(both[1]):
        ll, images = xc.contract_evaluate(model, field, t)
        assert np.isfinite(ll) and np.isfinite(prior[i])
        print('%s walker %d: log-posterior %.6f, relative error %.2e' % (level, i, got1[i],
                                                                         abs(got1[i] - (ll + prior[i])) / abs(ll)))
        assert abs(got1[i] - (ll + prior[i])) <= 1e-9 * abs(ll), (level, i, got1[i], ll + prior[i])
        if i < 2:
            err = xc.raw_error(raw[i], images['raw_model'], (level, i))
            print('%s walker %d: raw model max relative error %.2e' % (level, i, err))
            assert err <= RAW_BOUND, (level, i, err)

    # the aux layout again: field 1's blocks go, the context keeps their buffers
    call = AuxCall()
    model._register_layout(call)
    fs.context.layout_of(1).set_aux_layout(*call.args)
    again0, again1 = fs.log_posterior_batch(both)
    assert np.array_equal(again0, want0) and np.array_equal(again1, want1)

    fs.context.accumulate_theta(1, both[1])
    assert (fs.context.accumulated(0)[1], fs.context.accumulated(1)[1]) == (0, N_W)
    fs.close()
