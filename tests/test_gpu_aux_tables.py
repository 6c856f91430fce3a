"""A field's auxiliary table is rebuilt from the host record of what the field registered (csrc/psfmc_aux_table.h):
replaying registrations on a live context, the drop rules of include/psfmc_hip.h, refused calls and the context's
aux_stride.  One 64x64 field, four walkers at most; every comparison is bit for bit between contexts of one process."""
import numpy as np
import pytest

import test_radial_laws as trl
from test_gpu_general_components import make_field
from test_gpu_radial_laws import TWO, build, named, vector
from psfmc_amd.ModelComponents import Moffat, Sersic

pytestmark = pytest.mark.gpu

# a boxy Moffat with two free modes and a free spiral: base, Fourier, spiral and radial entries, all registered
FULL = [(Moffat, dict(angle='free', boxiness='free', fourier=TWO,
                      spiral=dict(r_in='free', r_out='free', winding='free', inclination=35.0, sky_angle=20.0)))]
CALLS = {'layout': 'set_layout', 'priors': 'set_priors', 'aux': 'set_aux_layout', 'fourier': 'set_fourier_layout',
         'spiral': 'set_spiral_layout', 'radial': 'set_radial_layout'}


def full_model(fld):
    model = build(fld, FULL, max_walkers=4)
    rec = trl.RecordingLayout()
    model._register_layout(rec)                       # the model's own registration calls, as it made them
    assert [c[0] for c in rec.calls] == ['layout', 'aux', 'fourier', 'spiral', 'radial']
    return model, rec.calls


def full_thetas(model, fld):
    rows = [dict(angle=30.0, beta=2.5, boxiness=0.4, f2_amp=0.2, f2_phase=30.0, f3_amp=0.1, fwhm=6.0, fwhm_b=4.0, mag=18.0,
                 spiral_r_in=2.0, spiral_r_out=10.0, spiral_wind=150.0, xy=(32.3, 30.8)),
            dict(angle=-20.0, beta=6.0, boxiness=-0.5, f2_amp=-0.1, f2_phase=-50.0, f3_amp=0.2, fwhm=8.0, fwhm_b=3.0,
                 mag=18.6, spiral_r_in=0.0, spiral_r_out=6.0, spiral_wind=-200.0, xy=(29.3, 34.2)),
            dict(angle=75.0, beta=1.2, boxiness=1.3, f2_amp=0.15, f2_phase=100.0, f3_amp=-0.2, fwhm=5.0, fwhm_b=4.5,
                 mag=18.9, spiral_r_in=1.0, spiral_r_out=15.0, spiral_wind=60.0, xy=(33.5, 31.5))]
    return np.array([vector(model, fld, named(2, 'Moffat', **r)) for r in rows])


def replay(model, calls, names):
    for name, args in calls:
        if name in names:
            getattr(model.engine, CALLS[name])(*args)


def test_replaying_the_registrations_on_a_live_context():
    fld = make_field(64, 64, seed=21)
    model, calls = full_model(fld)
    thetas = full_thetas(model, fld)
    lp0 = model.log_posterior_batch(thetas)
    assert np.all(np.isfinite(lp0)) and len(np.unique(lp0)) == 3
    replay(model, calls, ('fourier', 'spiral', 'radial'))
    assert np.array_equal(model.log_posterior_batch(thetas), lp0)
    replay(model, calls, CALLS)
    assert np.array_equal(model.log_posterior_batch(thetas), lp0)
    model.close()


def test_the_drop_rules_of_the_header():
    fld = make_field(64, 64, seed=21)
    a, calls = full_model(fld)
    b, _ = full_model(fld)
    thetas = full_thetas(a, fld)
    lp0 = a.log_posterior_batch(thetas)
    assert np.array_equal(b.log_posterior_batch(thetas), lp0)
    replay(a, calls, ('fourier',))                                    # a Fourier layout drops spirals and laws
    b.engine.set_spiral_layout([False], [-1] * 6, [0.0, 1.0, 0.0, 0.0, 0.0, 0.0])     # removes spirals, drops laws
    got_a, got_b = a.log_posterior_batch(thetas), b.log_posterior_batch(thetas)
    print('all blocks', lp0, 'modes only', got_a)
    assert np.all(np.isfinite(got_a)) and np.array_equal(got_a, got_b)
    assert np.all(got_a != lp0)
    replay(a, calls, ('spiral', 'radial'))
    assert np.array_equal(a.log_posterior_batch(thetas), lp0)
    a.close()
    b.close()


def test_a_refused_call_changes_nothing():
    from psfmc_amd.engine import NativeError
    fld = make_field(64, 64, seed=21)
    model, _ = full_model(fld)
    eng, n_par = model.engine, model.num_params
    thetas = full_thetas(model, fld)
    lp0 = model.log_posterior_batch(thetas)
    inside = [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    refused = [('mode', lambda: eng.set_fourier_layout([1 << 6], [-1] * 12, [0.0] * 12)),
               ('column', lambda: eng.set_fourier_layout([1], [n_par] + [-1] * 11, [0.0] * 12)),
               ('column', lambda: eng.set_spiral_layout([True], [n_par] + [-1] * 5, inside)),
               ('n_sersic', lambda: eng.set_spiral_layout([True, False], [-1] * 12, inside * 2)),
               ('kind', lambda: eng.set_radial_layout([3], [-1] * 2, [2.0, 0.0])),
               ('kind', lambda: eng.set_radial_layout([-1], [-1] * 2, [2.0, 0.0])),
               ('n_sersic', lambda: eng.set_radial_layout([1, 0], [-1] * 4, [2.0, 0.0] * 2)),
               ('column', lambda: eng.set_radial_layout([1], [n_par, -1], [2.0, 0.0]))]
    for match, call in refused:
        with pytest.raises(NativeError, match=match):
            call()
        assert np.array_equal(model.log_posterior_batch(thetas), lp0), match
    model.close()


def test_aux_stride_and_a_law_that_comes_and_goes():
    """A model with an aux layout and no blocks computes the same before a law is registered and after it is
    removed, although the context's auxiliary vectors have grown for good."""
    fld = make_field(64, 64, seed=21)
    plain = build(fld, [(Sersic, {})], max_walkers=4)
    assert plain.engine.get_option('aux_stride') == 0
    plain.close()
    model = build(fld, [(Sersic, dict(boxiness='free'))], max_walkers=4)
    n_sky, n_ser = 1, 1
    eng = model.engine
    assert eng.get_option('aux_stride') == 2 * n_sky + n_ser
    thetas = np.array([vector(model, fld, named(2, 'Sersic', boxiness=c, index=n, mag=18.5, reff=5.0, reff_b=3.5,
                                                xy=(32.3, 30.8))) for c, n in ((0.3, 1.0), (-0.4, 2.5), (1.2, 4.0))])
    lp0 = model.log_posterior_batch(thetas)
    assert np.all(np.isfinite(lp0))
    eng.set_radial_layout([1], [-1, -1], [2.5, 0.0])                  # a Moffat of beta 2.5 in the slot
    assert eng.get_option('aux_stride') == 2 * n_sky + 21 * n_ser
    law = model.log_posterior_batch(thetas)
    assert np.all(np.isfinite(law)) and np.all(law != lp0)
    eng.set_radial_layout([0], [-1, -1], [0.0, 0.0])
    assert eng.get_option('aux_stride') == 2 * n_sky + 21 * n_ser
    assert np.array_equal(model.log_posterior_batch(thetas), lp0)
    model.close()
