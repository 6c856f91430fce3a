"""The rounding-level reference of the Fisher entry, on the CPU: `mode_helpers.fisher_reference_longdouble` (the
definition in np.longdouble) and `mode_helpers.fisher_rounding_bound` (how far a correct fp64 evaluation of the same
images may sit from it), which tests/test_gpu_fisher.py, tests/test_gpu_fisher_paths.py and tests/test_gpu_fisher_fields.py
hold psfmc_fisher_rows to.

Two things are shown on the numpy oracle's images alone.  The bound is not too tight: the float64 definition
(`psfmc_amd.mode.fisher_from_stencil`) lies inside it.  The bound has teeth: numpy mutants of the kernel's per-pixel
form (psfmc_fisher.h fisher_entries), each one plausible mistake, miss the reference by at least 100 x the bound in at
least one case -- a condition on the cases, not a measurement -- while the bound the entry was held to before
(`fisher_error_bound`: the images' 1e-12 parity tolerance propagated) lets most of them through.

Cases: tests/test_gpu_fisher.py's `synth64` and `noisy-psf` (the same field with its PSF weight map times 1e-3, where
the variance half is most of F_kk for some column), and `sky62x66`: sky + point source + Sersic on a 62 x 66 field,
whose sky derivative does not vanish at the last pixels and whose 4092 pixels are not whole slabs of 64.  (The
library takes even sides only, so a pixel count is always a multiple of 4; the hook test reaches the other tails.)"""
import numpy as np
import pytest

import mode_helpers as mh
import test_gpu_fisher as tgf

MUTANT_FACTOR = 100.0            # every mutant misses the reference by at least this many bounds in some case
SKY_SHAPE = (62, 66)
MUTANTS = ['no-bb', 'short-sqrt-half', 'plus-one-in-d', 'w-of-plus', 'last-pixel-dropped', 'last-pixel-twice',
           'window-shifted']


def sky_case():
    return tgf._edge_case(SKY_SHAPE, [dict(type='sky', adu=0.004), tgf._ps(SKY_SHAPE[1], SKY_SHAPE[0]),
                                      tgf._sersic(SKY_SHAPE[1], SKY_SHAPE[0])])


CASES = [('synth64', None), ('noisy-psf', None), ('sky62x66', sky_case)]


@pytest.fixture(scope='module', params=CASES, ids=[c[0] for c in CASES])
def stencil(request):
    name, make = request.param
    return name, _stencil(name, make)


_STENCILS = {}


def _stencil(name, make):
    if name not in _STENCILS:
        _STENCILS[name] = _make_stencil(name, make)
    return _STENCILS[name]


def _make_stencil(name, make):
    ref = tgf.reference(name, make)
    field, imgs = ref['case']['field'], ref['imgs']
    sci, good = np.asarray(field.sci, dtype=np.float64), ~field.bad_px
    inv2h = 0.5 / ref['step'][0]
    args = (imgs['conv'], imgs['ivm'], sci, good, inv2h)
    want = mh.fisher_reference_longdouble(*args)
    return dict(ref=ref, args=args, want=want, bound=mh.fisher_rounding_bound(*args))


def kernel_form(conv, ivm, sci, good, inv2h, mutant=None):
    """F, g in float64 the way psfmc_fisher.h forms them -- per good pixel a_k = sqrt(w) dmu_k, b_k = (w / sqrt 2) dv_k,
    c = sqrt(w) r, d = (r^2 w - 1) / sqrt 2; F = a a^T + b b^T, g = a c + b d -- with one mistake where `mutant` names
    one."""
    inv2h = np.asarray(inv2h, dtype=np.float64).ravel()[:, None]
    shape = np.shape(sci)
    if mutant == 'window-shifted':               # the field's pixels read one column off the stash's
        sci, good = np.roll(sci, -1, axis=1), np.roll(good, -1, axis=1)
    n_st = 2 * len(inv2h) + 1
    conv, ivm = np.reshape(conv, (n_st, -1)), np.reshape(ivm, (n_st, -1))
    good = np.ravel(good) & np.isfinite(ivm[0])
    pix = np.flatnonzero(good)
    last = shape[0] * shape[1] - 1
    assert pix[-1] == last                       # the cases keep their last pixel
    if mutant == 'last-pixel-dropped':
        pix = pix[:-1]
    if mutant == 'last-pixel-twice':
        pix = np.append(pix, last)
    half = 0.7071 if mutant == 'short-sqrt-half' else np.sqrt(0.5)
    w = ivm[0][pix]
    w_k = ivm[1::2][:, pix] if mutant == 'w-of-plus' else w
    r = np.ravel(sci)[pix] - conv[0][pix]
    dmu = (conv[1::2][:, pix] - conv[2::2][:, pix]) * inv2h
    dv = (1.0 / ivm[1::2][:, pix] - 1.0 / ivm[2::2][:, pix]) * inv2h
    a, b = np.sqrt(w_k) * dmu, w_k * half * dv
    c, d = np.sqrt(w) * r, (r * r * w + (1.0 if mutant == 'plus-one-in-d' else -1.0)) * half
    fisher = np.dot(a, a.T) + (0.0 if mutant == 'no-bb' else np.dot(b, b.T))
    return fisher, np.dot(a, c) + np.dot(b, d)


def test_float64_definition_lies_inside_the_bound(stencil):
    """The float64 definition takes residual images, so its bound is the one with `via_residual`; the kernel's form on
    the same images is held to the bound the device is held to."""
    name, st = stencil
    imgs, ref = st['ref']['imgs'], st['ref']
    got = tgf.mode.fisher_from_stencil(imgs['resid'], imgs['ivm'], st['args'][3], st['args'][4])
    assert np.array_equal(got[0], ref['F']) and np.array_equal(got[1], ref['g'])
    err = mh.fisher_errors(got[0], got[1], *st['want'])
    bound = mh.fisher_rounding_bound(*st['args'], via_residual=True)
    print('%s: float64 definition against long double: F %.3g (bound %.3g), g %.3g (bound %.3g)' % (
        (name, err[0], bound[0], err[1], bound[1])))
    assert err[0] <= bound[0] and err[1] <= bound[1]
    assert bound[0] >= st['bound'][0] and bound[1] >= st['bound'][1]
    plain = kernel_form(*st['args'])
    err = mh.fisher_errors(plain[0], plain[1], *st['want'])
    print('%s: float64 kernel form against long double: F %.3g (bound %.3g), g %.3g (bound %.3g); the bound the entry '
          'was held to before: F %.3g, g %.3g' % ((name, err[0], st['bound'][0], err[1], st['bound'][1]) + ref['bounds']))
    assert err[0] <= st['bound'][0] and err[1] <= st['bound'][1]
    # the rounding-level bound is the tighter one by orders of magnitude
    assert st['bound'][0] < 1e-3 * ref['bounds'][0] and st['bound'][1] < 1e-3 * ref['bounds'][1]


def test_cases_meet_their_conditions():
    """Conditions on the oracle's images alone: the variance half carries weight in `noisy-psf`, F is positive
    definite, the sky is differentiated on the field with a slab tail, and its last pixel counts."""
    for name, make in CASES:
        ref = tgf.reference(name, make)
        assert np.linalg.eigvalsh(ref['F']).min() > 0, name
        print('%s: largest variance share %.3g' % (name, ref['share'].max()))
    assert tgf.reference('noisy-psf')['share'].max() >= tgf.MIN_VARIANCE_SHARE
    assert tgf.reference('synth64')['share'].max() < 1e-3
    sky = tgf.reference('sky62x66', sky_case)
    assert sky['case']['layout'][0] == ('sky',) and sky['columns'][0] == 0
    assert (SKY_SHAPE[0] * SKY_SHAPE[1]) % 64 != 0 and not sky['case']['field'].bad_px[-1, -1]
    # the cases of the GPU tests that need no oracle on the device, and the fields of the set
    import test_gpu_fisher_fields as tff
    import test_gpu_fisher_paths as tfp
    tfp.cases_meet_their_conditions()
    for f in range(len(tff.FIELDS)):
        ref = tgf.reference('set-field-%d' % f, tff._make(f))
        assert ref['case']['layout'][0] == ('sky',) and ref['columns'][0] == 0 and len(ref['columns']) == tff.K


@pytest.mark.parametrize('mutant', MUTANTS)
def test_the_bound_has_teeth(mutant):
    best = 0.0
    for name, make in CASES:
        st = _stencil(name, make)
        with np.errstate(all='ignore'):
            got = kernel_form(*st['args'], mutant=mutant)
            err = mh.fisher_errors(got[0], got[1], *st['want'])
        # (a shifted window may put a pixel without a finite weight among the counted ones: NaN, which no bound passes)
        err = tuple(e if np.isfinite(e) else np.inf for e in err)
        ratio = max(err[0] / st['bound'][0], err[1] / st['bound'][1])
        old = st['ref']['bounds']
        print('%-18s %-9s: F off by %.3g, g by %.3g = %.3g x the rounding bound; the old bound (F %.3g, g %.3g) '
              'would %s it' % (mutant, name, err[0], err[1], ratio, old[0], old[1],
                               'catch' if err[0] > old[0] or err[1] > old[1] else 'MISS'))
        best = max(best, ratio)
    assert best >= MUTANT_FACTOR
