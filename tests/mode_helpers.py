"""Shared by tests/test_mode_definition.py, tests/test_fisher_reference.py (CPU) and tests/test_gpu_fisher*.py: the
numpy oracle's images of a central-difference stencil, the definition (`psfmc_amd.mode.fisher_from_stencil`) fed with
them, a mode search driven by oracle callables alone, the error bound of a Fisher matrix whose images carry a given
per-pixel tolerance (`fisher_error_bound`), and the definition in long double with the bound of a correct fp64
evaluation of the SAME images against it (`fisher_reference_longdouble`, `fisher_rounding_bound`)."""
import numpy as np

import helpers
import psfmc_oracle as orc
import synth_field
from psfmc_amd import mode

SYNTH_SIDE = 64
SYNTH_LAYOUT = helpers.synth_layout(1)              # point source + Sersic: K = 10 free columns


def synth_field_64(psf_weight=1.0):
    """(synth field dict, oracle field) of the 64 x 64 point source + Sersic field, seed 0; its PSF weight map times
    `psf_weight` (below 1: a noisier PSF, so that the model's variance counts beside the data's)."""
    fld = synth_field.make_field(SYNTH_SIDE, 1, seed=0)
    if psf_weight != 1.0:
        fld['psf_ivm'] = (fld['psf_ivm'] * psf_weight).astype(fld['psf_ivm'].dtype)
    field = orc.make_field(fld['sci'], fld['ivm'], [fld['psf']], [fld['psf_ivm']], mag_zp=fld['mag_zp'])
    return fld, field


def scale_steps(theta, columns):
    """h_k = 1e-4 max(|theta_k|, 1): the steps of a search that knows no priors."""
    theta = np.atleast_2d(theta)
    return mode.STEP_FRACTION * np.maximum(np.abs(theta[:, columns]), 1.0)


def oracle_images(field, layout, vecs, has_psf_index=False, evaluate=None):
    """The oracle's images of [m, P] vectors: dict of [m, ny, nx] arrays 'conv', 'resid', 'ivm', and 'll' [m].
    evaluate(field, theta) -> (ll, images) replaces the layout-driven oracle call (models with general components)."""
    out = dict(conv=[], resid=[], ivm=[], ll=[])
    for t in vecs:
        if evaluate is None:
            comps, psf = helpers.comps_from_theta(layout, t, has_psf_index)
            ll, imgs = orc.evaluate(field, comps, psf, raw_dtype=np.float64)
        else:
            ll, imgs = evaluate(field, t)
        out['conv'].append(imgs['convolved_model'])
        out['resid'].append(imgs['residual'])
        out['ivm'].append(imgs['composite_ivm'])
        out['ll'].append(ll)
    return {k: np.array(v) for k, v in out.items()}


def oracle_fisher(field, layout, theta, step, columns, has_psf_index=False, evaluate=None):
    """(F, g, images of the stencil) of ONE base vector from the oracle's images."""
    vecs = mode.stencil(theta, step, columns)[0]
    imgs = oracle_images(field, layout, vecs, has_psf_index, evaluate)
    fisher, grad = mode.fisher_from_stencil(imgs['resid'], imgs['ivm'], ~field.bad_px, 0.5 / np.ravel(step))
    return fisher, grad, imgs


def oracle_loglike(field, layout, thetas, has_psf_index=False):
    thetas = np.atleast_2d(thetas)
    with np.errstate(all='ignore'):
        return np.array([helpers.oracle_loglike(field, layout, t, has_psf_index) for t in thetas])


_CPU_MODE = {}


def cpu_mode_search(max_iter=30):
    """The maximum-likelihood point of the 64 x 64 synth field found by `mode.lm_search` on oracle callables alone,
    from a start 30 sigma off the truth in every column (sigma from the Fisher matrix at the truth): computed once
    per process -> dict(result, field, fld, columns, start, sigma)."""
    if 'out' in _CPU_MODE:
        return _CPU_MODE['out']
    fld, field = synth_field_64()
    truth = fld['truth']
    columns = np.arange(len(truth))
    fisher, _, _ = oracle_fisher(field, SYNTH_LAYOUT, truth, scale_steps(truth, columns), columns)
    sigma = np.sqrt(np.diag(np.linalg.inv(fisher)))
    start = truth + 30.0 * sigma * np.where(np.arange(len(truth)) % 2, -1.0, 1.0)

    def curvature(thetas):
        pairs = [oracle_fisher(field, SYNTH_LAYOUT, t, scale_steps(t, columns), columns)[:2] for t in thetas]
        return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])

    result = mode.lm_search(curvature, lambda th: oracle_loglike(field, SYNTH_LAYOUT, th), start, columns,
                            max_iter=max_iter)[0]
    _CPU_MODE['out'] = dict(result=result, field=field, fld=fld, columns=columns, start=start, sigma=sigma)
    return _CPU_MODE['out']


def fisher_error_bound(imgs, field, inv2h, eps_conv, eps_ivm, factor=helpers.RASTER_ORACLE_FACTOR):
    """How far F and g of a stencil may move when every image carries a per-pixel error: |d conv| <= eps_conv,
    |d ivm| <= eps_ivm (absolute, the tolerances tests/test_gpu_parity.py test_images_match_fp64_oracle holds the
    device's convolved model and composite weight map to: 1e-12 of each image's largest finite value).

    First-order propagation through a_k = sqrt(w) dmu_k, b_k = (w / sqrt 2) dv_k, c = sqrt(w) r,
    d = (r^2 w - 1) / sqrt 2, with v = 1 / w so |d v| <= eps_ivm / w^2:
        |d dmu_k| <= 2 eps_conv inv2h_k                      |d dv_k| <= (eps_ivm / w+^2 + eps_ivm / w-^2) inv2h_k
        |d a_k|   <= sqrt(w) |d dmu_k| + |dmu_k| eps_ivm / (2 sqrt w)
        |d b_k|   <= (w |d dv_k| + |dv_k| eps_ivm) / sqrt 2
        |d c|     <= sqrt(w) eps_conv + |r| eps_ivm / (2 sqrt w)
        |d d|     <= (2 |r| w eps_conv + r^2 eps_ivm) / sqrt 2
        |d F_kl|  <= sum (|a_k| |d a_l| + |d a_k| |a_l| + |b_k| |d b_l| + |d b_k| |b_l|)
        |d g_k|   <= sum (|a_k| |d c| + |d a_k| |c| + |b_k| |d d| + |d b_k| |d|)
    evaluated on the oracle's images, normalised like the test's metric -- |dF_kl| / sqrt(F_kk F_ll),
    |dg_k| / sqrt(F_kk) -- and multiplied by the project's factor 4 (helpers.RASTER_ORACLE_FACTOR).
    -> (bound on the normalised F error, bound on the normalised g error), the largest entry of each."""
    good = (~field.bad_px) & np.isfinite(imgs['ivm'][0])
    inv2h = np.asarray(inv2h, dtype=np.float64)[:, None]
    w_all = imgs['ivm'][:, good]
    r = imgs['resid'][0][good]
    w = w_all[0]
    sw = np.sqrt(w)
    dmu = (imgs['conv'][1::2][:, good] - imgs['conv'][2::2][:, good]) * inv2h
    dv = (1.0 / w_all[1::2] - 1.0 / w_all[2::2]) * inv2h
    e_dmu = 2 * eps_conv * inv2h * np.ones_like(dmu)
    e_dv = (eps_ivm / w_all[1::2] ** 2 + eps_ivm / w_all[2::2] ** 2) * inv2h
    a, b = np.abs(sw * dmu), np.abs(w * dv) / np.sqrt(2)
    c, d = np.abs(sw * r), np.abs(r * r * w - 1) / np.sqrt(2)
    e_a = sw * e_dmu + np.abs(dmu) * eps_ivm / (2 * sw)
    e_b = (w * e_dv + np.abs(dv) * eps_ivm) / np.sqrt(2)
    e_c = sw * eps_conv + np.abs(r) * eps_ivm / (2 * sw)
    e_d = (2 * np.abs(r) * w * eps_conv + r * r * eps_ivm) / np.sqrt(2)
    e_f = np.dot(a, e_a.T) + np.dot(e_a, a.T) + np.dot(b, e_b.T) + np.dot(e_b, b.T)
    e_g = np.dot(a, e_c) + np.dot(e_a, c) + np.dot(b, e_d) + np.dot(e_b, d)
    diag = np.sqrt(np.diag(np.dot(a, a.T) + np.dot(b, b.T)))
    return factor * float(np.max(e_f / np.outer(diag, diag))), factor * float(np.max(e_g / diag))


def fisher_reference_longdouble(conv, ivm, sci, good, inv2h):
    """The definition (`psfmc_amd.mode.fisher_from_stencil`) in np.longdouble, from the convolved images and composite
    weight maps [2K+1, ...] of a stencil, the science image and the counted pixels:
        dmu_k = (conv[1+2k] - conv[2+2k]) inv2h_k     dv_k = (1 / ivm[1+2k] - 1 / ivm[2+2k]) inv2h_k
        r = sci - conv[0]      w = ivm[0]
        F_kl = sum_good w dmu_k dmu_l + 1/2 sum_good w^2 dv_k dv_l
        g_k  = sum_good r w dmu_k     + 1/2 sum_good (r^2 w^2 - w) dv_k
    with the pixels whose base weight is not finite left out, as the definition leaves them -> (F [K, K], g [K]) in
    np.longdouble."""
    ld = np.longdouble
    inv2h = np.asarray(inv2h, dtype=ld).ravel()
    n_st = 2 * len(inv2h) + 1
    conv = np.asarray(conv, dtype=np.float64).reshape(n_st, -1)
    ivm = np.asarray(ivm, dtype=np.float64).reshape(n_st, -1)
    good = np.asarray(good, dtype=bool).ravel() & np.isfinite(ivm[0])
    c_all, w_all = conv[:, good].astype(ld), ivm[:, good].astype(ld)
    with np.errstate(all='ignore'):
        v_all = ld(1) / w_all
        r, w = np.asarray(sci, dtype=np.float64).ravel()[good].astype(ld) - c_all[0], w_all[0]
        dmu = (c_all[1::2] - c_all[2::2]) * inv2h[:, None]
        dv = (v_all[1::2] - v_all[2::2]) * inv2h[:, None]
        fisher = np.dot(dmu * w, dmu.T) + np.dot(dv * (w * w), dv.T) / ld(2)
        grad = np.dot(dmu, r * w) + np.dot(dv, r * r * w * w - w) / ld(2)
    return fisher, grad


U64 = 2.0 ** -53                 # unit roundoff of fp64


def fisher_rounding_bound(conv, ivm, sci, good, inv2h, via_residual=False, factor=helpers.RASTER_ORACLE_FACTOR):
    """How far a correct fp64 evaluation of F and g may sit from `fisher_reference_longdouble` of the SAME images:
    the first-order propagation of `fisher_error_bound`, fed per pixel with the roundings that separate the two
    (u = 2^-53; every fp64 operation is taken as correctly rounded, relative error <= u).

    What the device entry (psfmc_fisher.h fisher_entries) reads and does, against what the reference is given:
      conv   `convolved_model` of `sample_images` is a bit copy of the stash: no error.
      w      the kernel's 1 / (mvar0 + obs_var) and the weight map's are both within 2u (sum, reciprocal) of the exact
             reciprocal's neighbourhood: |dw| <= 2u w.  sqrt(w): u from w, u of its own.
      dmu_k  fl(fl(conv+ - conv-) inv2h): 2u |dmu_k|.
      dv_k   the reference recovers v = 1 / ivm from weight maps that carry two roundings each (the sum and the
             reciprocal), the kernel subtracts mvar+ - mvar- directly: |d (v+ - v-)| <= 2u (v+ + v-), then the
             difference's and the product's roundings, 2u |dv_k|.  The first term is the large one: v+ - v- is a
             difference over a 1e-4 step.
      a_k = sqrt(w) dmu_k                   |da_k| <= 5u |a_k|                 (2u dmu, 2u sqrt w, the product)
      b_k = (w fl(1 / sqrt 2)) dv_k         |db_k| <= 7u |b_k| + (w / sqrt 2) 2u (v+ + v-) inv2h_k
                                            (2u w, u the constant, u w2's product, 2u dv, u the product)
      c   = sqrt(w) fl(sci - conv0)         |dc|   <= 4u |c|
      d   = (fl(fl(r r) w) - 1) fl(1/sqrt 2)  |dd| <= (6u r^2 w + 3u |r^2 w - 1|) / sqrt 2
                                            (r^2: 3u, w: 2u, the product: u; the difference, the constant, the product)
    (a fused multiply-add in place of a product and a sum only drops a rounding.)
    via_residual: the float64 definition takes RESIDUAL images, so its dmu_k = -(fl(sci - conv+) - fl(sci - conv-))
    carries u (|r+| + |r-|) inv2h_k more, and its v = fl(1 / ivm) u (v+ + v-) -- inside the 2u above.
      sums   N = 2 n_good products per entry, each rounded, added in fp64 in an unknown order:
             |dF_kl| <= N u sum (|a_k a_l| + |b_k b_l|), |dg_k| <= N u sum (|a_k c| + |b_k d|).
    Then, as in `fisher_error_bound`,
        |dF_kl| <= sum (|a_k| |da_l| + |da_k| |a_l| + |b_k| |db_l| + |db_k| |b_l|) + the sums' term
        |dg_k|  <= sum (|a_k| |dc| + |da_k| |c| + |b_k| |dd| + |db_k| |d|) + the sums' term
    normalised like the test's metric and multiplied by the project's factor 4 (helpers.RASTER_ORACLE_FACTOR).
    -> (bound on the normalised F error, bound on the normalised g error), the largest entry of each."""
    u = U64
    inv2h = np.asarray(inv2h, dtype=np.float64).ravel()[:, None]
    n_st = 2 * len(inv2h) + 1
    conv = np.asarray(conv, dtype=np.float64).reshape(n_st, -1)
    ivm = np.asarray(ivm, dtype=np.float64).reshape(n_st, -1)
    good = np.asarray(good, dtype=bool).ravel() & np.isfinite(ivm[0])
    c_all, w_all = conv[:, good], ivm[:, good]
    v_all = 1.0 / w_all
    sci = np.asarray(sci, dtype=np.float64).ravel()[good]
    r, w = sci - c_all[0], w_all[0]
    sw = np.sqrt(w)
    dmu = (c_all[1::2] - c_all[2::2]) * inv2h
    dv = (v_all[1::2] - v_all[2::2]) * inv2h
    v_sum = (np.abs(v_all[1::2]) + np.abs(v_all[2::2])) * inv2h
    a, b = np.abs(sw * dmu), np.abs(w * dv) / np.sqrt(2)
    c, d = np.abs(sw * r), np.abs(r * r * w - 1) / np.sqrt(2)
    e_a = 5 * u * a
    if via_residual:
        e_a = e_a + sw * u * (np.abs(sci - c_all[1::2]) + np.abs(sci - c_all[2::2])) * inv2h
    e_b = 7 * u * b + w / np.sqrt(2) * 2 * u * v_sum
    e_c = 4 * u * c
    e_d = (6 * u * r * r * w + 3 * u * np.abs(r * r * w - 1)) / np.sqrt(2)
    n_sum = 2 * int(good.sum()) * u
    e_f = (np.dot(a, e_a.T) + np.dot(e_a, a.T) + np.dot(b, e_b.T) + np.dot(e_b, b.T)
           + n_sum * (np.dot(a, a.T) + np.dot(b, b.T)))
    e_g = np.dot(a, e_c) + np.dot(e_a, c) + np.dot(b, e_d) + np.dot(e_b, d) + n_sum * (np.dot(a, c) + np.dot(b, d))
    diag = np.sqrt(np.diag(np.dot(a, a.T) + np.dot(b, b.T)))
    return factor * float(np.max(e_f / np.outer(diag, diag))), factor * float(np.max(e_g / diag))


def variance_share(conv, ivm, good, inv2h):
    """[K] share of the variance half, 1/2 sum w^2 dv_k^2, in F_kk of a stencil's images."""
    inv2h = np.asarray(inv2h, dtype=np.float64).ravel()[:, None]
    n_st = 2 * len(inv2h) + 1
    conv = np.asarray(conv, dtype=np.float64).reshape(n_st, -1)
    ivm = np.asarray(ivm, dtype=np.float64).reshape(n_st, -1)
    good = np.asarray(good, dtype=bool).ravel() & np.isfinite(ivm[0])
    w = ivm[0][good]
    dmu = (conv[1::2][:, good] - conv[2::2][:, good]) * inv2h
    dv = (1.0 / ivm[1::2][:, good] - 1.0 / ivm[2::2][:, good]) * inv2h
    mean, var = np.sum(w * dmu * dmu, axis=1), 0.5 * np.sum(w * w * dv * dv, axis=1)
    return var / (mean + var)


def fisher_errors(fisher, grad, want_f, want_g):
    """The test's metric: (max |dF_kl| / sqrt(F_kk F_ll), max |dg_k| / sqrt(F_kk)) against the definition's F, g."""
    diag = np.sqrt(np.diag(want_f))
    return (float(np.max(np.abs(fisher - want_f) / np.outer(diag, diag))),
            float(np.max(np.abs(grad - want_g) / diag)))
