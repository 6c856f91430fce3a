/*
 * psfmc_hip.h -- C ABI of libpsfmc_hip.so: the MI355X (gfx950) implementation of
 * psfMC's per-sample log-likelihood, batched over ensemble-sampler walkers.
 *
 * Drop-in boundary.  The reference evaluates one walker at a time inside
 *   MultiComponentModel.log_posterior          psfMC/models.py:193-243
 * which emcee reaches through `lnpostfn` / `pool.map` (psfMC/fitting.py:56-58).
 * Everything below the prior early-out (models.py:213-241) is replaced by
 * psfmc_eval_batch(); the one-time setup that feeds it (Configuration.py:41-52,
 * PSFSelector.py:32-43, utils.py:9-22 `pad_and_rfft_image`, :126-133
 * `pre_fft_psf`) is replaced by psfmc_ctx_create().  The Python host side
 * (psfmc_amd/engine.py) binds these entry points with ctypes; see INTEGRATION.md
 * for the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; caller owns every host buffer for the
 *     duration of the call; the context owns all device memory.
 *   - return 0 on success, a negative PSFMC_E* code otherwise, message in
 *     psfmc_last_error().  Numeric trouble is never an error: a NaN / inf
 *     log-likelihood is written to the output and the host maps it to -inf
 *     (psfMC/models.py:238-241).
 *   - a context is bound to one device and is not thread-safe.
 *   - images are row-major [ny][nx], x = column index = fastest axis, pixel
 *     centres at integer coordinates (psfMC/utils.py:35-42).  ny and nx must
 *     be even (psfMC/models.py:276 is broken for odd sizes too).
 */
#ifndef PSFMC_HIP_H
#define PSFMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psfmc_ctx psfmc_ctx;

/* error codes */
#define PSFMC_OK            0
#define PSFMC_EINVAL       -1   /* bad argument / unsupported shape        */
#define PSFMC_EHIP         -2   /* HIP runtime / hipFFT failure            */
#define PSFMC_ENOMEM       -3
#define PSFMC_ENODEV       -4   /* no usable gfx950 device                 */

/* convolution back ends (both run entirely on the GPU) */
#define PSFMC_BACKEND_FUSED   0  /* hand-written LDS FFT fused with rasteriser / spectral multiply / chi^2.
                                    BUILT sides: the rows of psfmc_amd/csrc/psfmc_sides.h (the powers of two
                                    64..2048, 1152, 1280, 1536 and the even sides up to 960 with factors 3, 5, 7, 11
                                    and 13 listed there; psfmc_amd/engine.py FUSED_SIDES is the same list)
                                    (nx and ny independently, any combination).  Any OTHER even side is EMBEDDED
                                    (round 3): it runs on the kernels of a built side >= side + PSF side - 1 of
                                    that axis (overlap-save; every array at this boundary keeps the image's own
                                    shape).  psfmc_ctx_create returns PSFMC_EINVAL only for odd sides and for an
                                    unbuilt side with side + PSF side - 1 above the largest built side */
#define PSFMC_BACKEND_HIPFFT  1  /* batched hipFFT D2Z/Z2D between separate kernels: any even shape
                                    (psfMC/utils.py:25-32 accepts those); also the cross-check path */

/* point-source shift methods (psfMC/ModelComponents/PointSource.py:40-51) */
#define PSFMC_PS_LANCZOS3   0
#define PSFMC_PS_BILINEAR   1

/*
 * Per-walker derived-parameter row (doubles), length psfmc_row_len():
 *   [0]                      sky level, ADU                      (Sky.py:14-16)
 *   per point source  (4):   flux, x0, y0, method                (PointSource.py:24-57; flux = utils.py:160-164)
 *   per Sersic        (9):   x0, y0, m00, m01, m10, m11, kappa, p, sb_eff
 *                            (M = inverse scale * inverse rotation, Sersic.py:80-91;
 *                             kappa = gammaincinv(2n, 1/2), Sersic.py:47-53; p = 0.5/n,
 *                             Sersic.py:121; sb_eff Sersic.py:55-71)
 *   [last]                   psf index (already rounded; PSFSelector.py:54-66)
 * Component groups are summed in the order sky, point sources, Sersics.
 */
#define PSFMC_ROW_SKY      1
#define PSFMC_ROW_PS       4
#define PSFMC_ROW_SERSIC   9

/*
 * Create a context for one observed field.
 *   sci, obs_var, bad_px  [ny][nx]  Configuration.obs_data / obs_var / bad_px
 *                                   (Configuration.py:44-46; obs_var = +inf at bad pixels,
 *                                   utils.py:68-70; bad_px nonzero = excluded from the sum)
 *   psf, psf_var          [n_psf][psf_ny][psf_nx]  normalised PSFs and their variance maps
 *                                   as returned by preprocess_psf / calculate_psf_variability
 *                                   (utils.py:106-157).  They are centre-padded to [ny][nx]
 *                                   at offset pad/2 and Fourier transformed ON THE DEVICE
 *                                   (replaces utils.py:9-22, :126-133).
 *   n_ps, n_sersic        component counts of the model (fixed per context)
 *   max_walkers           largest W a later call may pass
 */
int psfmc_ctx_create(psfmc_ctx** out, int device, int ny, int nx,
                     const double* sci, const double* obs_var, const uint8_t* bad_px,
                     int n_psf, int psf_ny, int psf_nx,
                     const double* psf, const double* psf_var,
                     int n_ps, int n_sersic, int max_walkers, int backend);

int psfmc_ctx_destroy(psfmc_ctx* ctx);

/* doubles per walker row: 2 + 4*n_ps + 9*n_sersic */
int psfmc_row_len(const psfmc_ctx* ctx);

/*
 * Walkers per internal pass the library uses for a batch of W walkers (the batch is
 * evaluated as ceil(W / pass) passes of at most this size; per-walker results do not depend
 * on it).  For tests that place known vectors at pass boundaries and for profiling scripts
 * that normalise per-launch counters; there is no reference counterpart.  < 0 on error.
 */
int psfmc_pass_size(const psfmc_ctx* ctx, int W);

/*
 * Log-likelihood of W walkers (models.py:213-216, 233-236 for each):
 *   loglike[w] = -0.5 * sum_{good px} ( resid^2 * ivm - ln(ivm / 2pi) )
 * rows [W][row_len] and skip [W] (nonzero = prior was not finite: the walker is
 * not evaluated and gets -inf, models.py:208-211; may be NULL) are HOST buffers;
 * the call returns after loglike[W] has been copied back.
 */
int psfmc_eval_batch(psfmc_ctx* ctx, int W, const double* rows,
                     const uint8_t* skip, double* loglike);

/*
 * Same, with DEVICE pointers, enqueued on `stream` (a hipStream_t, NULL = the
 * context's own stream) and not synchronised: for callers that keep walkers
 * resident in HBM (bench.py, the multi-GPU all-gather path).
 */
int psfmc_eval_batch_device(psfmc_ctx* ctx, int W, const double* d_rows,
                            const uint8_t* d_skip, double* d_loglike, void* stream);

/*
 * The five per-sample images of models.py:222-226 for W walkers, each
 * [W][ny][nx] host output or NULL: raw_model (models.py:245-253),
 * convolved_model (:255-263), residual (:282-294), composite_ivm (:265-280),
 * point_source_subtracted (:296-306).
 */
int psfmc_eval_images(psfmc_ctx* ctx, int W, const double* rows,
                      double* raw, double* conv, double* resid, double* ivm,
                      double* ps_sub);

/*
 * Raw emcee parameter vectors on the device: with the model's parameter layout and
 * its priors registered, psfmc_eval_theta computes the complete log-posterior
 * (models.py:193-243) of W vectors without any host arithmetic -- joint log-prior
 * (distributions.py:112-127 for the families below, Sersic.py:41-45), early-out,
 * Sersic kappa = gammaincinv(2n, 1/2) and Sigma_e (Sersic.py:47-71), flux
 * (utils.py:160-164), ellipse matrix (Sersic.py:80-91), likelihood, NaN -> -inf.
 *
 * Slots, in this order: n_sky x [adu] | n_ps x [mag, x, y] | n_sersic x [angle, index,
 * mag, reff, reff_b, x, y] | [psf_index].  slot_col[i] is the column of the vector that
 * feeds slot i (packing contract of ComponentBase.py:45-74 / models.py:174-185) or -1
 * for a constant slot_const[i].
 * Prior families per vector column: 0 = evaluated by the host (passed per walker in
 * `extra_lnprior`), 1 uniform(loc=p0, scale=p1), 2 normal(loc=p0, scale=p1),
 * 3 weibull_min(c=p0, loc=p1, scale=p2), 4 randint(low=p0, high=p1) on the rounded value.
 * psfmc_set_layout accepts families 0-4 only; psfmc_set_priors then replaces the whole table.
 */
#define PSFMC_PRIOR_HOST         0
#define PSFMC_PRIOR_UNIFORM      1
#define PSFMC_PRIOR_NORMAL       2
#define PSFMC_PRIOR_WEIBULL_MIN  3
#define PSFMC_PRIOR_RANDINT      4
int psfmc_set_layout(psfmc_ctx* ctx, int n_sky, int n_params, const int* slot_col,
                     const double* slot_const, const int* ps_method, const int* sersic_degrees,
                     double mag_zeropoint, const int* family, const double* p0, const double* p1,
                     const double* p2);
/*
 * The full prior table of field `field` (0 for a one-field context), after psfmc_set_layout[_field]:
 * family [n_params], params [n_params][PSFMC_PRIOR_NPAR] = the scipy.stats arguments in the order below,
 * unused trailing entries ignored.  Each column's log-density is scipy's frozen logpdf (logpmf for
 * randint) of the column's value: the same support, closed or open as scipy's (lognorm and invgamma
 * open, the rest closed), so that the support's edges and the values one ulp on either side give scipy's
 * result (-inf, a finite value or +inf); NaN gives NaN, and the walker is skipped.
 *    0 host                                   1 uniform (loc, scale)
 *    2 norm (loc, scale)                      3 weibull_min (c, loc, scale)
 *    4 randint (low, high) -- a location is folded in: (low + loc, high + loc)
 *    5 truncnorm (a, b, loc, scale)           6 lognorm (s, loc, scale)
 *    7 halfnorm (loc, scale)                  8 expon (loc, scale)
 *    9 laplace (loc, scale)                  10 cauchy (loc, scale)
 *   11 halfcauchy (loc, scale)               12 logistic (loc, scale)
 *   13 t (df, loc, scale)                    14 beta (a, b, loc, scale)
 *   15 reciprocal = loguniform (a, b, loc, scale)
 *   16 weibull_max (c, loc, scale)           17 invgamma (a, loc, scale)
 * PSFMC_EINVAL, with the previous table kept, for an unknown code, parameters scipy rejects (scale <= 0,
 * a shape <= 0, a >= b for truncnorm / reciprocal, randint bounds not integers with low < high) or that
 * are not finite (truncnorm's a, b may be infinite), n_params other than the layout's, or no layout yet.
 */
#define PSFMC_PRIOR_NPAR         4
#define PSFMC_PRIOR_TRUNCNORM    5
#define PSFMC_PRIOR_LOGNORM      6
#define PSFMC_PRIOR_HALFNORM     7
#define PSFMC_PRIOR_EXPON        8
#define PSFMC_PRIOR_LAPLACE      9
#define PSFMC_PRIOR_CAUCHY      10
#define PSFMC_PRIOR_HALFCAUCHY  11
#define PSFMC_PRIOR_LOGISTIC    12
#define PSFMC_PRIOR_T           13
#define PSFMC_PRIOR_BETA        14
#define PSFMC_PRIOR_RECIPROCAL  15
#define PSFMC_PRIOR_WEIBULL_MAX 16
#define PSFMC_PRIOR_INVGAMMA    17
int psfmc_set_priors(psfmc_ctx* ctx, int field, int n_params, const int* family, const double* params);
/*
 * Pixel-integrated Sersic components (not the reference's profile): integrate[k] != 0 makes Sersic component k
 * (model-file order among the Sersics) of observed field `field` (0 in an ordinary context) the PIXEL-INTEGRATED
 * profile -- the plain profile times its full two-dimensional second-order term, midpoint grids in a box of
 * pixels around the centre, recursive refinement of the pixel(s) that hold the centre (definition:
 * psfmc_amd/ModelComponents/Sersic.py Sersic.integrated_image; kernels: csrc/psfmc_integrated.h) -- in every entry
 * point that rasterises: rows and raw vectors, log-likelihoods, images, posterior sums, the device samplers, on both
 * back ends and with either storage.  It is finite where the centre is a pixel centre (the default profile is NaN
 * there).  The fields of one context keep their own flags.  A context that never receives a non-zero flag
 * allocates nothing, launches nothing more and computes what it did without this call; the first non-zero flag
 * allocates max_walkers images of the transform's size.  Call between batches (it waits for the context's stream).
 */
int psfmc_set_sersic_integrate(psfmc_ctx* ctx, int field, int n_sersic, const int* integrate);
/*
 * Ties: parameters of one model that are not independent (Tied(source, ratio, offset); GALFIT's constraints; not the
 * reference's).  Tie t of observed field `field` (0 in an ordinary context) has the value
 *     ratio * theta[src_col[t]] + offset,
 * ratio = theta[ratio_col[t]] or, where ratio_col[t] = -1, ratio_const[t]; offset likewise.  The arithmetic is two
 * separately rounded fp64 operations, product then sum, never a fused multiply-add: numpy's `ratio * source + offset`
 * to the bit.  In every column table the library takes -- psfmc_set_layout[_field]'s slot_col, psfmc_set_aux_layout's
 * aux_col and the col of psfmc_set_fourier / _spiral / _radial / _truncation / _bending_layout -- an entry <= -2
 * names tie t = -2 - entry; -1 stays "the constant" and >= 0 "the column".  A tied entry has no prior of its own
 * (the prior table stays over the n_params free columns); every support rule (reff_b > reff, boxiness <= -2,
 * sum |a_m| >= 1, the spiral, law, truncation and bending rules) reads the resolved value.  The ties are resolved
 * inside the kernels that derive the records and the joint log-priors: no launch is added, and a field without ties
 * runs what it ran.  Call BEFORE the field's psfmc_set_layout[_field]: the ties take effect with that call, which
 * checks them against its n_params, and a registered layout keeps the ties it was checked against until the field's
 * next layout.  n_ties = 0 clears the field's ties (with its next layout).  PSFMC_EINVAL: n_ties outside
 * [0, PSFMC_MAX_TIES], a source column < 0, a ratio / offset column < -1 or a constant that is not finite (here); a
 * tie column >= n_params, a tie on the PSF-index slot (psfmc_set_layout[_field]); a table entry naming tie >= n_ties
 * (the call that passes the table).  In joint fits the columns are the joint vector's.
 */
#define PSFMC_MAX_TIES 64
int psfmc_set_ties(psfmc_ctx* ctx, int field, int n_ties, const int* src_col, const int* ratio_col,
                   const double* ratio_const, const int* offset_col, const double* offset_const);
/*
 * Auxiliary parameters: free parameters beyond the caller row, with the components that read them (not the
 * reference's): a tilted sky (Sky(..., slope=(sx, sy))) and boxy / disky Sersic isophotes (Sersic(..., boxiness=c),
 * GALFIT's C0).  Definitions: psfmc_amd/ModelComponents/Sky.py Sky.tilted_image and Sersic.py Sersic.general_image;
 * kernels: csrc/psfmc_general.h.  Every walker carries an auxiliary vector of n_aux = 2 n_sky + n_sersic doubles:
 * per Sky (model-file order) its slope d/dx, d/dy in ADU per pixel per pixel, then per Sersic its boxiness.
 * aux_col[j] / aux_const[j] have the meaning of psfmc_set_layout's slot_col / slot_const (column of theta, or -1
 * and a constant); a component without the keyword has -1 and 0.  sky_slope_flags [n_sky] and sersic_general_flags
 * [n_sersic] say which components read their entries: a flagged Sky adds sx (x - (nx-1)/2) + sy (y - (ny-1)/2)
 * over the field's own image shape, a flagged Sersic is rendered with rho^2 = (|u|^e + |v|^e)^(2/e), e = c + 2, and
 * Sigma_e / A(c) (total magnitude kept); c <= -2 or not finite gives log-posterior -inf.  A flag on a pixel-
 * integrated component is refused.  Call after the field's psfmc_set_layout[_field] (a new layout drops the
 * field's aux layout) and, in joint fits, before psfmc_set_joint_priors.  n_aux = 0 removes the field's aux layout.
 * The fields of one context keep their own flags and aux layouts.  A context that never receives an aux layout
 * allocates nothing, launches nothing more and computes what it did without this call; the first one allocates
 * max_walkers aux vectors and parameter blocks and (shared with the pixel-integrated profile) max_walkers images of
 * the transform's size.  Every raw-vector entry point (log-posteriors, posterior sums, the device samplers, field
 * sets, joint fits) derives the aux vectors on the device.
 */
int psfmc_set_aux_layout(psfmc_ctx* ctx, int field, int n_aux, const int* aux_col, const double* aux_const,
                         const int* sky_slope_flags, const int* sersic_general_flags);
/*
 * Row-based entry points (psfmc_eval_batch[_field / _device], psfmc_eval_images[_field], psfmc_accumulate_images)
 * take the auxiliary vectors of their W walkers from this companion call: aux [W][n_aux] (host) serves the NEXT
 * row-based call of the context, which must have the same W; on a context with a flagged component such a call
 * without its aux rows is refused (PSFMC_EINVAL), never evaluated without the terms.
 */
int psfmc_set_aux_rows(psfmc_ctx* ctx, int W, const double* aux);
/*
 * Azimuthal Fourier modes on the isophotes of general Sersic components (Sersic(..., fourier={m: (a_m, phi_m)}),
 * GALFIT's F1 ... F6; not the reference's).  Definition: psfmc_amd/ModelComponents/Sersic.py Sersic.fourier_image;
 * kernels: csrc/psfmc_general.h.  mode_mask [n_sersic]: bit m - 1 set where Sersic component k (model-file order)
 * has mode m, m = 1 ... PSFMC_FOURIER_MODES; col / konst [n_sersic][PSFMC_FOURIER_MODES][2] have the meaning of
 * psfmc_set_layout's slot_col / slot_const for the amplitude and the phase of every mode (an absent mode has -1 and
 * 0).  The call APPENDS these 12 n_sersic entries to the field's auxiliary table behind the 2 n_sky + n_sersic
 * entries of psfmc_set_aux_layout, whose indexing does not change; from the first such call on, every walker's
 * auxiliary vector of the context -- psfmc_set_aux_rows' rows included -- has 2 n_sky + 13 n_sersic doubles, the
 * entries of a field without modes unused.  A component with modes is rendered with rho^2 = (|u|^e + |v|^e)^(2/e)
 * (1 + eps)^2, eps = sum_m a_m cos(m (t + phi_m)), t the angle in the component's (u, v) frame, and Sigma_e /
 * (A(c) Q) with Q the 128-point area ratio of the definition (total magnitude kept); phases are in degrees where
 * the layout's sersic_degrees flag of the component is set.  A value that is not finite, or sum_m |a_m| >= 1,
 * gives log-posterior -inf.  Call after the field's psfmc_set_aux_layout, which must flag the components that
 * have modes as general (a new layout or aux layout drops the field's modes) and, in joint fits, before
 * psfmc_set_joint_priors; an all-zero mask removes the field's modes.  Refused: a mode on a pixel-integrated or
 * unflagged component, a mask bit above mode 6, a field without an aux layout.  The fields of one context keep
 * their own masks, registered in any order.  A context that never receives a mode allocates nothing, launches
 * nothing more and computes what it did without this call.
 */
#define PSFMC_FOURIER_MODES 6
int psfmc_set_fourier_layout(psfmc_ctx* ctx, int field, int n_sersic, const int* mode_mask, const int* col,
                             const double* konst);
/*
 * Spiral arms on general Sersic components by coordinate rotation (Sersic(..., spiral={...}); GALFIT-style, not
 * GALFIT's formula and not the reference's).  Definition: psfmc_amd/ModelComponents/Sersic.py Sersic.spiral_image;
 * kernels: csrc/psfmc_general.h.  flags [n_sersic]: nonzero where Sersic component k (model-file order) has a spiral;
 * col / konst [n_sersic][PSFMC_SPIRAL_PARAMS] have the meaning of psfmc_set_layout's slot_col / slot_const, per
 * component in the order r_in, r_out, winding, alpha, inclination, sky_angle, as declared: the three angles are in
 * degrees where the layout's sersic_degrees flag of the component is set.  An unflagged component's entries are never
 * read; give it constants inside the support.  The call APPENDS these 6 n_sersic entries to the field's auxiliary
 * table BEHIND everything it holds: the 2 n_sky + n_sersic entries of psfmc_set_aux_layout and the 12 n_sersic of
 * psfmc_set_fourier_layout, whose indexing and argument checks do not change.  A context with spirals ALWAYS carries
 * the Fourier block: a field without modes gets an empty one (constants 0, nothing more is launched for it), so that
 * from the first such call on every walker's auxiliary vector of the context -- psfmc_set_aux_rows' rows included --
 * has 2 n_sky + 19 n_sersic doubles, the spiral entries of Sersic k at 2 n_sky + 13 n_sersic + 6 k, the entries of a
 * field without a spiral unused; the first call also allocates the per-walker constants spar[w][k][8].  A flagged
 * component is rendered with its pixel offsets deprojected into the disk plane (sky angle, inclination), turned there
 * by t = winding T(r) (r / r_out)^alpha, T = (1 + tanh(2 (2 r - r_in - r_out) / (r_out - r_in))) / 2, and then as a
 * general component (boxiness and modes included) at Sigma_e / cos(inclination) (total magnitude kept).  A value that
 * is not finite, r_in < 0, r_out <= r_in, alpha < 0 or |inclination| >= a right angle gives log-posterior -inf (NaN
 * through a row-based call without writable skip flags).  Call after the field's psfmc_set_aux_layout, which must
 * flag the components that have a spiral as general, after its psfmc_set_fourier_layout where that one is called (a
 * new layout, aux layout or Fourier layout of the field drops its spirals) and, in joint fits, before
 * psfmc_set_joint_priors; all-zero flags remove the field's spirals.  Refused (PSFMC_EINVAL): a flag on a
 * pixel-integrated component or on one that is not flagged general, a field without an aux layout, a wrong n_sersic.
 * The fields of one context keep their own flags, registered in any order.  A context that never receives a spiral
 * allocates nothing, launches nothing more and computes what it did without this call.
 */
#define PSFMC_SPIRAL_PARAMS 6
int psfmc_set_spiral_layout(psfmc_ctx* ctx, int field, int n_sersic, const int* flags, const int* col,
                            const double* konst);
/*
 * Radial laws other than the Sersic law on general components (the Moffat and Ferrer component types of GALFIT; not
 * the reference's).  Definition: psfmc_amd/ModelComponents/Sersic.py Sersic.radial_image; kernels:
 * csrc/psfmc_general.h.  kinds [n_sersic]: per Sersic slot (model-file order) 0 the Sersic law, 1 Moffat, 2 Ferrer;
 * col / konst [n_sersic][PSFMC_RADIAL_PARAMS] have the meaning of psfmc_set_layout's slot_col / slot_const, per slot
 * (beta, unused) of a Moffat or (alpha, beta) of a Ferrer.  A slot of kind 0 has entries that are never read.  A slot
 * with a law has index 1 in the field's layout and the law's two radii -- the full widths at half maximum of a
 * Moffat, the truncation radii of a Ferrer -- in the places of reff and reff_b; mag stays the total magnitude.  It
 * is rendered as a general component (boxiness, modes and spiral included) with
 *     Moffat  Sigma_0 (1 + g rho^2)^-beta, g = 4 (2^(1/beta) - 1), Sigma_0 = F g (beta - 1) / (pi r_a r_b N)
 *     Ferrer  Sigma_0 (1 - rho^(2 - beta))^alpha inside rho = 1 and 0 outside,
 *             Sigma_0 = F / (pi r_a r_b N (2/k) B(2/k, alpha + 1)), k = 2 - beta
 * (N = A(c) Q cos(inclination)) in place of the Sersic law and its centroid term: the value is the law at the pixel
 * centre, Sigma_0 where the centre is a pixel centre.  The call APPENDS these 2 n_sersic entries to the field's
 * auxiliary table BEHIND everything it holds.  A context with laws ALWAYS carries the Fourier block and the spiral
 * block: a field without modes gets an empty Fourier block, a field without a spiral entries inside the spiral's
 * support that are never read (nothing more is launched for either), so that from the first such call on every
 * walker's auxiliary vector of the context -- psfmc_set_aux_rows' rows included -- has 2 n_sky + 21 n_sersic doubles,
 * the laws' entries of Sersic k at 2 n_sky + 19 n_sersic + 2 k, the entries of a field without laws unused.  A
 * Moffat's beta not finite or <= 1, a Ferrer's alpha or beta not finite, alpha < 0 or beta >= 2 gives log-posterior
 * -inf (NaN through a row-based call without writable skip flags).  Call after the field's psfmc_set_aux_layout,
 * which must flag the slots that have a law as general, after its psfmc_set_fourier_layout and
 * psfmc_set_spiral_layout where those are called (a new layout, aux layout, Fourier layout or spiral layout of the
 * field drops its laws) and, in joint fits, before psfmc_set_joint_priors; all-zero kinds remove the field's laws.
 * Refused (PSFMC_EINVAL): a kind outside 0 ... 2, a law on a pixel-integrated slot or on one that is not flagged
 * general, a field without an aux layout, a wrong n_sersic.  The fields of one context keep their own kinds,
 * registered in any order.  A context that never receives a law allocates nothing, launches the kernels it launched
 * and computes what it did without this call.
 */
#define PSFMC_RADIAL_PARAMS 2
int psfmc_set_radial_layout(psfmc_ctx* ctx, int field, int n_sersic, const int* kinds, const int* col,
                            const double* konst);
/*
 * Inner and outer TRUNCATION of general components (GALFIT's truncation function in spirit, not its parametrisation;
 * not the reference's).  Definition: psfmc_amd/ModelComponents/Sersic.py Sersic.truncation_weight and
 * Sersic.truncated_image; kernels: csrc/psfmc_general.h.  flags [n_sersic]: per Sersic slot (model-file order) bit 0
 * an inner, bit 1 an outer truncation; col / konst [n_sersic][PSFMC_TRUNC_PARAMS] have the meaning of
 * psfmc_set_layout's slot_col / slot_const, per slot in_lo, in_hi, out_lo, out_hi in pixels along the slot's major
 * axis; the entries of a side that is absent are never read.  With rho the slot's generalised radius in units of its
 * semi-major radius r_major = 1 / hypot(m00, m01) (boxiness, modes and winding included) and s = r_major rho, the
 * slot's value -- the Sersic law times its centroid term, a Moffat's or Ferrer's law, or with psfmc_set_general_mean
 * every sample of the pixel mean -- is multiplied by
 *     inner = 1 / (1 + exp(-2 a(in_lo, in_hi))),  outer = 1 / (1 + exp(+2 a(out_lo, out_hi))),
 *     a(lo, hi) = 2 (2 s - lo - hi) / (hi - lo)
 * ((1 +- tanh a) / 2 without the cancellation; 0.018 / 0.982 at the two radii of a side; an absent side's factor is left out): the truncation follows the
 * component's own isophotes.  mag stays the total magnitude of the UNTRUNCATED component.  The call APPENDS these
 * 4 n_sersic entries to the field's auxiliary table BEHIND everything it holds.  A context with truncations ALWAYS
 * carries the Fourier, the spiral and the radial block: a field without them gets entries inside their supports that
 * are never read (nothing more is launched for them), so that from the first such call on every walker's auxiliary
 * vector of the context -- psfmc_set_aux_rows' rows included -- has 2 n_sky + 25 n_sersic doubles, the truncation
 * entries of Sersic k at 2 n_sky + 21 n_sersic + 4 k, the entries of a field without truncations unused.  A value of
 * a side present that is not finite, lo < 0 or hi <= lo gives log-posterior -inf (NaN through a row-based call
 * without writable skip flags); there is no condition between the two sides.  Call after the field's
 * psfmc_set_aux_layout, which must flag the truncated slots as general, after its psfmc_set_fourier_layout,
 * psfmc_set_spiral_layout and psfmc_set_radial_layout where those are called (each of them, like a new layout or aux
 * layout, drops the field's truncations) and, in joint fits, before psfmc_set_joint_priors; psfmc_set_general_mean
 * keeps them; all-zero flags remove them, and the slots are rendered as they were, bit for bit.  Refused
 * (PSFMC_EINVAL) with nothing changed: a flag outside 0 ... 3, a truncation on a pixel-integrated slot or on one
 * that is not flagged general, a field without an aux layout, a wrong n_sersic.  The fields of one context keep their
 * own flags, registered in any order.  A context that never receives a nonzero flag allocates nothing, launches the
 * kernels it launched and computes what it did without this call.
 */
#define PSFMC_TRUNC_PARAMS 4
int psfmc_set_truncation_layout(psfmc_ctx* ctx, int field, int n_sersic, const int* flags, const int* col,
                                const double* konst);
/*
 * BENDING MODES of general components (GALFIT's bending modes; not the reference's).  Definition:
 * psfmc_amd/ModelComponents/Sersic.py Sersic.bend and Sersic.bent_image; kernels: csrc/psfmc_general.h.  mode_mask
 * [n_sersic]: per Sersic slot (model-file order) bit m - 1 set where it has bending mode m, m = 1 ... PSFMC_BEND_MODES;
 * col / konst [n_sersic][PSFMC_BEND_MODES] have the meaning of psfmc_set_layout's slot_col / slot_const, per slot the
 * amplitudes a_1 ... a_4 in units of the semi-major radius; the entry of an absent mode is a finite constant (0 by
 * convention) that no pixel reads.  With (u, v) the slot's coordinates in units of its semi-major and semi-minor radius
 * (after the spiral's winding where there is one), r_a = 1 / hypot(m00, m01) and r_b = 1 / hypot(m10, m11),
 *     v' = v + (r_a / r_b) sum_m a_m u^m
 * and everything downstream -- the generalised radius, the angle of the Fourier modes, the centre, the laws and the
 * truncation ramps -- reads (u, v').  In pixels along (x) and across (y) the major axis this is y' = y + sum_m a_m
 * (x / r_a)^m r_a: the ridge lies at Y = -r_a sum_m a_m (X / r_a)^m.  The shear has unit Jacobian and leaves the centre
 * where it is: mag stays the total magnitude, and psfmc_set_general_mean averages the bent law with its scheme
 * unchanged.  The call APPENDS these 4 n_sersic entries to the field's auxiliary table BEHIND everything it holds.  A
 * context with bending modes ALWAYS carries the Fourier, spiral, radial and truncation blocks: a field without them gets
 * entries inside their supports that are never read (nothing more is launched for them), so that from the first such
 * call on every walker's auxiliary vector of the context -- psfmc_set_aux_rows' rows included -- has 2 n_sky +
 * 29 n_sersic doubles, the amplitudes of Sersic k at 2 n_sky + 25 n_sersic + 4 k, the entries of a field without
 * bending modes unused.  An amplitude that is not finite gives log-posterior -inf (NaN through a row-based call without
 * writable skip flags); the shear is a bijection for every finite value, so there is no further condition.  Call after
 * the field's psfmc_set_aux_layout, which must flag the bent slots as general, after its psfmc_set_fourier_layout,
 * psfmc_set_spiral_layout, psfmc_set_radial_layout and psfmc_set_truncation_layout where those are called (each of
 * them, like a new layout or aux layout, drops the field's bending modes) and, in joint fits, before
 * psfmc_set_joint_priors; psfmc_set_general_mean keeps them; all-zero masks remove them, and the slots are rendered as
 * they were, bit for bit.  Refused (PSFMC_EINVAL) with nothing changed: a mask bit above 3, bending on a
 * pixel-integrated slot or on one that is not flagged general, a field without an aux layout, a wrong n_sersic, a
 * column outside the layout.  The fields of one context keep their own masks, registered in any order.  A context that
 * never receives a nonzero mask allocates nothing, launches the kernels it launched and computes what it did without
 * this call.
 */
#define PSFMC_BEND_MODES 4
int psfmc_set_bending_layout(psfmc_ctx* ctx, int field, int n_sersic, const int* mode_mask, const int* col,
                             const double* konst);
/*
 * General components rendered as the MEAN OF THEIR LAW OVER EACH PIXEL (Sersic(..., pixel_mean=True) with a boxiness,
 * modes or a spiral, Moffat(..., pixel_mean=True), Ferrer(..., pixel_mean=True); not the reference's).  Definition:
 * psfmc_amd/ModelComponents/Sersic.py Sersic.general_point and Sersic.general_mean_image; kernels:
 * csrc/psfmc_general_mean.h.  flags [n_sersic]: nonzero where Sersic slot k (model-file order) of the field is
 * rendered so.  A flagged slot's value at a pixel is no longer its law at the pixel centre (times the reference's
 * centroid term for the Sersic law) but (2 g(centre) + the mean of g at the four corners) / 3 with g the law without
 * a centroid term; the mean of g over an 8 x 8 midpoint grid in a pixel that a Ferrer's truncation edge crosses; and
 * in the 7 x 7 pixels around the centre the midpoint grids and the dyadic refinement of the pixel-integrated profile
 * (psfmc_set_sersic_integrate) with g in place of the plain profile: finite where the centre is a pixel centre, mag
 * the total magnitude as before.  The call adds NO entries to the auxiliary table and no parameter: the walkers'
 * auxiliary vectors, psfmc_set_aux_rows' rows and psfmc_debug_aux_table are what they were.  Call after the field's
 * psfmc_set_aux_layout, which must flag the slots as general; psfmc_set_fourier_layout, psfmc_set_spiral_layout and
 * psfmc_set_radial_layout keep the flags (call them before or after), psfmc_set_layout[_field] and
 * psfmc_set_aux_layout drop the field's; all-zero flags remove them, and the slots are rendered as they were, bit for
 * bit.  Refused (PSFMC_EINVAL) with nothing changed: a flag on a slot that is not flagged general or that is
 * pixel-integrated, a field without an aux layout, a wrong n_sersic.  The fields of one context keep their own flags,
 * registered in any order.  A context that never receives a nonzero flag allocates nothing, launches nothing more and
 * passes every kernel the arguments it passed without this call.
 */
int psfmc_set_general_mean(psfmc_ctx* ctx, int field, int n_sersic, const int* flags);
/* host buffers theta [W][n_params], extra_lnprior [W] or NULL, lnprob [W] */
int psfmc_eval_theta(psfmc_ctx* ctx, int W, const double* theta, const double* extra_lnprior,
                     double* lnprob);
/* device buffers, enqueued on `stream` (NULL = the context's stream), not synchronised */
int psfmc_eval_theta_device(psfmc_ctx* ctx, int W, const double* d_theta, const double* d_extra_lnprior,
                            double* d_lnprob, void* stream);

/*
 * Several observed fields in one context (fused back end).  The reference fits one field per process
 * (psfMC/fitting.py:13-113 builds one MultiComponentModel per model file); a survey of many small fields --
 * BASELINE config 5: independent 256 x 256 fields x 256 walkers each -- then makes many small batches, each
 * paying the fixed cost of a call.  Here the fields' walkers share the batches: every walker's record carries
 * (field * n_psf + PSF) as its kernel-spectrum index, the row kernels pick the field's pixels (and, embedded,
 * its image's place in the transform) from it, and 8 x 256 walkers run at the rate of one 2048-walker ensemble.
 * psfmc_ctx_create_fields_shaped: field f is an image of ny[f] x nx[f] pixels (even sides) with n_psf[f] PSFs
 *   of psf_ny[f] x psf_nx[f] (no larger than the image); n_psf[f] is the same for every field.
 *   sci / obs_var / bad_px  the fields' [ny[f]][nx[f]] arrays concatenated in field order;
 *   psf / psf_var           the fields' [n_psf][psf_ny[f]][psf_nx[f]] arrays concatenated in field order.
 *   The fields share ONE transform shape: per axis the fields' common side if it is built, else the cheapest
 *   built side (<= 2048) that every field either has or holds with its wrap-around margin (side + PSF side - 1).
 *   EVERY FIELD PAYS FOR THAT TRANSFORM: a 96 x 96 field in a set with a 256 x 256 one costs what a 256 x 256
 *   walker costs.  Grouping fields of very different sizes into separate sets is the caller's choice.
 *   get_option "transform_ny" / "transform_nx" report the shared transform, psfmc_field_shape a field's own
 *   image sides -- the shape of every pixel array of that field at this ABI (psfmc_eval_images_field,
 *   psfmc_get_accumulated_field).  Arguments are checked (naming the field) before any device is touched.
 * psfmc_ctx_create_fields: the same with every field of one shape: sci / obs_var / bad_px [n_fields][ny][nx],
 *   psf / psf_var [n_fields][n_psf][psf_ny][psf_nx].
 *   the same component counts (n_ps, n_sersic) and parameter layout structure for every field;
 *   psfmc_set_layout (= field 0) first, then psfmc_set_layout_field for fields 1..: own constants, priors
 *   psfmc_eval_theta[_device]_fields: segment i = seg_count[i] consecutive walkers of field seg_field[i];
 *   theta [W][n_params], lnprob [W] in segment order, W = sum of the counts <= max_walkers.
 * Round 3: a context of several fields is also FITTED as one (psfMC/fitting.py:56-113 for every field at once):
 *   psfmc_stretch_run_fields      every field's ensemble (W walkers each, own random numbers) sampled together,
 *                                 the half-step proposals of all fields in one batch of n_fields W / 2 walkers;
 *                                 arrays as psfmc_stretch_run's with the field as the leading dimension
 *   psfmc_accumulate_theta_field  posterior-image sums of ONE field from raw vectors (analysis/images.py:62-74)
 *   psfmc_get_accumulated_field   that field's five posterior images (models.py:74-97) and sample count
 *   psfmc_eval_images_field       the five per-sample images (models.py:222-226) of walkers of one field
 *   psfmc_eval_batch_field        psfmc_eval_batch for derived rows of one field (round 4: models.py:213-216,
 *                                 233-236 on caller-derived scalars; the rows' PSF index counts within the field)
 * psfmc_reset_accumulated clears every field's sums, psfmc_reset_accumulated_field one field's.  The raw-sum exchange for sharded ranks
 * (psfmc_get/set_accumulated_sums) and the half-step API (psfmc_stretch_open ...) serve one-field contexts.
 */
int psfmc_ctx_create_fields_shaped(psfmc_ctx** out, int device, int n_fields, const int* ny, const int* nx,
                                   const double* sci, const double* obs_var, const uint8_t* bad_px, const int* n_psf,
                                   const int* psf_ny, const int* psf_nx, const double* psf, const double* psf_var,
                                   int n_ps, int n_sersic, int max_walkers);
int psfmc_ctx_create_fields(psfmc_ctx** out, int device, int ny, int nx, int n_fields, const double* sci,
                            const double* obs_var, const uint8_t* bad_px, int n_psf, int psf_ny, int psf_nx,
                            const double* psf, const double* psf_var, int n_ps, int n_sersic, int max_walkers);
int psfmc_field_shape(psfmc_ctx* ctx, int field, int* ny, int* nx);
int psfmc_set_layout_field(psfmc_ctx* ctx, int field, int n_sky, int n_params, const int* slot_col,
                           const double* slot_const, const int* ps_method, const int* sersic_degrees,
                           double mag_zeropoint, const int* family, const double* p0, const double* p1,
                           const double* p2);
int psfmc_stretch_run_fields(psfmc_ctx* ctx, int W, int n_iter, double* pos, double* lnprob, int lnprob_valid,
                             const double* z, const double* lz, const int* partner, const double* log_u,
                             double* chain, double* lnprob_chain, long long* naccepted, int accumulate);
int psfmc_accumulate_theta_field(psfmc_ctx* ctx, int field, int W, const double* theta);
int psfmc_reset_accumulated_field(psfmc_ctx* ctx, int field);
int psfmc_get_accumulated_field(psfmc_ctx* ctx, int field, double* raw, double* conv, double* resid, double* ivm,
                                double* ps_sub, long long* count);
int psfmc_eval_images_field(psfmc_ctx* ctx, int field, int W, const double* rows, double* raw, double* conv,
                            double* resid, double* ivm, double* ps_sub);
int psfmc_eval_batch_field(psfmc_ctx* ctx, int field, int W, const double* rows, const uint8_t* skip,
                           double* loglike);
int psfmc_eval_theta_fields(psfmc_ctx* ctx, int n_seg, const int* seg_field, const int* seg_count,
                            const double* theta, const double* extra_lnprior, double* lnprob);
int psfmc_eval_theta_device_fields(psfmc_ctx* ctx, int n_seg, const int* seg_field, const int* seg_count,
                                   const double* d_theta, const double* d_extra_lnprior, double* d_lnprob,
                                   void* stream);
/*
 * Joint fits: several exposures of ONE object (dithers, visits, filters; each field its own data, PSFs,
 * constants and zeropoint) fitted with ONE parameter vector per walker, its log-posterior
 *   lnp(theta) = ((ll_0(theta_0) + ll_1(theta_1)) + ... + ll_{F-1}(theta_{F-1})) + lnprior(theta),
 * theta_f = field f's values read from theta through its own slot -> column map.  A column read by several
 * fields is a shared parameter; a column read by one field only is a per-field one.  -inf when the joint
 * log-prior is not finite, when some field's Sersic component has reff_b > reff, or when the summed
 * log-likelihood is not finite.  A walker's value does not depend on the rest of its batch.
 *   psfmc_set_layout / psfmc_set_layout_field  every field's layout with n_params = the JOINT column count,
 *                                 slot_col into the joint columns; the fields' own prior tables are ignored
 *   psfmc_set_joint_priors        the joint prior table [n_params] (codes and checks of psfmc_set_priors;
 *                                 every column a device family, not PSFMC_PRIOR_HOST), each column counted
 *                                 ONCE.  Valid after every field has its layout; a later layout call
 *                                 invalidates it (call it again).
 *   psfmc_eval_theta_joint[_device]  theta [W][n_params] -> lnprob [W]
 *   psfmc_stretch_run_joint       psfmc_stretch_run's arrays for ONE ensemble of W joint walkers (pos
 *                                 [W][n_params] ...); accumulate: every field's posterior-image sums get the
 *                                 current positions (psfmc_get_accumulated_field)
 * Capacity: each walker is n_fields field records, so n_fields x W <= max_walkers for an evaluation and for
 * the sampler (its start positions and image sums are n_fields x W records).  Beyond it a call returns
 * PSFMC_EINVAL naming max_walkers before any device work is enqueued.  Fused back end only (the contexts of
 * psfmc_ctx_create_fields[_shaped], one field included).
 */
int psfmc_set_joint_priors(psfmc_ctx* ctx, int n_params, const int* family, const double* params);
int psfmc_eval_theta_joint(psfmc_ctx* ctx, int W, const double* theta, double* lnprob);
/* device buffers, enqueued on `stream` (NULL = the context's stream), not synchronised */
int psfmc_eval_theta_joint_device(psfmc_ctx* ctx, int W, const double* d_theta, double* d_lnprob, void* stream);
int psfmc_stretch_run_joint(psfmc_ctx* ctx, int W, int n_iter, double* pos, double* lnprob, int lnprob_valid,
                            const double* z, const double* lz, const int* partner, const double* log_u,
                            double* chain, double* lnprob_chain, long long* naccepted, int accumulate);
/* test hook: the derived rows [W][row_len], log-priors [W] and skip flags [W] the device
 * computes for W vectors */
int psfmc_debug_theta_rows(psfmc_ctx* ctx, int W, const double* theta, double* rows, double* lnprior,
                           uint8_t* skip);

/*
 * Stretch-move ensemble sampling with the walkers resident on the device: n_iter
 * iterations of the two half-ensemble proposals of emcee 2.2.1's EnsembleSampler
 * (the sampler the reference drives, psfMC/fitting.py:56-86; algorithm restated in
 * SURVEY.md Appendix A).  The caller supplies the random numbers in emcee's draw order
 * (per half-step: z, partner index, ln u), so a run reproduces the host-side sampler;
 * nothing is copied to the host between iterations.  Needs psfmc_set_layout (and psfmc_set_priors)
 * with every prior on the device (no PSFMC_PRIOR_HOST column).
 *   pos [W][P], lnprob [W]      in/out (host); lnprob is computed first if !lnprob_valid
 *   lz, log_u [n_iter][2][W/2]  (P-1) ln z and ln u;  z [n_iter][2][W/2]
 *   partner [n_iter][2][W/2]    index into the complementary half-ensemble
 *   chain [W][n_iter][P], lnprob_chain [W][n_iter]   outputs (host, may be NULL)
 *   naccepted [W]               in/out acceptance counters
 *   accumulate                  nonzero: after every iteration add the images of all W
 *                               positions to the posterior sums (psfmc_accumulate_images)
 */
int psfmc_stretch_run(psfmc_ctx* ctx, int W, int n_iter, double* pos, double* lnprob,
                      int lnprob_valid, const double* z, const double* lz, const int* partner,
                      const double* log_u, double* chain, double* lnprob_chain,
                      long long* naccepted, int accumulate);

/*
 * Proposal moves (no reference counterpart; the contract is psfmc_amd/sampler.py's EnsembleSampler(moves=...),
 * which these calls reproduce bit for bit).  psfmc_stretch_run's sampler with the move of every iteration named
 * by the caller: kind[it] is the move of BOTH half-steps of iteration it,
 *   PSFMC_MOVE_STRETCH  q_i = c[a_i] - z_i (c[a_i] - s_i)   scal = z, lz = (P-1) ln z, partner_b unread
 *   PSFMC_MOVE_DE       q_i = s_i + g_i (c[a_i] - c[b_i])   scal = g, lz = 0 (no Hastings term), a_i != b_i
 * (s the active half-ensemble, c the other one; differential evolution, ter Braak 2006, on the split ensemble
 * as emcee 3's DEMove).  Acceptance is psfmc_stretch_run's, (lz + lnp_new) - lnp > ln u.
 *   psfmc_move_run        psfmc_stretch_run's arguments (scal in the place of z; partner is a) plus
 *                           kind [n_iter]             the move codes
 *                           partner_b [n_iter][2][W/2]   the second partner of a DE proposal
 *                         One-field contexts.  Every half-step is four stages: the proposal kernel, the
 *                         record derivation from the proposals, the likelihood pipeline, the accept step; never
 *                         whole-iteration launches ("speculate") or a captured graph.
 *   psfmc_move_run_joint  the same for ONE ensemble of joint walkers (psfmc_stretch_run_joint's rules)
 *   psfmc_stretch_set_moves   between psfmc_stretch_open and the first psfmc_stretch_half_eval: the open run
 *                         proposes by kind (open's z is scal, its partner is a); without it nothing changes
 * PSFMC_EINVAL, with a psfmc_last_error text and before anything is uploaded, for: a kind that is no move code;
 * W < 4 with any DE kind; a partner index outside [0, W/2) (a always, b in DE iterations); a == b in a DE
 * iteration; a PSFMC_PRIOR_HOST column; a context of several fields (psfmc_move_run, psfmc_stretch_set_moves).
 */
#define PSFMC_MOVE_STRETCH 0
#define PSFMC_MOVE_DE 1
int psfmc_move_run(psfmc_ctx* ctx, int W, int n_iter, double* pos, double* lnprob, int lnprob_valid,
                   const double* scal, const double* lz, const int* partner, const double* log_u,
                   const int* kind, const int* partner_b, double* chain, double* lnprob_chain,
                   long long* naccepted, int accumulate);
int psfmc_move_run_joint(psfmc_ctx* ctx, int W, int n_iter, double* pos, double* lnprob, int lnprob_valid,
                         const double* scal, const double* lz, const int* partner, const double* log_u,
                         const int* kind, const int* partner_b, double* chain, double* lnprob_chain,
                         long long* naccepted, int accumulate);
int psfmc_stretch_set_moves(psfmc_ctx* ctx, const int* kind, const int* partner_b);

/*
 * Parallel tempering (no reference counterpart; the contract is psfmc_amd/sampler.py's
 * TemperedEnsembleSampler, which these calls reproduce bit for bit).  One-field contexts with every prior
 * on the device; multi-field and joint contexts and PSFMC_PRIOR_HOST columns return PSFMC_EINVAL (a joint fit
 * goes through psfmc_eval_theta_joint_split / psfmc_pt_run_joint below, the independent fields of a set through
 * psfmc_eval_theta_split_fields / psfmc_pt_run_fields further down).
 * psfmc_eval_theta_split: psfmc_eval_theta's evaluation with the two terms apart -- lnlike [W] (-inf when
 *   the walker is skipped or its log-likelihood is not finite) and lnprior [W] (the device log-prior plus
 *   extra_lnprior), the values psfmc_pt_run works with.
 * psfmc_pt_run: n_iter tempered iterations, nothing copied to the host in between.  T ensembles of W walkers
 *   sample beta_t lnL + lnpi on the ladder betas [T] (1 = beta_0 > ... > beta_{T-1} = 0; T = 1: betas = {1}).
 *   A walker's lnp is beta lnL + lnpi, that product then that sum; lnL = lnp = -inf where lnpi or lnL is not
 *   finite.  Per iteration: the stretch half-steps h = 0, 1 of every rung (one proposal launch, one pipeline
 *   pass over T W/2 records, one accept launch each; random numbers in the host sampler's order, rung-major
 *   within a half-step), then ONE swap launch: for t = T-1 ... 1, walker swap_i[k] of rung t and swap_j[k] of
 *   rung t-1 exchange positions, lnL and lnpi when swap_log_u[k] < (beta_{t-1} - beta_t)(lnL_t - lnL_{t-1}).
 *     pos [T][W][P], lnlike [T][W], lnprior [T][W]   in/out; lnlike / lnprior are evaluated first unless
 *                                 state_valid
 *     z, lz, log_u, partner [n_iter][2][T][W/2]      psfmc_stretch_run's, per rung (partner in [0, W/2))
 *     swap_i, swap_j, swap_log_u [n_iter][T-1][W]    entry t-1 is the rung pair (t-1, t); swap_i and swap_j
 *                                 permutations of [0, W) (checked)
 *     chain [T][W][n_iter][P]     every rung's positions after each iteration's swaps, the beta = 1 rung
 *                                 first: its first W n_iter P entries are the beta = 1 chain (may be NULL)
 *     lnprob_chain [W][n_iter]    lnp of the beta = 1 rung (may be NULL)
 *     lnlike_chain, lnprior_chain [T][W][n_iter]     every rung's lnL and lnpi (may be NULL): with chain, a
 *                                 state to resume from after any iteration
 *     naccepted [T][W], nswap [T-1]                  in/out counters (nswap: accepted swaps per rung pair)
 *     accumulate                  nonzero: after every iteration add the images of the beta = 1 rung's W
 *                                 positions to the posterior sums
 *   PSFMC_EINVAL for T W > max_walkers, an odd W, a bad ladder, a host prior or a context of several fields.
 */
int psfmc_eval_theta_split(psfmc_ctx* ctx, int W, const double* theta, const double* extra_lnprior,
                           double* lnlike, double* lnprior);
int psfmc_pt_run(psfmc_ctx* ctx, int T, int W, int n_iter, const double* betas, double* pos, double* lnlike,
                 double* lnprior, int state_valid, const double* z, const double* lz, const int* partner,
                 const double* log_u, const int* swap_i, const int* swap_j, const double* swap_log_u,
                 double* chain, double* lnprob_chain, double* lnlike_chain, double* lnprior_chain,
                 long long* naccepted, long long* nswap, int accumulate);

/*
 * Parallel tempering of a JOINT fit: contexts of psfmc_ctx_create_fields after psfmc_set_joint_priors.  A
 * walker is one joint vector (P = the joint column count) and F field records.
 * psfmc_eval_theta_joint_split: psfmc_eval_theta_joint with the two terms apart.  lnlike [W] =
 *   ((ll_0 + ll_1) + ...) + ll_{F-1} in psfmc_eval_theta_joint's order, -inf where any field's record is
 *   skipped or the sum is not finite; lnprior [W] the joint log-prior (every joint column once, then every
 *   field's axis-ratio rule).  Where both are finite, lnlike + lnprior is psfmc_eval_theta_joint's value bit
 *   for bit.  F W <= max_walkers, as psfmc_eval_theta_joint.
 * psfmc_pt_run_joint: psfmc_pt_run for T ensembles of W joint walkers -- the same arguments, array shapes,
 *   ladder rules, index checks and swap rule.  Per half-step: one proposal-and-prior launch over T W/2 records,
 *   one record launch over the F fields, one pipeline pass over T W/2 F records (record r of field f at
 *   r + f T W/2), one accept launch that sums each proposal's fields; then psfmc_pt_run's swap launch.  The
 *   start state is one batch of T W walkers.  accumulate: every field's posterior sums get the beta = 1 rung's
 *   W positions after every iteration.
 *   PSFMC_EINVAL, before anything is uploaded, for T W F > max_walkers, an odd W, a bad ladder, an index out
 *   of range, swap indices that are no permutations, or a context without joint priors.
 */
int psfmc_eval_theta_joint_split(psfmc_ctx* ctx, int W, const double* theta, double* lnlike, double* lnprior);
int psfmc_pt_run_joint(psfmc_ctx* ctx, int T, int W, int n_iter, const double* betas, double* pos, double* lnlike,
                       double* lnprior, int state_valid, const double* z, const double* lz, const int* partner,
                       const double* log_u, const int* swap_i, const int* swap_j, const double* swap_log_u,
                       double* chain, double* lnprob_chain, double* lnlike_chain, double* lnprior_chain,
                       long long* naccepted, long long* nswap, int accumulate);

/*
 * Parallel tempering of EVERY field of a set together: contexts of psfmc_ctx_create_fields[_shaped] with
 * per-field layouts and device priors (no joint priors).  Field f's ladder is its own psfmc_pt_run: given the
 * same start, ladder and random numbers, every output equals the one of field f's own one-field context bit for
 * bit (a walker's value does not depend on its batch).
 * psfmc_eval_theta_split_fields: psfmc_eval_theta_fields (its segments, order and capacity) with the two terms
 *   apart by psfmc_eval_theta_split's rules -- lnlike [W] -inf where the walker is skipped or its log-likelihood
 *   is not finite, lnprior [W] the device log-prior plus extra_lnprior.  Where both are finite, lnlike + lnprior
 *   is psfmc_eval_theta_fields' value bit for bit.
 * psfmc_pt_run_fields: psfmc_pt_run for the F = n_fields independent ladders, one ladder betas [T] for all.
 *   Ensemble e = f T + t is rung t of field f; every array of psfmc_pt_run carries the field in front of the
 *   rung, the random numbers behind the iteration (and half-step):
 *     pos [F][T][W][P]; lnlike, lnprior, naccepted [F][T][W]; nswap [F][T-1]
 *     z, lz, log_u, partner [n_iter][2][F][T][W/2]
 *     swap_i, swap_j, swap_log_u [n_iter][F][T-1][W]
 *     chain [F][T][W][n_iter][P]; lnprob_chain [F][W][n_iter] (each field's beta = 1 rung);
 *     lnlike_chain, lnprior_chain [F][T][W][n_iter]
 *   Launches per iteration do not depend on F or T.  Per half-step: one proposal launch over the F T W/2
 *   records, one record launch over the F fields, one pipeline pass over F T W/2 records, one accept launch;
 *   then ONE swap launch, workgroup f doing field f's ladder.  The start state is one batch of F T W records.
 *   accumulate: after every iteration field f's posterior sums get the W positions of its beta = 1 rung.
 *   PSFMC_EINVAL, with a psfmc_last_error text and before anything is uploaded, for F T W > max_walkers (the
 *   text names max_walkers and the field count), an odd W, a bad ladder, a partner outside [0, W/2), swap
 *   indices out of range or no permutations (per iteration, field and rung pair), a field without a layout, a
 *   PSFMC_PRIOR_HOST column, or a context with joint priors set.
 */
int psfmc_eval_theta_split_fields(psfmc_ctx* ctx, int n_seg, const int* seg_field, const int* seg_count,
                                  const double* theta, const double* extra_lnprior, double* lnlike,
                                  double* lnprior);
int psfmc_pt_run_fields(psfmc_ctx* ctx, int T, int W, int n_iter, const double* betas, double* pos, double* lnlike,
                        double* lnprior, int state_valid, const double* z, const double* lz, const int* partner,
                        const double* log_u, const int* swap_i, const int* swap_j, const double* swap_log_u,
                        double* chain, double* lnprob_chain, double* lnlike_chain, double* lnprior_chain,
                        long long* naccepted, long long* nswap, int accumulate);

/*
 * Proposal moves on tempered ladders (the contract is TemperedEnsembleSampler.set_moves): psfmc_pt_run,
 * psfmc_pt_run_joint and psfmc_pt_run_fields with the move of every iteration named, as psfmc_move_run names
 * it for one ensemble.  The arguments are the twin's plus, behind log_u,
 *     kind        [n_iter] (psfmc_pt_move_run_fields: [n_iter][F], each field's ladder its own move)
 *                 PSFMC_MOVE_STRETCH or PSFMC_MOVE_DE: the move of BOTH half-steps of EVERY rung of the ladder
 *     partner_b   shaped as partner: the DE moves' second partner, from the same rung's other half; not read
 *                 in a stretch iteration
 * and z carries the move's scalar (z, or the DE g), lz its Hastings term ((P - 1) ln z, or 0), partner the
 * first partner.  Per half-step: ONE proposal launch by kind over all rungs' (and ladders') records
 * (k_pt_move_propose; a DE element is three roundings: the difference, the product, the sum), the records of
 * the given vectors (a joint fit: the joint prior launch and the F fields' record launch), the pipeline pass and
 * the twin's accept launch; swaps, chains, counters and accumulate are the twin's.  One launch more per
 * half-step than psfmc_pt_run and psfmc_pt_run_joint, none more than psfmc_pt_run_fields.  With T = 1 and betas
 * = {1}, psfmc_pt_move_run_fields is the moves run of a field set's plain ensembles.
 * PSFMC_EINVAL, with a psfmc_last_error text and before anything is uploaded, for everything the twin refuses
 * and for: a NULL kind or partner_b, a kind that is no move code, W < 4 in a DE iteration, and in a DE
 * iteration a partner_b outside [0, W/2) or equal to partner.
 */
int psfmc_pt_move_run(psfmc_ctx* ctx, int T, int W, int n_iter, const double* betas, double* pos, double* lnlike,
                      double* lnprior, int state_valid, const double* z, const double* lz, const int* partner,
                      const double* log_u, const int* kind, const int* partner_b, const int* swap_i,
                      const int* swap_j, const double* swap_log_u, double* chain, double* lnprob_chain,
                      double* lnlike_chain, double* lnprior_chain, long long* naccepted, long long* nswap,
                      int accumulate);
int psfmc_pt_move_run_joint(psfmc_ctx* ctx, int T, int W, int n_iter, const double* betas, double* pos,
                            double* lnlike, double* lnprior, int state_valid, const double* z, const double* lz,
                            const int* partner, const double* log_u, const int* kind, const int* partner_b,
                            const int* swap_i, const int* swap_j, const double* swap_log_u, double* chain,
                            double* lnprob_chain, double* lnlike_chain, double* lnprior_chain,
                            long long* naccepted, long long* nswap, int accumulate);
int psfmc_pt_move_run_fields(psfmc_ctx* ctx, int T, int W, int n_iter, const double* betas, double* pos,
                             double* lnlike, double* lnprior, int state_valid, const double* z, const double* lz,
                             const int* partner, const double* log_u, const int* kind, const int* partner_b,
                             const int* swap_i, const int* swap_j, const double* swap_log_u, double* chain,
                             double* lnprob_chain, double* lnlike_chain, double* lnprior_chain,
                             long long* naccepted, long long* nswap, int accumulate);

/*
 * The same sampler one half-step at a time, for walkers sharded over several GPUs (one
 * process per GPU).  Every rank opens the SAME ensemble with the SAME
 * random numbers; per half-step each rank calls psfmc_stretch_half_eval for its contiguous
 * block [lo, lo + n) of the half-ensemble's proposals (the proposals, priors and prep records
 * of the whole half are formed on every rank; only the block's likelihood pipeline runs), the
 * caller all-gathers the blocks' log-posteriors (torch.distributed / RCCL: the one collective
 * of the path) and hands the gathered half-ensemble vector to psfmc_stretch_half_accept, which
 * applies the identical accept / move / chain entry on every rank.  There is no reference
 * counterpart (psfMC/fitting.py:55 gave up on parallel evaluation); the result equals
 * psfmc_stretch_run's chain bit for bit.  d_* are device pointers, `stream` a hipStream_t
 * (NULL = the context's stream); nothing is synchronised except in open / close.
 *   psfmc_stretch_accumulate   add the images of walkers [lo, lo + n) of the current
 *                              ensemble to this rank's posterior sums
 *   psfmc_get/set_accumulated_sums   the raw sums [4][ny][nx] (raw, convolved, model
 *                              variance, PS-only convolved) + sample count, so that ranks'
 *                              shares can be added up (all-reduce) before
 *                              psfmc_get_accumulated turns them into means
 */
int psfmc_stretch_open(psfmc_ctx* ctx, int W, int n_iter, const double* pos, const double* lnprob,
                       const double* z, const double* lz, const int* partner, const double* log_u,
                       const long long* naccepted, int store_chain);
int psfmc_stretch_half_eval(psfmc_ctx* ctx, int it, int h, int lo, int n, double* d_newlnp_block,
                            void* stream);
int psfmc_stretch_half_accept(psfmc_ctx* ctx, int it, int h, const double* d_newlnp_half, void* stream);
int psfmc_stretch_accumulate(psfmc_ctx* ctx, int lo, int n, void* stream);
int psfmc_stretch_close(psfmc_ctx* ctx, double* pos, double* lnprob, double* chain,
                        double* lnprob_chain, long long* naccepted, void* stream);
int psfmc_get_accumulated_sums(psfmc_ctx* ctx, double* sums, long long* count);
int psfmc_set_accumulated_sums(psfmc_ctx* ctx, const double* sums, long long count);

/*
 * One process driving several GPUs (the form SURVEY.md section 8(b) sketched; the
 * one-process-per-GPU form with torch.distributed / RCCL is psfmc_amd/parallel.py).  The
 * field is replicated on every listed device (a device may be listed more than once),
 * walkers are split into contiguous blocks (block r = walkers [r W/n ...)), every device's
 * upload, evaluation and download are enqueued before any is waited for, and each block
 * lands at its offset of the caller's host array.  max_walkers bounds W of the whole
 * group.  Results equal the single-context ones bit for bit.  No reference counterpart
 * (psfMC/fitting.py:55).
 */
typedef struct psfmc_group psfmc_group;
int psfmc_group_create(psfmc_group** out, int n_dev, const int* devices, int ny, int nx,
                       const double* sci, const double* obs_var, const uint8_t* bad_px,
                       int n_psf, int psf_ny, int psf_nx, const double* psf, const double* psf_var,
                       int n_ps, int n_sersic, int max_walkers, int backend);
int psfmc_group_destroy(psfmc_group* group);
int psfmc_group_size(const psfmc_group* group);
int psfmc_group_set_layout(psfmc_group* group, int n_sky, int n_params, const int* slot_col,
                           const double* slot_const, const int* ps_method, const int* sersic_degrees,
                           double mag_zeropoint, const int* family, const double* p0, const double* p1,
                           const double* p2);
/* psfmc_set_priors on every device of the group */
int psfmc_group_set_priors(psfmc_group* group, int n_params, const int* family, const double* params);
/* psfmc_set_ties (field 0) on every device of the group; before psfmc_group_set_layout */
int psfmc_group_set_ties(psfmc_group* group, int n_ties, const int* src_col, const int* ratio_col,
                         const double* ratio_const, const int* offset_col, const double* offset_const);
/* psfmc_set_aux_layout (field 0) on every device of the group (raw-vector entry points; the group's row-based
 * psfmc_group_eval_batch has no aux rows and is refused on such a group) */
int psfmc_group_set_aux_layout(psfmc_group* group, int n_aux, const int* aux_col, const double* aux_const,
                               const int* sky_slope_flags, const int* sersic_general_flags);
/* psfmc_set_fourier_layout (field 0) on every device of the group */
int psfmc_group_set_fourier_layout(psfmc_group* group, int n_sersic, const int* mode_mask, const int* col,
                                   const double* konst);
/* psfmc_set_spiral_layout (field 0) on every device of the group */
int psfmc_group_set_spiral_layout(psfmc_group* group, int n_sersic, const int* flags, const int* col,
                                  const double* konst);
/* psfmc_set_truncation_layout (field 0) on every device of the group */
int psfmc_group_set_truncation_layout(psfmc_group* group, int n_sersic, const int* flags, const int* col,
                                      const double* konst);
/* psfmc_set_bending_layout (field 0) on every device of the group */
int psfmc_group_set_bending_layout(psfmc_group* group, int n_sersic, const int* mode_mask, const int* col,
                                   const double* konst);
/* psfmc_set_radial_layout (field 0) on every device of the group */
int psfmc_group_set_radial_layout(psfmc_group* group, int n_sersic, const int* kinds, const int* col,
                                  const double* konst);
/* psfmc_set_general_mean (field 0) on every device of the group */
int psfmc_group_set_general_mean(psfmc_group* group, int n_sersic, const int* flags);
/* psfmc_set_sersic_integrate (field 0) on every device of the group */
int psfmc_group_set_sersic_integrate(psfmc_group* group, int n_sersic, const int* integrate);
int psfmc_group_eval_batch(psfmc_group* group, int W, const double* rows, const uint8_t* skip,
                           double* loglike);
int psfmc_group_eval_theta(psfmc_group* group, int W, const double* theta, const double* extra_lnprior,
                           double* lnprob);

/*
 * Posterior-image accumulation on the device (replaces the per-sample blob
 * hand-over and the running mean of MultiComponentModel.accumulate_images,
 * models.py:74-97, fed from fitting.py:83).  psfmc_accumulate_images adds the images
 * of W walkers (rows as above) to device-resident sums; composite_ivm is averaged as
 * a variance (models.py:81-97).  psfmc_get_accumulated returns the means ([ny][nx]
 * each, any pointer may be NULL; ivm = 1 / mean variance) and the sample count.
 */
int psfmc_accumulate_images(psfmc_ctx* ctx, int W, const double* rows);
/* the same for W raw parameter vectors [W][n_params] (psfmc_set_layout): records derived on the device */
int psfmc_accumulate_theta(psfmc_ctx* ctx, int W, const double* theta);
int psfmc_get_accumulated(psfmc_ctx* ctx, double* raw, double* conv, double* resid, double* ivm,
                          double* ps_sub, long long* count);
int psfmc_reset_accumulated(psfmc_ctx* ctx);

/*
 * Device-computed PSF spectra, for checking the on-device replacement of
 * pre_fft_psf (utils.py:126-133): out arrays [n_psf][ny][nx/2+1][2] (re, im),
 * equal to numpy.fft.rfft2 of the centre-padded images.
 */
int psfmc_get_spectra(psfmc_ctx* ctx, double* psf_spec, double* var_spec);

/* tuning knobs: "chunk_walkers" (walkers per internal pass), "streams" (passes in
 * flight, 1..4), "cols_grid", "stagger" (0 / 1: the second pass in flight starts one
 * forward-row kernel after the first; default per image shape, results do not depend on it),
 * "linear_accumulation" (0 / 1, default 1, fused back end): posterior-image samples are added up as
 * raw / raw^2 / point-source-only raw and convolved once when the images are read, instead of every
 * sample going through the transforms (the five images are linear in those three),
 * "profile" (1: time every kernel with HIP events; read
 * back with get_option "prof_ms_rows_fwd" / "prof_n_rows_fwd", ..._cols, ..._rows_inv).
 * "storage_f32" (0 / 1, default 0): keep the fused path's intermediate half-spectra as
 * complex64 while every operation stays fp64 -- half the memory traffic; the log-posterior is
 * then good to ~1e-7 relative, the class of the reference's own float32 raw-model accumulator
 * (psfMC/models.py:249), not an fp64 result.  Power-of-two sides, fused back end only.
 * "cols3" (0 ... 4, default 1): which column kernel runs -- 0 the two-stage engine wherever a side has one, 1 the
 * wave-wide three-stage engines where they measured faster (round 4: k_cols3f at 512 / 1024 / 1536 / 2048, k_cols3g
 * at the other sides of psfmc_fft.h fft3g_pick), 2 k_cols3g at those four as well, 3 round 3's k_cols3 at 512 and
 * 1024 (elsewhere as 2), 4 the same as 1; results agree to rounding.  Sides above 1024 have only the three-stage
 * kernels: there 0 is refused, as is any value other than 0 ... 4, and the context keeps the engine it had.
 * "exclusive" (bits 0 / 1 / 2 = forward rows / columns / inverse rows, default 0): chain the two passes in flight so
 * that two kernels of that kind never run side by side (measurement knob; slower in every combination).
 * "speculate" (device sampler, psfmc_stretch_run): ensembles of up to 2 n walkers run ONE pipeline pass per
 * iteration -- the first half's proposals and both candidate proposals of every second-half walker (partner
 * moved / partner stayed) -- instead of two half-steps; the chain is the same bit for bit.  0 never, n > 0 that
 * bound, -1 (default) n = 3e6 / transform pixels, the measured break-even; needs max_walkers >= 1.5 W.
 * get_option only: "pow_tabs" (1: this context's rasterising kernels take (rho^2)^p from per-walker power tables --
 * transforms of more than 256 pixels per row --, 0: log2 + exp2 per pixel; a property of the transform shape),
 * "pow_tabs_built" (1: the last batch's forward rows read the tables k_pow_tables built in memory, 0: its row waves
 * formed the entries themselves -- small batches, psfmc_hip.hip launch_pow_tables -- or the context has no tables),
 * "raster_group" (the pixels per lane the forward row kernel's power-table rasteriser takes through the profile
 * together: 1, 2 or 4 by row length and embedding; 0 where it is the log2 + exp2 form; NaN on the hipFFT back end),
 * "transform_ny" / "transform_nx" (the transform shape: the image's own, or the built sides an
 * image of unbuilt sides is embedded in), "speculated_runs", "graph_launches", "row_group",
 * "partials_per_walker", "cols3", "column_engine" (the column kernel this context launches now: 0 k_cols, 1 k_cols3, 2
 * k_cols3g, 3 k_cols3f), "rows3" (bit 0 / bit 1: the forward / inverse row kernel is the one-row-per-wave
 * three-stage one of csrc/psfmc_rows3_path.h -- both above 1024, the inverse one at seven general sides; the
 * environment variable PSFMC_ROWS3 = 1 / 0, read at context creation, forces every built one / none: A/B runs),
 * "aux_stride" (doubles per walker of the context's auxiliary vectors, psfmc_set_aux_rows' rows included: 0 before
 * the first aux layout, then 2 n_sky + n_sersic, + 12 / 18 / 20 n_sersic from the first modes / spiral / law of any
 * field on; it never shrinks).
 */
int psfmc_set_option(psfmc_ctx* ctx, const char* key, double value);
double psfmc_get_option(const psfmc_ctx* ctx, const char* key);

/*
 * Diagnostic hook: evaluate one of the library's fp64 device functions on n host
 * values (op 0 log2, 1 exp2, 2 reciprocal, 3 single-Newton reciprocal, 4 exp2 without
 * clamp, 5 the rasteriser's table-driven log2, 6 exp2 with the lower clamp only; op 100: x^p through the
 * rasteriser's per-walker power tables, with p passed as in[n], i.e. `in` holds n + 1 values) so tests can
 * check the hand-written elementary functions of the rasteriser against numpy.
 */
int psfmc_debug_math(int device, int op, int n, const double* in, double* out);
/*
 * Diagnostic hook: the auxiliary table the library composes for ONE field from what the field registered, on the
 * host alone (no context, no device).  base_col / base_const [2 n_sky + n_sersic]: psfmc_set_aux_layout's arrays
 * (NULL: no aux layout); per block the tags [n_sersic] -- mode masks, spiral flags, radial kinds -- and col / konst
 * of psfmc_set_fourier_layout, psfmc_set_spiral_layout and psfmc_set_radial_layout (NULL tags: never registered).
 * out_const / out_col [2 n_sky + 21 n_sersic] receive the table's first counts[0] entries in the order the device
 * reads them, out_kinds [n_sersic] the kinds behind the columns (written where counts[3] > 0); counts [4] =
 * n_aux, n_fou, n_spi, n_rad of the field's layout.
 */
int psfmc_debug_aux_table(int n_sky, int n_sersic, const int* base_col, const double* base_const,
                          const int* mode_mask, const int* fou_col, const double* fou_const,
                          const int* spi_flags, const int* spi_col, const double* spi_const,
                          const int* rad_kinds, const int* rad_col, const double* rad_const,
                          double* out_const, int* out_col, int* out_kinds, int* counts);
/*
 * ... and with the truncation block (psfmc_set_truncation_layout's flags, col and konst; NULL flags: never
 * registered, and the call is psfmc_debug_aux_table).  out_const / out_col [2 n_sky + 25 n_sersic]; where tru_flags
 * is given, out_sides [n_sersic] receives the sides behind the kinds (written where counts[4] > 0; the kinds are
 * then zeros for a field without laws) and counts has five entries: n_aux, n_fou, n_spi, n_rad, n_tru.
 */
int psfmc_debug_aux_table_blocks(int n_sky, int n_sersic, const int* base_col, const double* base_const,
                                 const int* mode_mask, const int* fou_col, const double* fou_const,
                                 const int* spi_flags, const int* spi_col, const double* spi_const,
                                 const int* rad_kinds, const int* rad_col, const double* rad_const,
                                 const int* tru_flags, const int* tru_col, const double* tru_const,
                                 double* out_const, int* out_col, int* out_kinds, int* out_sides, int* counts);
/*
 * ... and with the bending block (psfmc_set_bending_layout's mode_mask, col and konst; NULL bnd_mask: never registered,
 * and the call is psfmc_debug_aux_table_blocks).  out_const / out_col [2 n_sky + 29 n_sersic]; where bnd_mask is given,
 * out_sides [n_sersic] is written where counts[4] > 0 (zeros for a field without truncations), out_bends [n_sersic]
 * receives the bending masks (written where counts[5] > 0) and counts has six entries: n_aux, n_fou, n_spi, n_rad,
 * n_tru, n_bnd.
 */
int psfmc_debug_aux_table_bending(int n_sky, int n_sersic, const int* base_col, const double* base_const,
                                  const int* mode_mask, const int* fou_col, const double* fou_const,
                                  const int* spi_flags, const int* spi_col, const double* spi_const,
                                  const int* rad_kinds, const int* rad_col, const double* rad_const,
                                  const int* tru_flags, const int* tru_col, const double* tru_const,
                                  const int* bnd_mask, const int* bnd_col, const double* bnd_const,
                                  double* out_const, int* out_col, int* out_kinds, int* out_sides, int* out_bends,
                                  int* counts);

/*
 * Fisher matrix and gradient of the Gaussian log-likelihood
 *   lnL = -1/2 sum_good [ r^2 w - ln(w / 2 pi) ],  r = sci - conv,  w = 1 / (model_var + obs_var)
 * at n_base points, from central-difference stencils of images (the definition: psfmc_amd/mode.py
 * fisher_from_stencil).  A stencil of K differentiated columns is 2K + 1 walkers: the base
 * vector, then theta + h_k e_k and theta - h_k e_k for k = 0 ... K-1.
 *   rows    [n_base][2K+1][row_len]  derived rows exactly as psfmc_eval_images[_field] takes them (a context with an
 *                                    aux layout: psfmc_set_aux_rows for the n_base (2K+1) walkers first)
 *   inv2h   [n_base][K]              1 / (2 h_k)
 *   F       [n_base][K][K]           out: sum_good w dmu_k dmu_l + 1/2 sum_good w^2 dv_k dv_l  (exactly symmetric)
 *   g       [n_base][K]              out: d lnL / d theta_k = sum_good r w dmu_k + 1/2 sum_good (r^2 w^2 - w) dv_k
 *   lnlike  [n_base]                 out: the base's log-likelihood, the bits psfmc_eval_batch gives for its row
 * 1 <= K <= 63 and n_base (2K+1) <= max_walkers.  The walkers run in passes of psfmc_get_option "chunk_walkers" like
 * psfmc_eval_images'; a stencil may straddle passes, and its F, g and lnlike do not depend on where in the batch it
 * stands or on what stands beside it.  "good": not in bad_px and a finite base weight; an image that is not finite
 * on a good pixel (or a negative weight) gives NaN results for that stencil, not an error.  Both back ends.
 * PSFMC_EINVAL with "storage_f32" on: images good to 1e-7 divided by a 1e-4 step are noise.  A context that never
 * calls this allocates and launches nothing for it.
 */
int psfmc_fisher_rows(psfmc_ctx* ctx, int field, int n_base, int K, const double* rows, const double* inv2h,
                      double* F, double* g, double* lnlike);
/*
 * psfmc_fisher_rows for stencils of DIFFERENT fields of a psfmc_ctx_create_fields context in one call (DESIGN.md
 * section 31): stencil s is 2K + 1 walkers of field field[s]; every stencil of a call has the same K.
 *   field   [n_stencils]                 the stencils' fields, in any order, a field as often as wanted
 *   rows    [n_stencils][2K+1][row_len]  as psfmc_fisher_rows takes them (the PSF index counts within the field; a
 *                                        context with an aux layout: psfmc_set_aux_rows for all n_stencils (2K+1)
 *                                        walkers first)
 *   inv2h   [n_stencils][K]
 *   F [n_stencils][K][K], g [n_stencils][K], lnlike [n_stencils]   out
 * Stencil s's F, g and lnlike are the bits psfmc_fisher_rows(ctx, field[s], 1, K, ...) gives for that stencil alone,
 * whatever stands beside it, in whatever field order, and wherever a pass boundary falls.  The records are derived
 * per run of equal field; the image passes run over the mixed records (a record's field is its kernel-spectrum
 * index / PSFs per field, as in the log-posterior pipeline); then ONE Gram and ONE finish launch serve every stencil
 * through a per-stencil device table.  1 <= K <= 63 and n_stencils (2K+1) <= max_walkers.  Fused back end and fp64
 * storage only (PSFMC_EINVAL otherwise), as every shared context is.  Nothing is allocated or launched for it
 * until the first call.
 */
int psfmc_fisher_rows_fields(psfmc_ctx* ctx, int n_stencils, int K, const int* field, const double* rows,
                             const double* inv2h, double* F, double* g, double* lnlike);
/*
 * Fisher matrix and gradient of a JOINT fit (psfmc_eval_theta_joint's likelihood: the fields' sum) at n_base points.
 * Field f of the context reads K_field of the K_joint differentiated joint columns: its column k is joint column
 * col_of[f][k].  Stencil (b, f) holds field f's base row of point b and the +- rows of those K_field columns only.
 *   col_of  [n_fields][K_field]                        injective per field, values in [0, K_joint)
 *   rows    [n_base][n_fields][2 K_field + 1][row_len]
 *   inv2h   [n_base][n_fields][K_field]                (the fields that share a joint column share its step)
 *   F       [n_base][K_joint][K_joint]   out: element (r, c) starts at +0.0 and adds, for f = 0 ... n_fields - 1 in
 *                                        that order, F_f[kr][kc] with col_of[f][kr] = r, col_of[f][kc] = c; a field
 *                                        that does not read both is skipped.  Exactly symmetric.
 *   g       [n_base][K_joint]            out: the same sum of g_f[kr]
 *   lnlike  [n_base]                     out: ((ll_0 + ll_1) + ...) + ll_{F-1}, the sum psfmc_eval_theta_joint_split
 *                                        defines, of the ROW-based ll_f (unguarded: not -inf'ed where it is not
 *                                        finite).  The split entry forms its records from raw vectors on the device,
 *                                        these rows come from the caller: the two values agree to rounding (2e-13
 *                                        relative measured), not in their bits.
 * F_f, g_f and ll_f are the bits psfmc_fisher_rows gives for field f's stencil alone.  A joint column no field reads
 * is a zero row and column.  1 <= K_field <= 63; K_joint is limited by memory only (one thread per element of the
 * result, no atomics); n_base n_fields (2 K_field + 1) <= max_walkers.  A col_of that is not injective or leaves
 * [0, K_joint) is PSFMC_EINVAL.  Contexts with or without joint priors (the images do not read them).  Back end,
 * storage and aux rows as psfmc_fisher_rows_fields.
 */
int psfmc_fisher_rows_joint(psfmc_ctx* ctx, int n_base, int K_joint, int K_field, const int* col_of,
                            const double* rows, const double* inv2h, double* F, double* g, double* lnlike);
/*
 * Diagnostic hook: the Gram and finish kernels of psfmc_fisher_rows alone, on caller-supplied per-pixel vectors
 * a, b [K][n_pix] and c, d [n_pix]:  F = sum_pix (a a^T + b b^T) [K][K],  g_k = sum_pix (a_k c + b_k d) [K].
 * Small-integer data make every product and sum exact in fp64, so a wrong lane map shows as a wrong integer.
 */
int psfmc_debug_fisher_gram(int device, int K, int n_pix, const double* a, const double* b, const double* c,
                            const double* d, double* F, double* g);

/*
 * Diagnostic hook: time `reps` plain sweeps over a scratch buffer of nbytes (>= 1 MiB) -- mode 0
 * every byte written once, 1 read and written back in place, 2 read once: the memory traffic of
 * the three kernels of a pass without their arithmetic.  *us_per_sweep = average microseconds.
 * bench.py reports them beside the timed step ("sweep_ceiling").
 */
int psfmc_debug_sweep(int device, int mode, size_t nbytes, int reps, double* us_per_sweep);
/* measurement hook: nanoseconds per fp64 vector wave-instruction per SIMD with `waves_per_simd` waves on every
 * SIMD of the chip (64 v_fma_f64 per loop iteration): the VALU ceiling next to psfmc_debug_sweep's memory one */
int psfmc_debug_valu_rate(int device, int waves_per_simd, int iters, double* ns_per_instruction);

/* message of the last failing call on this thread ("" if none) */
const char* psfmc_last_error(void);

/* library/ABI version (bumped when a signature changes) */
int psfmc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PSFMC_HIP_H */
