// psfmc_general.h -- components with FREE PARAMETERS BEYOND THE ROW: boxy / disky Sersic isophotes
// (`Sersic(..., boxiness=c)`, GALFIT's C0) and a tilted sky (`Sky(..., slope=(sx, sy))`).  Not the reference's.
//
// Definitions: psfmc_amd/ModelComponents/Sersic.py `Sersic.general_image` and Sky.py `Sky.tilted_image` (numpy);
// these kernels are held to them.  The new parameters reach the device as a per-walker AUXILIARY VECTOR
// aux[w][n_aux] = per Sky (sx, sy), then per Sersic its boxiness (k_theta_prep writes it from the walker's parameter
// tile, psfmc_set_aux_rows from the host for row-based calls); caller rows and prep records keep their layouts.
// Per walker the kernels write (or, behind the pixel-integrated profile's kernels, add to) the walker's EXTRA IMAGE
// (psfmc_integrated.h: [ny][nx] doubles at model coordinates, added by the EXTRA instantiations of the rasterising
// kernels).  A general Sersic component's block of the prep record is replaced by the neutral block, as an
// integrated one's is, and its real block moves to gpar[w][k][kGenPar].
//
//   k_general_split   per (walker, component): move a flagged block to gpar with e = c + 2, 2 / e and Sigma_e / A(c),
//                     A(c) = 4 Gamma(1 + 1/e)^2 / (pi Gamma(1 + 2/e)) (lgamma once per walker and component);
//                     leave the neutral block; c <= -2 or not finite: the walker is skipped (log-posterior -inf)
//   k_general_rows    a wave per image row over the field's own ly x lx pixels: the slope terms of the flagged skies
//                     (the constant level stays in the record's head) plus every general component
//   k_fourier_prep    (contexts with azimuthal Fourier modes only, between the two) a wave per (walker, component
//                     with modes): a_m cos(m phi_m), a_m sin(m phi_m) per mode and the area ratio Q of the
//                     perturbed isophote, Sigma_e / A(c) becomes Sigma_e / (A(c) Q); outside the support (a value
//                     not finite, sum |a_m| >= 1) the walker is skipped
// The work per walker is fixed, each pixel is one lane's own sum in component order, there are no atomics: a
// walker's bits do not depend on its batch.
//
// AZIMUTHAL FOURIER MODES (`Sersic(..., fourier={m: (a_m, phi_m)})`, GALFIT's F1 ... F6; definition: Sersic.py
// `Sersic.fourier_image`): rho^2 = (|u|^e + |v|^e)^(2/e) (1 + eps)^2, eps = sum_m a_m cos(m (t + phi_m)), t the angle
// of (u, v).  psfmc_set_fourier_layout appends 2 kFouModes entries per Sersic -- per mode 1 ... 6 its amplitude and
// its phase as declared (degrees where the layout's sersic_degrees flag is set) -- to the walkers' auxiliary vectors
// BEHIND the aux_len entries; a per (field, Sersic) byte holds the mode mask (bit m - 1) and the degrees flag (bit 6).
//
// SPIRAL ARMS (`Sersic(..., spiral={...})`, GALFIT-style coordinate rotation; definition: Sersic.py
// `Sersic.spiral_image`): ahead of u, v the pixel offsets are deprojected into a disk plane (sky angle, inclination),
// r is the radius there and the coordinates are turned by t = winding T(r) (r / r_out)^alpha, T the tanh ramp between
// r_in and r_out; Sigma_e is divided by cos(inclination).  psfmc_set_spiral_layout appends kSpiIn entries per Sersic
// -- r_in, r_out, winding, alpha, inclination, sky angle as declared (angles in degrees where the layout's
// sersic_degrees flag is set) -- BEHIND the Fourier entries (a context with spirals always carries the Fourier block,
// zeros where a field has no modes); a per (field, Sersic) byte holds the flag (bit 0) and the degrees flag (bit 1).
// The per-walker constants spar[w][k][kSpiPar] are formed by the SPI instantiation of k_general_split, in the thread
// that moves the component's block: no launch is added.
//
// RADIAL LAWS (`Moffat`, `Ferrer`, GALFIT's component types; definition: Sersic.py `Sersic.radial_image`): a general
// component whose value is a function of rho other than the Sersic law, without a centroid term:
//     Moffat  Sigma_0 (1 + g rho^2)^-beta,  g = 4 (2^(1/beta) - 1),  Sigma_0 = F g (beta - 1) / (pi r_a r_b N)
//     Ferrer  Sigma_0 (1 - rho^k)^alpha inside rho = 1, 0 outside,  k = 2 - beta,
//             Sigma_0 = F / (pi r_a r_b N (2/k) B(2/k, alpha + 1))
// N = A(c) Q cos(incl).  The component occupies a Sersic slot of index 1 with r_a, r_b in the places of the effective
// radii, so F / (pi r_a r_b) = Sigma_e 2 e^kappa / kappa^2 comes from the block k_theta_prep made.
// psfmc_set_radial_layout appends kRadIn entries per Sersic -- (beta, unused) or (alpha, beta) -- BEHIND the spiral
// entries.  A context with laws ALWAYS carries the Fourier and the spiral block (zeros / constants inside the support
// where a field has none): a walker's auxiliary vector then has 2 n_sky + 21 n_sersic doubles.  A per (field, Sersic)
// byte holds the kind (0 Sersic, 1 Moffat, 2 Ferrer).  The per-walker constants rpar[w][k][kRadPar] are formed by the
// LAW instantiation of k_general_split.  Such a context runs ONE further instantiation of each of the two kernels
// (FOU, SPI and LAW all set; the kind is a wave-uniform branch); contexts without laws run the kernels they ran.
//
// TRUNCATION (`Sersic / Moffat / Ferrer(..., truncation={'inner': (lo, hi), 'outer': (lo, hi)})`, GALFIT's truncation
// function in spirit; definition: Sersic.py `Sersic.truncation_weight`): the component's value is multiplied by
//     inner = 1 / (1 + exp(-2 a(in_lo, in_hi))),  outer = 1 / (1 + exp(+2 a(out_lo, out_hi))),
//     a(lo, hi) = 2 (2 s - lo - hi) / (hi - lo),  s = r_major rho        ((1 +- tanh a) / 2 without the cancellation)
// with rho the component's own generalised radius (boxiness, modes and winding included) and r_major its semi-major
// radius in pixels: the truncation follows the component's isophotes.  psfmc_set_truncation_layout appends kTruIn
// entries per Sersic -- in_lo, in_hi, out_lo, out_hi -- BEHIND the laws' entries.  A context with truncations ALWAYS
// carries the Fourier, spiral and radial blocks: a walker's auxiliary vector then has 2 n_sky + 25 n_sersic doubles.
// A per (field, Sersic) byte holds the sides (bit 0 inner, bit 1 outer).  The per-walker constants
// tpar[w][k][kTruPar] are formed by the TRU instantiation of k_general_split.  Such a context runs ONE further
// instantiation of each of the two kernels (every flag set; the byte is a wave-uniform branch); contexts without
// truncations run the kernels they ran.  `mag` stays the magnitude of the UNTRUNCATED component.
//
// BENDING MODES (`Sersic / Moffat / Ferrer(..., bending={m: a_m})`, m = 1 ... 4, GALFIT's bending modes; definition:
// Sersic.py `Sersic.bend`): with (u, v) formed as ever (after the winding), r_a = 1 / hypot(m00, m01) and r_b =
// 1 / hypot(m10, m11),
//     v' = v + (r_a / r_b) sum_m a_m u^m
// and everything downstream -- |u|^e + |v'|^e, the angle of eps, the centre, rho of the laws and of the truncation --
// reads (u, v').  A shear with unit Jacobian and f(0) = 0: `mag`, A(c), Q, cos(incl), Sigma_0 and the centre stay.
// psfmc_set_bending_layout appends kBndIn entries per Sersic -- a_1 ... a_4 -- BEHIND the truncations' entries.  A
// context with bending ALWAYS carries the four blocks before it: a walker's auxiliary vector then has 2 n_sky +
// 29 n_sersic doubles.  A per (field, Sersic) byte holds the modes (bit m - 1).  The per-walker constants
// bpar[w][k][kBndPar] = a_m r_a / r_b are formed by the BND instantiation of k_general_split.  Such a context runs ONE
// further instantiation of each kernel (every flag set; the byte is a wave-uniform branch); contexts without bending
// run the kernels they ran.
#pragma once
#include "psfmc_device.h"
#include "psfmc_integrated.h"
#include <type_traits>

namespace psfmc {

constexpr int kGenPar = 12;          // the nine of a Sersic block (Sigma_e / A(c) in [8]), e, 2 / e, spare

// aux[2 k], aux[2 k + 1]: Sky k's slope; aux[2 n_sky + k]: Sersic k's boxiness
__host__ __device__ inline int aux_len(int n_sky, int n_sersic) { return 2 * n_sky + n_sersic; }

constexpr int kFouModes = 6;         // modes 1 ... 6 (PSFMC_FOURIER_MODES)
constexpr int kFouPar = 2 * kFouModes;   // per mode a_m cos(m phi_m), a_m sin(m phi_m); zeros for an absent mode
constexpr int kFouPoints = 128;      // midpoint rule of Q (Sersic.FOURIER_POINTS): two points per lane
constexpr int kFouModeBits = (1 << kFouModes) - 1, kFouDegrees = 1 << kFouModes;
// the Fourier entries behind the aux_len ones: aux[base + kFouPar k + 2 (m - 1)] = a_m, ... + 1 = phi_m of Sersic k
__host__ __device__ inline int fourier_len(int n_sersic) { return kFouPar * n_sersic; }

constexpr int kSpiIn = 6;            // r_in, r_out, winding, alpha, inclination, sky angle (PSFMC_SPIRAL_PARAMS)
constexpr int kSpiPar = 8;           // cos, sin of the sky angle, 1 / cos(incl), k1, k0, alpha, log2 r_out, winding
constexpr int kSpiFlag = 1, kSpiDegrees = 2;
// the spiral entries behind the Fourier ones: aux[base + fourier_len + kSpiIn k + j] of Sersic k
__host__ __device__ inline int spiral_len(int n_sersic) { return kSpiIn * n_sersic; }

constexpr int kRadIn = 2;            // (beta, unused) of a Moffat, (alpha, beta) of a Ferrer (PSFMC_RADIAL_PARAMS)
constexpr int kRadPar = 4;           // Moffat: g, -beta, 0; Ferrer: k / e, k, alpha; then the kind
constexpr int kRadMoffat = 1, kRadFerrer = 2;
// the laws' entries behind the spiral ones: aux[base + fourier_len + spiral_len + kRadIn k + j] of Sersic k
__host__ __device__ inline int radial_len(int n_sersic) { return kRadIn * n_sersic; }

constexpr int kTruIn = 4;            // in_lo, in_hi, out_lo, out_hi (PSFMC_TRUNC_PARAMS)
constexpr int kTruPar = 6;           // inner k1, k0, outer k1, k0 (the ramp's argument is k1 rho + k0), 1 / e, spare
constexpr int kTruInner = 1, kTruOuter = 2;
// the truncations' entries behind the laws': aux[base + fourier_len + spiral_len + radial_len + kTruIn k + j]
__host__ __device__ inline int trunc_len(int n_sersic) { return kTruIn * n_sersic; }

constexpr int kBndModes = 4;         // modes 1 ... 4 (PSFMC_BEND_MODES)
constexpr int kBndIn = kBndModes;    // a_1 ... a_4
constexpr int kBndPar = kBndModes;   // a_m r_a / r_b; zeros for an absent mode
constexpr int kBndModeBits = (1 << kBndModes) - 1;
// the bending entries behind the truncations': aux[base + fourier_len + ... + trunc_len + kBndIn k + (m - 1)]
__host__ __device__ inline int bend_len(int n_sersic) { return kBndIn * n_sersic; }

// skip: the context's own flags (writable) or nullptr (row-based calls without flags: a bad boxiness then makes the
// component, and with it the walker's likelihood, NaN)
// SPI: the context has spirals (spar, smasks set, aux_spi the offset of the spiral entries in a walker's vector); the
// thread of a flagged component also forms the spiral's constants
//     cos(sky), sin(sky), 1 / cos(incl), k1 = 4 / (r_out - r_in), k0 = -2 (r_in + r_out) / (r_out - r_in)  (the ramp's
//     argument is k1 r + k0), alpha, log2 r_out, the winding in radians
// and divides Sigma_e / A(c) by cos(incl); outside the support (a value not finite, r_in < 0, r_out <= r_in,
// alpha < 0, |incl| >= a right angle in its declared unit) Sigma_e becomes NaN and the walker is skipped like a bad
// boxiness.  The SPI = false instantiation is the kernel as it was.
// LAW: the context has radial laws (rpar, rkinds set, aux_rad the offset of their entries); the thread of a slot of
// kind != 0 turns Sigma_e / A(c) into Sigma_0 A(c) Q cos(incl) / (A(c) cos(incl)) -- k_fourier_prep's division by Q
// follows as for every component -- and stores the law's constants: Moffat g, -beta; Ferrer k / e, k, alpha.  Outside
// the support (Moffat: beta not finite or <= 1; Ferrer: alpha or beta not finite, alpha < 0, beta >= 2) the walker
// is skipped like a bad boxiness.  lgamma, exp and expm1 run once per walker and component.
// TRU: the context has truncations (tpar, tmasks set, aux_tru the offset of their entries); the thread of a slot with
// a side forms, per side present, k1 = 4 r_major / (hi - lo) and k0 = -2 (lo + hi) / (hi - lo) with r_major =
// 1 / hypot(m00, m01) the slot's semi-major radius in pixels (zeros for an absent side), and 1 / e.  Outside the
// support of a side present (a value not finite, lo < 0, hi <= lo) Sigma becomes NaN and the walker is skipped like a
// bad boxiness.  The TRU = false instantiations are the kernels as they were.
// BND: the context has bending modes (bpar, bmasks set, aux_bnd the offset of their entries); the thread of a slot with
// a mode stores a_m r_a / r_b per mode present (zeros for an absent one), r_a = 1 / hypot(m00, m01), r_b =
// 1 / hypot(m10, m11).  An amplitude of a mode present that is not finite makes Sigma NaN and the walker is skipped
// like a bad boxiness.  The BND = false instantiations are the kernels as they were.
template <bool SPI, bool LAW = false, bool TRU = false, bool BND = false>
__global__ void k_general_split(double* __restrict__ prep, int plen, uint8_t* __restrict__ skip,
                                double* __restrict__ gpar, const double* __restrict__ aux, int aux_stride, int n_sky,
                                const uint8_t* __restrict__ flags, int n_ps, int n_sersic, int n_psf, int n_psf_field,
                                int n, double* __restrict__ spar, const uint8_t* __restrict__ smasks, int aux_spi,
                                double* __restrict__ rpar = nullptr, const uint8_t* __restrict__ rkinds = nullptr,
                                int aux_rad = 0, double* __restrict__ tpar = nullptr,
                                const uint8_t* __restrict__ tmasks = nullptr, int aux_tru = 0,
                                double* __restrict__ bpar = nullptr, const uint8_t* __restrict__ bmasks = nullptr,
                                int aux_bnd = 0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * n_sersic) return;
    const int w = i / n_sersic, k = i - w * n_sersic;
    // (skip[w] is not read here: sibling threads of the walker may set it in this launch, and every thread does the
    // same work whatever they do -- a skipped walker's record is scratch, its PSF index is clamped below)
    double* rec = prep + (size_t)w * plen;
    int idx = (int)rec[kPrepPsfIdx];
    idx = idx < 0 ? 0 : (idx >= n_psf ? n_psf - 1 : idx);
    if (!flags[(idx / n_psf_field) * n_sersic + k]) return;
    double* b = rec + kPrepHead + kPrepPs * n_ps + kPrepSersic * k;
    double* o = gpar + (size_t)i * kGenPar;
    const double c = aux[(size_t)w * aux_stride + 2 * n_sky + k];
    const double e = c + 2.0;
    bool bad = !(c > -2.0) || !(c < INFINITY);
    // 1 / A(c): the ellipse's area over the superellipse's
    double inv_a = 0.78539816339744830962 * exp(lgamma(1.0 + 2.0 / e) - 2.0 * lgamma(1.0 + 1.0 / e));
    if constexpr (SPI) {
        const int sm = smasks[(idx / n_psf_field) * n_sersic + k];
        if (sm & kSpiFlag) {
            const double* a = aux + (size_t)w * aux_stride + aux_spi + kSpiIn * k;
            const double r_in = a[0], r_out = a[1], alpha = a[3];
            double wind = a[2], incl = a[4], sky = a[5];
            const double quarter = (sm & kSpiDegrees) ? 90.0 : 1.57079632679489661923;
            bool fin = true;
            for (int j = 0; j < kSpiIn; ++j) fin = fin && fabs(a[j]) < INFINITY;     // (false for a NaN)
            bad = bad || !fin || !(r_in >= 0.0) || !(r_out > r_in) || !(alpha >= 0.0) || !(fabs(incl) < quarter);
            if (sm & kSpiDegrees) {
                wind *= M_PI / 180.0;
                incl *= M_PI / 180.0;
                sky *= M_PI / 180.0;
            }
            double sn, cs;
            sincos(sky, &sn, &cs);
            const double ci = cos(incl), span = r_out - r_in;
            double* sp = spar + (size_t)i * kSpiPar;
            sp[0] = cs;
            sp[1] = sn;
            sp[2] = 1.0 / ci;
            sp[3] = 4.0 / span;
            sp[4] = -2.0 * (r_in + r_out) / span;
            sp[5] = alpha;
            sp[6] = log2(r_out);
            sp[7] = wind;
            inv_a /= ci;                                               // (incl = 0: a division by 1, exact)
        }
    }
    if constexpr (LAW) {
        const int kind = rkinds[(idx / n_psf_field) * n_sersic + k];
        if (kind) {
            const double* a = aux + (size_t)w * aux_stride + aux_rad + kRadIn * k;
            const double kap = b[6];
            // F / (pi r_a r_b) over Sigma_e at index 1: 2 n e^kappa kappa^(-2n) Gamma(2n)
            double f = 2.0 * exp(kap) / (kap * kap);
            double* rp = rpar + (size_t)i * kRadPar;
            if (kind == kRadMoffat) {
                const double beta = a[0];
                bad = bad || !(beta > 1.0) || !(beta < INFINITY);
                const double g = 4.0 * expm1(0.69314718055994530942 / beta);
                f *= g * (beta - 1.0);
                rp[0] = g;
                rp[1] = -beta;
                rp[2] = 0.0;
            } else {
                const double alpha = a[0], beta = a[1];
                bad = bad || !(alpha >= 0.0) || !(alpha < INFINITY) || !(beta < 2.0) || !(fabs(beta) < INFINITY);
                const double kk = 2.0 - beta, tk = 2.0 / kk;
                f /= tk * exp(lgamma(tk) + lgamma(alpha + 1.0) - lgamma(tk + alpha + 1.0));
                rp[0] = kk / e;
                rp[1] = kk;
                rp[2] = alpha;
            }
            rp[3] = (double)kind;
            inv_a *= f;
        }
    }
    if constexpr (TRU) {
        const int tm = tmasks[(idx / n_psf_field) * n_sersic + k];
        if (tm) {
            const double* a = aux + (size_t)w * aux_stride + aux_tru + kTruIn * k;
            const double r_major = 1.0 / hypot(b[2], b[3]);
            double* tp = tpar + (size_t)i * kTruPar;
            for (int side = 0; side < 2; ++side) {
                const double lo = a[2 * side], hi = a[2 * side + 1], span = hi - lo;
                const bool on = (tm >> side) & 1;
                if (on) bad = bad || !(lo >= 0.0) || !(hi > lo) || !(hi < INFINITY);
                tp[2 * side] = on ? 4.0 * r_major / span : 0.0;
                tp[2 * side + 1] = on ? -2.0 * (lo + hi) / span : 0.0;
            }
            tp[4] = 1.0 / e;
            tp[5] = 0.0;
        }
    }
    if constexpr (BND) {
        const int bm = bmasks[(idx / n_psf_field) * n_sersic + k];
        if (bm) {
            const double* a = aux + (size_t)w * aux_stride + aux_bnd + kBndIn * k;
            const double r_a = 1.0 / hypot(b[2], b[3]), r_b = 1.0 / hypot(b[4], b[5]);
            const double ratio = r_a / r_b;
            double* bp = bpar + (size_t)i * kBndPar;
            for (int m = 0; m < kBndModes; ++m) {
                const bool on = (bm >> m) & 1;
                if (on) bad = bad || !(fabs(a[m]) < INFINITY);                 // (true for a NaN)
                bp[m] = on ? a[m] * ratio : 0.0;
            }
        }
    }
    for (int j = 0; j < kPrepSersic - 1; ++j) o[j] = b[j];
    o[8] = bad ? __builtin_nan("") : b[8] * inv_a;
    o[9] = e;
    o[10] = 2.0 / e;
    o[11] = 0.0;
    integ_neutral_block(b);
    if (bad && skip) skip[w] = 1;
}

// eps = sum_m a_m cos(m (t + phi_m)) = sum_m (cos(m t) A_m - sin(m t) B_m) from c1 = cos t, s1 = sin t: cos(m t),
// sin(m t) by complex multiplication; modes above `top` (wave-uniform) are absent
struct FouPar { double a[kFouModes], b[kFouModes]; int top; };
__device__ __forceinline__ double fourier_eps(const FouPar& F, double c1, double s1) {
    double cm = c1, sm = s1;
    double eps = __builtin_fma(cm, F.a[0], -(sm * F.b[0]));
#pragma unroll
    for (int m = 1; m < kFouModes; ++m) {
        if (m < F.top) {                                               // wave-uniform
            const double cn = __builtin_fma(cm, c1, -(sm * s1));
            sm = __builtin_fma(sm, c1, cm * s1);
            cm = cn;
            eps += __builtin_fma(cm, F.a[m], -(sm * F.b[m]));
        }
    }
    return eps;
}

// 1 / sqrt(x): v_rsq_f64 and two Newton steps (as fast_rcp); x = 0 gives NaN (inf 0), which is what the centre
// pixel is to be
__device__ __forceinline__ double general_rsqrt(double x) {
    double r = __builtin_amdgcn_rsq(x);
    r = __builtin_fma(0.5 * r, __builtin_fma(-(x * r), r, 1.0), r);
    return __builtin_fma(0.5 * r, __builtin_fma(-(x * r), r, 1.0), r);
}

// A wave per (walker, component): grid ceil(n n_sersic / 4), 4 waves per workgroup.  Lanes 0 ... 5 form their mode's
// A_m = a_m cos(m phi_m), B_m = a_m sin(m phi_m) (zeros for an absent mode) and write them to fpar[w][k][kFouPar];
// every lane then takes two of the kFouPoints points of
//     Q = sum_k w_k (1 + eps(t_k))^-2 / sum_k w_k,   t_k = 2 pi (k + 1/2) / kFouPoints,  w_k = (|cos|^e + |sin|^e)^(-2/e)
// and the two sums are reduced by a fixed xor butterfly (no atomics: the bits do not depend on the batch).  Lane 0
// divides the component's Sigma_e / A(c) (gpar[8], written by k_general_split) by Q.  Outside the support -- an
// amplitude or phase of the component's modes not finite, or sum |a_m| >= 1 in mode order -- gpar[8] becomes NaN and
// the walker is skipped where the flags are writable (skip as for k_general_split).
__global__ void __launch_bounds__(256)
k_fourier_prep(const double* __restrict__ prep, int plen, uint8_t* __restrict__ skip, double* __restrict__ gpar,
               double* __restrict__ fpar, const double* __restrict__ aux, int aux_stride, int aux_base,
               const uint8_t* __restrict__ masks, int n_sersic, int n_psf, int n_psf_field, int n) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (i >= n * n_sersic) return;                                     // wave-uniform
    const int w = i / n_sersic, k = i - w * n_sersic;
    int idx = (int)prep[(size_t)w * plen + kPrepPsfIdx];
    idx = idx < 0 ? 0 : (idx >= n_psf ? n_psf - 1 : idx);
    const int mask = masks[(idx / n_psf_field) * n_sersic + k];
    if (!(mask & kFouModeBits)) return;                                // wave-uniform
    const double* a = aux + (size_t)w * aux_stride + aux_base + kFouPar * k;
    double amp = 0.0, ca = 0.0, sa = 0.0;
    bool fin = true;
    if (lane < kFouModes && ((mask >> lane) & 1)) {
        amp = a[2 * lane];
        double ph = a[2 * lane + 1];
        fin = fabs(amp) < INFINITY && fabs(ph) < INFINITY;             // (false for a NaN)
        if (mask & kFouDegrees) ph *= M_PI / 180.0;
        double sn, cs;
        sincos((double)(lane + 1) * ph, &sn, &cs);
        ca = amp * cs;
        sa = amp * sn;
    }
    FouPar F;
    double sum_abs = 0.0;
#pragma unroll
    for (int m = 0; m < kFouModes; ++m) {
        F.a[m] = __shfl(ca, m, 64);
        F.b[m] = __shfl(sa, m, 64);
        sum_abs += fabs(__shfl(amp, m, 64));
    }
    F.top = kFouModes;
    const bool bad = __any(!fin) || !(sum_abs < 1.0);
    double* g = gpar + (size_t)i * kGenPar;
    const double e = g[9], me2 = -g[10];
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const double t = 6.283185307179586 * ((double)(lane + 64 * half) + 0.5) / (double)kFouPoints;
        double sn, cs;
        sincos(t, &sn, &cs);
        const double wk = pow(pow(fabs(cs), e) + pow(fabs(sn), e), me2);
        const double d = 1.0 + fourier_eps(F, cs, sn);
        num += wk / (d * d);
        den += wk;
    }
    for (int off = 32; off > 0; off >>= 1) {
        num += __shfl_xor(num, off, 64);
        den += __shfl_xor(den, off, 64);
    }
    if (lane < kFouModes) {
        double* o = fpar + (size_t)i * kFouPar;
        o[2 * lane] = ca;
        o[2 * lane + 1] = sa;
    }
    if (lane == 0) {
        g[8] = bad ? __builtin_nan("") : g[8] * (den / num);
        if (bad && skip) skip[w] = 1;
    }
}

// one general component at one pixel: Sigma_e / A exp(-kappa (t - 1)) (1 + (2 kappa p t)^2 / (12 (dx^2 + dy^2))),
// t = (|u|^e + |v|^e)^(2 p / e) -- the reference's formula with rho^2 = (|u|^e + |v|^e)^(2/e) (the elliptical radius of
// its centroid term cancels as in raster_row), through the rasteriser's log2 / exp2
struct GenPar { SersicPar s; double e, pe2, nkl, gk; };
__device__ __forceinline__ GenPar load_general(const double* __restrict__ g) {
    GenPar G;
    G.s = load_sersic(g);
    G.e = g[9];
    G.pe2 = G.s.p * g[10];
    G.nkl = -G.s.kappa * kIntegLog2e;
    G.gk = -2.0 * G.s.kappa * G.s.p * 0.28867513459481288225;      // sqrt(1/12)
    return G;
}
// FOURIER: the component has azimuthal modes -- t = rho^(2p) gains the factor (1 + eps)^(2p), folded into the third
// log2 / exp2 pair at the price of one more fast_log2; cos t, sin t from a reciprocal square root of u^2 + v^2.  The
// FOURIER = false instantiation is the function as it was before the modes existed.
// SPIRAL: the component's coordinates are wound ahead of u, v (file header; `Sersic.spiral_image`); dx, dy of the
// centroid term stay the pixel plane's.  The SPIRAL = false forms are the functions as they were.
struct SpiPar { double cs, sn, icos, ek1, ek0, alpha, l2ro, wind, chk; };
__device__ __forceinline__ SpiPar load_spiral(const double* __restrict__ sp) {
    SpiPar S;
    S.cs = sp[0]; S.sn = sp[1]; S.icos = sp[2];
    // T = (1 + tanh z) / 2 = 1 / (1 + 2^(-2 log2(e) z)), z = k1 r + k0
    S.ek1 = -2.0 * kIntegLog2e * sp[3];
    S.ek0 = -2.0 * kIntegLog2e * sp[4];
    S.alpha = sp[5]; S.l2ro = sp[6]; S.wind = sp[7];
    // (a NaN among the constants reaches the pixel through general_pixel's chk, whatever the clamps do)
    S.chk = ((S.cs + S.sn) + (S.icos + S.ek1)) + ((S.ek0 + S.alpha) + (S.l2ro + S.wind));
    return S;
}
// T at disk-plane radius r.  The exponent is capped at 1000 as in trunc_apply below: a ramp narrow against its radius
// ((r_in + r_out) / (r_out - r_in) above ~177) has an exponent above 1024 inside r_in, where fast_exp2 returns inf and
// the reciprocal's Newton step turns it into NaN; capped, T there is ~1e-301 and the winding angle 0 to every digit.
__device__ __forceinline__ double spiral_ramp(const SpiPar& S, double r) {
    return fast_rcp(1.0 + fast_exp2(__builtin_fmin(__builtin_fma(S.ek1, r, S.ek0), 1000.0)));
}

// sin and cos of t for the winding angle, |t| up to tens (thousands) of radians: t = n pi/2 + r by a two-constant
// Cody-Waite reduction -- with fused multiply-adds the first step's error is one rounding of r, so r is good to
// ~1e-16 + |n| 1.5e-33 -- and the fdlibm kernel polynomials on |r| <= pi/4 (below 1 ulp each).  t not finite: NaN.
__device__ __forceinline__ void spiral_sincos(double t, double* sn, double* cs) {
    const double n = __builtin_rint(t * 0.63661977236758134308);
    double r = __builtin_fma(-n, 1.57079632679489655800e+00, t);
    r = __builtin_fma(-n, 6.12323399573676603587e-17, r);
    const double z = r * r;
    double ps = 1.58969099521155010221e-10;
    ps = __builtin_fma(ps, z, -2.50507602534068634195e-08);
    ps = __builtin_fma(ps, z, 2.75573137070700676789e-06);
    ps = __builtin_fma(ps, z, -1.98412698298579493134e-04);
    ps = __builtin_fma(ps, z, 8.33333333332248946124e-03);
    ps = __builtin_fma(ps, z, -1.66666666666666324348e-01);
    const double s = __builtin_fma(r * z, ps, r);
    double pc = -1.13596475577881948265e-11;
    pc = __builtin_fma(pc, z, 2.08757232129817482790e-09);
    pc = __builtin_fma(pc, z, -2.75573143513906633035e-07);
    pc = __builtin_fma(pc, z, 2.48015872894767294178e-05);
    pc = __builtin_fma(pc, z, -1.38888888888741095749e-03);
    pc = __builtin_fma(pc, z, 4.16666666666666019037e-02);
    const double c = __builtin_fma(z * z, pc, __builtin_fma(-0.5, z, 1.0));
    const int q = (int)(n - 4.0 * __builtin_floor(0.25 * n));          // n mod 4 in 0 ... 3
    const double a = (q & 1) ? c : s, b = (q & 1) ? s : c;
    *sn = (q & 2) ? -a : a;
    *cs = ((q + 1) & 2) ? -b : b;
}

// LAW: the component's radial law is Moffat's or Ferrer's (file header; `Sersic.radial_image`): everything up to
// s = |u|^e + |v|^e and eps is shared, then
//     Moffat  Sigma_0 2^(-beta log2(1 + g rho^2)),  rho^2 = 2^((2/e) log2 s + 2 log2(1 + eps))
//     Ferrer  x = 2^((k/e) log2 s + k log2(1 + eps));  x < 1 ? Sigma_0 2^(alpha log2(1 - x)) : 0
// (alpha = 0: 2^0, exactly Sigma_0), no centroid term, and s = 0 gives Sigma_0 by a select.  The kind is
// wave-uniform.  The LAW = false forms are the functions as they were.
struct RadPar { double a, b, c, chk; int kind; };
__device__ __forceinline__ RadPar load_radial(const double* __restrict__ rp) {
    RadPar R;
    R.a = rp[0]; R.b = rp[1]; R.c = rp[2];
    R.kind = (int)rp[3];
    R.chk = (R.a + R.b) + R.c;       // (a NaN among the constants reaches the pixel through general_pixel's chk)
    return R;
}

// TRU: the component is truncated (file header; `Sersic.truncation_weight`): rho = 2^(log2(s) / e + log2(1 + eps)) from
// the log2 terms the branch holds (0 at s = 0), then per side present one exp2 and one reciprocal,
//     inner = 1 / (1 + 2^(-2 log2(e) (k1 rho + k0))),  outer = 1 / (1 + 2^(+2 log2(e) (k1 rho + k0)))
// (the exponent is capped at 1000, so that the sum stays finite and a factor far outside its ramp is ~1e-301, not the
// NaN of a reciprocal of inf).  The sides are wave-uniform.  The TRU = false forms are the functions as they were.
struct TruPar { double ik1, ik0, ok1, ok0, ie, chk; int sides; };
__device__ __forceinline__ TruPar load_trunc(const double* __restrict__ tp, int sides) {
    TruPar T;
    T.ik1 = -2.0 * kIntegLog2e * tp[0];
    T.ik0 = -2.0 * kIntegLog2e * tp[1];
    T.ok1 = 2.0 * kIntegLog2e * tp[2];
    T.ok0 = 2.0 * kIntegLog2e * tp[3];
    T.ie = tp[4];
    T.sides = sides;
    // (a NaN among the constants reaches the pixel through general_pixel's chk, whatever the clamps do)
    T.chk = ((T.ik1 + T.ik0) + (T.ok1 + T.ok0)) + T.ie;
    return T;
}
// value * inner * outer at generalised radius rho (in units of the semi-major radius)
__device__ __forceinline__ double trunc_apply(const TruPar& T, double val, double rho) {
    if (T.sides & kTruInner)                                           // wave-uniform
        val *= fast_rcp(1.0 + fast_exp2(__builtin_fmin(__builtin_fma(T.ik1, rho, T.ik0), 1000.0)));
    if (T.sides & kTruOuter)                                           // wave-uniform
        val *= fast_rcp(1.0 + fast_exp2(__builtin_fmin(__builtin_fma(T.ok1, rho, T.ok0), 1000.0)));
    return val;
}

// BND: the component is bent (file header; `Sersic.bend`): v' = v + u (b_1 + u (b_2 + u (b_3 + u b_4))) by Horner from
// the highest mode present (`top`, wave-uniform, as FouPar::top), b_m = a_m r_a / r_b: top multiply-adds between
// forming (u, v) and |u|^e + |v|^e.  The BND = false forms are the functions as they were.
// (A NaN among the constants of the modes up to `top` makes v' NaN and so joins general_pixel's chk through u + v'.)
struct BndPar { double b[kBndModes]; int top; };
__device__ __forceinline__ BndPar load_bend(const double* __restrict__ bp, int modes) {
    BndPar B;
#pragma unroll
    for (int m = 0; m < kBndModes; ++m) B.b[m] = bp[m];
    B.top = 32 - __builtin_clz((unsigned)modes);                       // the highest mode present
    return B;
}
__device__ __forceinline__ double bend_apply(const BndPar& B, double u, double v) {
    double f = 0.0;
#pragma unroll
    for (int m = kBndModes - 1; m >= 0; --m)
        if (m < B.top) f = __builtin_fma(f, u, B.b[m]);                // wave-uniform
    return __builtin_fma(f, u, v);
}

template <bool FOURIER, bool SPIRAL = false, bool LAW = false, bool TRU = false, bool BND = false>
__device__ __forceinline__ double general_pixel(const GenPar& G, const FouPar& F, double x, double y,
                                                const SpiPar* SP = nullptr, const RadPar* RP = nullptr,
                                                const TruPar* TP = nullptr, const BndPar* BP = nullptr) {
    const double dx = x - G.s.x0, dy = y - G.s.y0;
    double u, v, spi_chk = 0.0;
    if constexpr (SPIRAL) {
        const SpiPar& S = *SP;
        const double X = __builtin_fma(S.cs, dx, S.sn * dy);
        const double Y = __builtin_fma(S.cs, dy, -(S.sn * dx)) * S.icos;
        const double r2 = __builtin_fma(X, X, Y * Y);
        const bool pos = r2 > 0.0;
        const double r = pos ? r2 * general_rsqrt(r2) : 0.0;
        const double T = spiral_ramp(S, r);
        double wt = S.wind * T;
        if (S.alpha != 0.0)                                            // wave-uniform; (r / r_out)^0 = 1 at r = 0 too
            wt *= pos ? fast_exp2(S.alpha * __builtin_fma(0.5, fast_log2(r2), -S.l2ro)) : 0.0;
        double st, ct;
        spiral_sincos(wt, &st, &ct);
        const double Xr = __builtin_fma(ct, X, st * Y);
        const double Yr = __builtin_fma(ct, Y, -(st * X));
        u = __builtin_fma(G.s.m00, Xr, G.s.m01 * Yr);
        v = __builtin_fma(G.s.m10, Xr, G.s.m11 * Yr);
        spi_chk = S.chk;
    } else {
        u = __builtin_fma(G.s.m00, dx, G.s.m01 * dy);
        v = __builtin_fma(G.s.m10, dx, G.s.m11 * dy);
    }
    if constexpr (BND) v = bend_apply(*BP, u, v);
    const double au = fabs(u), av = fabs(v);
    // |u| = 0 gives the term exactly 0 (not log2(0) e)
    const double pu = au > 0.0 ? fast_exp2(G.e * fast_log2(au)) : 0.0;
    const double pv = av > 0.0 ? fast_exp2(G.e * fast_log2(av)) : 0.0;
    const double s = pu + pv;
    if constexpr (LAW) {
        const RadPar& R = *RP;
        double l1e = 0.0;                                              // log2(1 + eps)
        if constexpr (FOURIER) {
            const double rinv = general_rsqrt(__builtin_fma(u, u, v * v));
            l1e = fast_log2(1.0 + fourier_eps(F, u * rinv, v * rinv));
        }
        const double ls = fast_log2(s);
        double val;
        if (R.kind == kRadMoffat) {                                    // wave-uniform
            const double rho2 = fast_exp2(__builtin_fma(G.pe2 + G.pe2, ls, l1e + l1e));      // (p = 1/2: pe2 = 1/e)
            val = G.s.sbeff * fast_exp2(R.b * fast_log2(__builtin_fma(R.a, rho2, 1.0)));
        } else {
            const double xk = fast_exp2(__builtin_fma(R.a, ls, R.b * l1e));
            val = xk < 1.0 ? G.s.sbeff * fast_exp2(R.c * fast_log2(1.0 - xk)) : 0.0;
        }
        val = s > 0.0 ? val : G.s.sbeff;                               // the centre: Sigma_0, finite
        double chk = (u + v) + (G.s.sbeff + R.chk);    // (the comparisons and the exponentials' clamps swallow a NaN)
        if constexpr (SPIRAL) chk += spi_chk;
        if constexpr (TRU) {
            // (the centre: the factors at rho = 0; a NaN of l1e there is never read)
            val = trunc_apply(*TP, val, s > 0.0 ? fast_exp2(__builtin_fma(TP->ie, ls, l1e)) : 0.0);
            chk += TP->chk;
        }
        return chk == chk ? val : chk;
    }
    double t, rho = 0.0;
    if constexpr (FOURIER) {
        const double rinv = general_rsqrt(__builtin_fma(u, u, v * v));
        const double eps = fourier_eps(F, u * rinv, v * rinv);
        // (1 + eps > 0 inside the support; a NaN of the centre pixel is swallowed by the clamps and comes back
        // through the 0 * inf of the last term, as without modes)
        const double l1e = fast_log2(1.0 + eps), ls = fast_log2(s);
        const double l1 = (G.s.p + G.s.p) * l1e;
        t = s > 0.0 ? fast_exp2(__builtin_fma(G.pe2, ls, l1)) : 0.0;
        if constexpr (TRU) rho = s > 0.0 ? fast_exp2(__builtin_fma(TP->ie, ls, l1e)) : 0.0;
    } else {
        const double ls = fast_log2(s);
        t = s > 0.0 ? fast_exp2(G.pe2 * ls) : 0.0;
        if constexpr (TRU) rho = s > 0.0 ? fast_exp2(TP->ie * ls) : 0.0;
    }
    const double sb = G.s.sbeff * fast_exp2_floor(__builtin_fma(G.nkl, t, -G.nkl));
    const double gt = G.gk * t;
    double val = sb * __builtin_fma(gt * gt, fast_rcp(__builtin_fma(dx, dx, dy * dy)), 1.0);
    double chk = (u + v) + (G.nkl + G.pe2);            // (the comparisons and the exponentials' clamps swallow a NaN)
    if constexpr (SPIRAL) chk += spi_chk;
    if constexpr (TRU) {
        val = trunc_apply(*TP, val, rho);
        chk += TP->chk;
    }
    return chk == chk ? val : chk;
}

// grid (ceil(ny / 4), n), 4 waves = 4 rows per workgroup.  add != 0: the pixel-integrated profile's kernels have
// written the walkers' extra images, this one adds to them; else it writes them.
// Only the field's own ly x lx corner of a walker's [ny][nx] slot is written (as k_integ_rows does); the EXTRA
// readers clip to the same ly, lx from wrap_tab and never read beyond it.
// FOU: the context has Fourier modes (fpar, fmasks set); the FOU = false instantiation is the kernel as it was before
// the modes existed -- its registers and occupancy are not paid for by contexts without modes.
// SPI: the context has spirals (spar, smasks set); a component with the flag runs the SPIRAL pixel function, with or
// without modes.  The SPI = false instantiations are the kernels as they were.
// LAW: the context has radial laws (rpar, rkinds set; instantiated with FOU and SPI set only, such a context carries
// both blocks); a slot of kind != 0 runs the LAW pixel function, with or without modes and spiral.
// TRU: the context has truncations (tpar, tmasks set; instantiated with every other flag set only, such a context
// carries every block); a slot with a side runs the TRU pixel function of its law, with or without modes and spiral.
// BND: the context has bending modes (bpar, bmasks set; instantiated with every other flag set only); a slot with a
// mode runs the BND pixel function of its law, with or without modes, spiral and truncation.
template <bool FOU, bool SPI = false, bool LAW = false, bool TRU = false, bool BND = false>
__global__ void __launch_bounds__(256)
k_general_rows(const double* __restrict__ prep, int plen, const uint8_t* __restrict__ skip,
               const double* __restrict__ gpar, const double* __restrict__ aux, int aux_stride, int n_sky,
               const uint8_t* __restrict__ sky_flags, const uint8_t* __restrict__ flags, int n_sersic, int n_psf,
               int n_psf_field, const WrapDesc* __restrict__ wrap_tab, int ny, int nx, double* __restrict__ img,
               int add, const double* __restrict__ fpar, const uint8_t* __restrict__ fmasks,
               const double* __restrict__ spar = nullptr, const uint8_t* __restrict__ smasks = nullptr,
               const double* __restrict__ rpar = nullptr, const uint8_t* __restrict__ rkinds = nullptr,
               const double* __restrict__ tpar = nullptr, const uint8_t* __restrict__ tmasks = nullptr,
               const double* __restrict__ bpar = nullptr, const uint8_t* __restrict__ bmasks = nullptr) {
    const int w = blockIdx.y;
    if (skip && skip[w]) return;
    const int lane = threadIdx.x & 63;
    const int iy = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int idx = integ_psf_index(prep + (size_t)w * plen, n_psf);
    const int ly = wrap_tab ? wrap_tab[idx].ly : ny, lx = wrap_tab ? wrap_tab[idx].lx : nx;
    if (iy >= ly || iy >= ny) return;
    const int field = idx / n_psf_field;
    const uint8_t* fl = flags + field * n_sersic;
    const uint8_t* sfl = sky_flags + field * n_sky;
    const double* a = aux + (size_t)w * aux_stride;
    double* out = img + ((size_t)w * ny + iy) * nx;
    const double y = (double)iy;
    const double cx = 0.5 * (double)(lx - 1), cy = 0.5 * (double)(ly - 1);
    const int xn = lx < nx ? lx : nx;
    // what the row holds before the general components: the image the integrated kernels wrote (add) plus the skies'
    // slope terms.  Each lane owns its pixels, so the passes below need no synchronisation.
    auto base = [&](int ix) {
        double acc = add ? out[ix] : 0.0;
        for (int k = 0; k < n_sky; ++k) {
            if (!sfl[k]) continue;                                     // wave-uniform
            acc += __builtin_fma(a[2 * k], (double)ix - cx, a[2 * k + 1] * (y - cy));
        }
        return acc;
    };
    // components outermost: a component's parameters are loaded and its constants formed once per row, not per
    // 64-pixel chunk; the first flagged component's pass starts from `base`, the later ones add to the row
    bool first = true;
    for (int k = 0; k < n_sersic; ++k) {
        if (!fl[k]) continue;                                          // wave-uniform
        const GenPar G = load_general(gpar + ((size_t)w * n_sersic + k) * kGenPar);
        FouPar F{};
        // a component without modes runs the loop it always ran
        const int modes = FOU ? fmasks[field * n_sersic + k] & kFouModeBits : 0;         // wave-uniform
        const bool wound = SPI ? (smasks[field * n_sersic + k] & kSpiFlag) != 0 : false; // wave-uniform
        if (FOU && modes) {
            const double* f = fpar + ((size_t)w * n_sersic + k) * kFouPar;
#pragma unroll
            for (int m = 0; m < kFouModes; ++m) {
                F.a[m] = f[2 * m];
                F.b[m] = f[2 * m + 1];
            }
            F.top = 32 - __builtin_clz((unsigned)modes);                                 // the highest mode present
        }
        const int kind = LAW ? rkinds[field * n_sersic + k] : 0;                         // wave-uniform
        const int sides = TRU ? tmasks[field * n_sersic + k] : 0;                        // wave-uniform
        const int bends = BND ? bmasks[field * n_sersic + k] & kBndModeBits : 0;         // wave-uniform
        if (BND && bends) {
            const BndPar B = load_bend(bpar + ((size_t)w * n_sersic + k) * kBndPar, bends);
            TruPar T{};
            RadPar R{};
            SpiPar S{};
            if (sides) T = load_trunc(tpar + ((size_t)w * n_sersic + k) * kTruPar, sides);
            if (kind) R = load_radial(rpar + ((size_t)w * n_sersic + k) * kRadPar);
            if (wound) S = load_spiral(spar + ((size_t)w * n_sersic + k) * kSpiPar);
            auto pass = [&](auto fou, auto spi, auto law, auto tru) {
                for (int x0 = 0; x0 < xn; x0 += 64) {
                    const int ix = x0 + lane;
                    if (ix < xn)
                        out[ix] = (first ? base(ix) : out[ix]) +
                                  general_pixel<decltype(fou)::value, decltype(spi)::value, decltype(law)::value,
                                                decltype(tru)::value, true>(G, F, (double)ix, y, &S, &R, &T, &B);
                }
            };
            auto by_tru = [&](auto fou, auto spi, auto law) {
                if (sides) pass(fou, spi, law, std::true_type{});
                else pass(fou, spi, law, std::false_type{});
            };
            auto by_law = [&](auto fou, auto spi) {
                if (kind) by_tru(fou, spi, std::true_type{});
                else by_tru(fou, spi, std::false_type{});
            };
            if (wound) {
                if (modes) by_law(std::true_type{}, std::true_type{});
                else by_law(std::false_type{}, std::true_type{});
            } else {
                if (modes) by_law(std::true_type{}, std::false_type{});
                else by_law(std::false_type{}, std::false_type{});
            }
        } else if (TRU && sides) {
            const TruPar T = load_trunc(tpar + ((size_t)w * n_sersic + k) * kTruPar, sides);
            RadPar R{};
            SpiPar S{};
            if (kind) R = load_radial(rpar + ((size_t)w * n_sersic + k) * kRadPar);
            if (wound) S = load_spiral(spar + ((size_t)w * n_sersic + k) * kSpiPar);
            auto pass = [&](auto fou, auto spi, auto law) {
                for (int x0 = 0; x0 < xn; x0 += 64) {
                    const int ix = x0 + lane;
                    if (ix < xn)
                        out[ix] = (first ? base(ix) : out[ix]) +
                                  general_pixel<decltype(fou)::value, decltype(spi)::value, decltype(law)::value,
                                                true>(G, F, (double)ix, y, &S, &R, &T);
                }
            };
            auto by_law = [&](auto fou, auto spi) {
                if (kind) pass(fou, spi, std::true_type{});
                else pass(fou, spi, std::false_type{});
            };
            if (wound) {
                if (modes) by_law(std::true_type{}, std::true_type{});
                else by_law(std::false_type{}, std::true_type{});
            } else {
                if (modes) by_law(std::true_type{}, std::false_type{});
                else by_law(std::false_type{}, std::false_type{});
            }
        } else if (LAW && kind) {
            const RadPar R = load_radial(rpar + ((size_t)w * n_sersic + k) * kRadPar);
            SpiPar S{};
            if (wound) S = load_spiral(spar + ((size_t)w * n_sersic + k) * kSpiPar);
            auto pass = [&](auto fou, auto spi) {
                for (int x0 = 0; x0 < xn; x0 += 64) {
                    const int ix = x0 + lane;
                    if (ix < xn)
                        out[ix] = (first ? base(ix) : out[ix]) +
                                  general_pixel<decltype(fou)::value, decltype(spi)::value, true>(G, F, (double)ix, y,
                                                                                                  &S, &R);
                }
            };
            if (wound) {
                if (modes) pass(std::true_type{}, std::true_type{});
                else pass(std::false_type{}, std::true_type{});
            } else {
                if (modes) pass(std::true_type{}, std::false_type{});
                else pass(std::false_type{}, std::false_type{});
            }
        } else if (SPI && wound) {
            const SpiPar S = load_spiral(spar + ((size_t)w * n_sersic + k) * kSpiPar);
            if (FOU && modes) {
                for (int x0 = 0; x0 < xn; x0 += 64) {
                    const int ix = x0 + lane;
                    if (ix < xn)
                        out[ix] = (first ? base(ix) : out[ix]) + general_pixel<true, true>(G, F, (double)ix, y, &S);
                }
            } else {
                for (int x0 = 0; x0 < xn; x0 += 64) {
                    const int ix = x0 + lane;
                    if (ix < xn)
                        out[ix] = (first ? base(ix) : out[ix]) + general_pixel<false, true>(G, F, (double)ix, y, &S);
                }
            }
        } else if (FOU && modes) {
            for (int x0 = 0; x0 < xn; x0 += 64) {
                const int ix = x0 + lane;
                if (ix < xn) out[ix] = (first ? base(ix) : out[ix]) + general_pixel<true>(G, F, (double)ix, y);
            }
        } else {
            for (int x0 = 0; x0 < xn; x0 += 64) {
                const int ix = x0 + lane;
                if (ix < xn) out[ix] = (first ? base(ix) : out[ix]) + general_pixel<false>(G, F, (double)ix, y);
            }
        }
        first = false;
    }
    if (first)
        for (int x0 = 0; x0 < xn; x0 += 64) {
            const int ix = x0 + lane;
            if (ix < xn) out[ix] = base(ix);
        }
}

}  // namespace psfmc
