// psfmc_theta.h -- raw emcee parameter vectors on the device: priors for the
// common distribution families, the Sersic constants (kappa = b_n, Sigma_e) and
// the expansion into prep records, so that a batch needs no host arithmetic.
//
// Reference: packing contract ComponentBase.py:45-74 + models.py:174-185; priors
// distributions.py:112-127 (scipy.stats frozen logpdf / logpmf) and Sersic.py:41-45;
// kappa Sersic.py:47-53 (scipy.special.gammaincinv(2n, 1/2)); Sigma_e Sersic.py:55-71;
// flux utils.py:160-164; ellipse matrix Sersic.py:80-91.
#pragma once
#ifndef PSFMC_PART
#define PSFMC_PART 0      /* single translation unit (see psfmc_hip.hip) */
#endif
#include "psfmc_device.h"

namespace psfmc {

enum PriorFamily { PRIOR_HOST = 0, PRIOR_UNIFORM = 1, PRIOR_NORMAL = 2, PRIOR_WEIBULL_MIN = 3,
                   PRIOR_RANDINT = 4, PRIOR_TRUNCNORM = 5, PRIOR_LOGNORM = 6, PRIOR_HALFNORM = 7,
                   PRIOR_EXPON = 8, PRIOR_LAPLACE = 9, PRIOR_CAUCHY = 10, PRIOR_HALFCAUCHY = 11,
                   PRIOR_LOGISTIC = 12, PRIOR_T = 13, PRIOR_BETA = 14, PRIOR_RECIPROCAL = 15,
                   PRIOR_WEIBULL_MAX = 16, PRIOR_INVGAMMA = 17, PRIOR_N_FAMILIES = 18 };
constexpr int kPriorNpar = 4;           // parameters per column in psfmc_set_priors

// slots of a model, in this order: n_sky x [adu] | n_ps x [mag, x, y] |
// n_sersic x [angle, index, mag, reff, reff_b, x, y] | [psf_index]
__host__ __device__ inline int n_slots(int n_sky, int n_ps, int n_sersic) {
    return n_sky + 3 * n_ps + 7 * n_sersic + 1;
}

struct ThetaLayout {
    int n_sky, n_ps, n_sersic, n_params, n_psf;
    double mag_zp;
    const int* slot_col;        // [n_slots] column of theta, or -1
    const double* slot_const;   // [n_slots]
    const int* ps_method;       // [n_ps]
    const int* sersic_deg;      // [n_sersic] angle in degrees?
    const int* family;          // [n_params]
    const double* pa;           // [n_params] loc / c / low
    const double* pb;           // [n_params] scale / loc / high
    const double* pc;           // [n_params] - / scale / -
    const double* pd;           // [n_params] families 5..: see prior_prepare
    const double* pk;           // [n_params] the family's constant log term (prior_log_norm,
                                //            prior_prepare), filled by psfmc_set_layout / _priors
    // auxiliary parameters (psfmc_set_aux_layout, psfmc_general.h): per Sky its two slope values, then per
    // Sersic its boxiness; entries as slot_col / slot_const.  n_aux = 0: none (the layout of a model without
    // the keywords).  These two tables stay in global memory.
    int n_aux;
    const int* aux_col;         // [n_aux] column of theta, or -1
    const double* aux_const;    // [n_aux]
    // azimuthal Fourier modes (psfmc_set_fourier_layout): the LAST n_fou = 12 n_sersic of the n_aux entries, per
    // Sersic and mode 1 ... 6 an amplitude and a phase; 0: none (every layout before the call)
    int n_fou;
    // spiral arms (psfmc_set_spiral_layout): the LAST n_spi = 6 n_sersic of the n_aux entries, behind the Fourier
    // ones (n_spi > 0 implies n_fou > 0: a field with a spiral carries the Fourier block, empty without modes); per
    // Sersic r_in, r_out, winding, alpha, inclination, sky angle; 0: none (every layout before the call)
    int n_spi;
    // radial laws (psfmc_set_radial_layout): the LAST n_rad = 2 n_sersic of the n_aux entries, behind the spiral ones
    // (n_rad > 0 implies n_fou > 0 and n_spi > 0: a field with a law carries both blocks, empty without the
    // keywords); per Sersic slot (beta, unused) of a Moffat or (alpha, beta) of a Ferrer; rad_kind [n_sersic] in
    // global memory: 0 Sersic, 1 Moffat, 2 Ferrer; 0 / nullptr: none (every layout before the call)
    int n_rad;
    const int* rad_kind;
    // truncations (psfmc_set_truncation_layout): the LAST n_tru = 4 n_sersic of the n_aux entries, behind the laws'
    // (n_tru > 0 implies the three blocks before it, empty without the keywords); per Sersic slot in_lo, in_hi, out_lo,
    // out_hi; tru_side [n_sersic] in global memory: bit 0 inner, bit 1 outer; 0 / nullptr: none (every layout before
    // the call)
    // bending modes (psfmc_set_bending_layout): the LAST n_bnd = 4 n_sersic of the n_aux entries, behind the
    // truncations' (n_bnd > 0 implies the four blocks before it, empty without the keywords); per Sersic slot a_1 ... a_4,
    // zeros for absent modes; 0: none (every layout before the call).  (Between n_tru and the pointer: the struct keeps
    // its size.)
    int n_tru;
    int n_bnd;
    const int* tru_side;
    // ties (psfmc_set_ties): an entry e <= -2 of slot_col, aux_col or a block's columns names tie t = -2 - e, whose
    // value is ratio * theta[source] + offset (theta_value).  tie_col [3 n_ties]: the source columns, then the ratio
    // columns, then the offset columns (-1: the constant); tie_const [2 n_ties]: the ratio constants, then the offset
    // constants.  Both stay in global memory beside the aux tables; 0 / nullptr: none (a model without ties).
    int n_ties;
    const int* tie_col;
    const double* tie_const;
};

// where k_theta_prep writes the walkers' auxiliary vectors: aux[w][stride] (stride: the context's, the same for
// every field; a field whose layout has n_aux = 0 writes nothing)
struct AuxOut {
    double* aux;
    int stride;
};

// ---------------------------------------------------------------------------
// regularised lower incomplete gamma P(a, x), series form (valid and fast for
// x < a + 1, which brackets the median), and its inverse at 1/2
// ---------------------------------------------------------------------------
// x^a e^-x / Gamma(a+1), the prefactor of the series.  Below a = 20 it is formed
// directly from Gamma(a) (`tg`, which the caller needs for Sigma_e anyway: one OCML
// tgamma instead of lgamma + tgamma); from a = 20 on, Gamma(a+1) = sqrt(2 pi a) (a/e)^a
// exp(corr(a)) avoids the cancellation of a ln x - x against ln Gamma, and `stirling`
// = ln sqrt(2 pi a) + corr(a) depends on a only.
__device__ inline double igam_stirling_term(double a) {
    const double ia = 1.0 / a, ia2 = ia * ia;
    const double corr = ia * (1.0 / 12.0 + ia2 * (-1.0 / 360.0 + ia2 * (1.0 / 1260.0 + ia2 *
                        (-1.0 / 1680.0 + ia2 * (1.0 / 1188.0 + ia2 * (-691.0 / 360360.0))))));
    return 0.5 * log(6.28318530717958647693 * a) + corr;
}
__device__ inline double igam_prefactor(double a, double x, double tg, double stirling) {
    if (a < 20.0) return exp(a * log(x) - x) / (a * tg);
    const double u = (x - a) / a;
    return exp(a * (log1p(u) - u) - stirling);
}

// kappa = gammaincinv(a, 1/2), a = 2n > 0.  `tg` = tgamma(a) (used for a < 20 only).
__device__ inline double gamma_median(double a, double tg) {
    if (!(a > 0.0) || !(a < 1e6)) return __builtin_nan("");
    double x;
    if (a < 1.0) {
        x = exp(log(0.5 * a * tg) / a);                         // P ~ x^a / Gamma(a+1)
    } else {
        // Ciotti & Bertin (1999) eq. 18, plus a fitted remainder i^3 (c0 + c1 i + c2 i^2)
        // (least squares against gammaincinv over n in [0.5, 40]): relative error of the
        // start <= 1.1e-7 instead of 3.6e-4 at n = 0.5, so ONE Halley step is enough
        const double n = 0.5 * a, i = 1.0 / n;
        x = a - 1.0 / 3.0 + i * (4.0 / 405.0 + i * (46.0 / 25515.0 + i * (131.0 / 1148175.0 -
            i * (2194697.0 / 30690717750.0))));
        x -= i * i * i * (2.47501670e-05 + i * (3.05002372e-05 - i * 1.35458779e-05));
    }
    const double stirling = a < 20.0 ? 0.0 : igam_stirling_term(a);
    // Halley on P(a, x) = 1/2: cubic convergence, so a step below 1e-6 x leaves an
    // error of order 1e-18 x and the iteration stops there
    for (int it = 0; it < 12; ++it) {
        const double pre = igam_prefactor(a, x, tg, stirling);    // x^a e^-x / Gamma(a+1)
        // four terms per round: their reciprocals do not depend on each other, so the dependent chain
        // is four multiplications instead of four reciprocals (k_theta_prep is latency-bound: one
        // lane per walker)
        double term = 1.0, sum = 1.0, ap = a;
        for (int k = 0; k < 500; ++k) {
            const double q1 = x * fast_rcp(ap + 1.0), q2 = x * fast_rcp(ap + 2.0);
            const double q3 = x * fast_rcp(ap + 3.0), q4 = x * fast_rcp(ap + 4.0);
            ap += 4.0;
            const double t1 = term * q1, t2 = t1 * q2, t3 = t2 * q3;
            term = t3 * q4;
            sum = (((sum + t1) + t2) + t3) + term;
            if (term < 1e-17 * sum) break;
        }
        const double f = sum * pre - 0.5;
        const double d1 = pre * a / x;                            // dP/dx = x^(a-1) e^-x / Gamma(a)
        const double r = f / d1;
        const double dx = r / (1.0 + 0.5 * r * (1.0 - (a - 1.0) / x));
        x -= dx;
        if (!(x > 0.0)) x = 0.5 * (x + dx);
        if (fabs(dx) <= 1e-6 * x) break;
    }
    return x;
}

// Sigma_e (Sersic.py:55-71); tg = tgamma(2n)
__device__ inline double sersic_sb_eff(double flux, double n, double reff, double reff_b, double kappa,
                                       double tg) {
    return flux / (M_PI * reff * reff_b * 2.0 * n * exp(kappa + log(kappa) * -2.0 * n) * tg);
}

// ---------------------------------------------------------------------------
// priors
// ---------------------------------------------------------------------------
// The x-independent term of each family's log-density, computed once on the host
// (ten log() calls per walker otherwise).
__host__ inline double prior_log_norm(int fam, double a, double b, double c) {
    switch (fam) {
        case PRIOR_UNIFORM: return -log(b);
        case PRIOR_NORMAL: return -0.91893853320467274178 - log(b);
        case PRIOR_WEIBULL_MIN: return log(a) - log(c);
        case PRIOR_RANDINT: return -log(b - a);
        default: return 0.0;
    }
}

// log Phi(x), the standard normal CDF: erfc on the side away from zero, and below -20 the asymptotic
// series of the Mills ratio (Abramowitz & Stegun 26.2.12; the tenth term is < 1e-20 there)
__host__ inline double prior_log_ndtr(double x) {
    if (x >= 0.0) return log1p(-0.5 * erfc(x * 0.70710678118654752440));
    if (x > -20.0) return log(0.5 * erfc(-x * 0.70710678118654752440));
    const double r = 1.0 / (x * x);
    double term = 1.0, sum = 1.0;
    for (int k = 1; k <= 10; ++k) {
        term *= -(2.0 * k - 1.0) * r;
        sum += term;
    }
    return -0.5 * x * x - log(-x) - 0.91893853320467274178 + log(sum);
}

// log(Phi(b) - Phi(a)), a < b: both bounds in the left tail, mirrored when both are in the right one
__host__ inline double prior_log_gauss_mass(double a, double b) {
    if (b <= 0.0 || a > 0.0) {
        const double hi = b <= 0.0 ? prior_log_ndtr(b) : prior_log_ndtr(-a);
        const double lo = b <= 0.0 ? prior_log_ndtr(a) : prior_log_ndtr(-b);
        return hi + log1p(-exp(lo - hi));
    }
    return log1p(-0.5 * erfc(-a * 0.70710678118654752440) - 0.5 * erfc(b * 0.70710678118654752440));
}

// Would scipy.stats accept these parameters?  (`_argcheck`, scale > 0; randint: integer low < high.)
// p = the family's scipy arguments in order (include/psfmc_hip.h PSFMC_PRIOR_*).  Locations, scales and
// shapes must also be finite, and truncnorm's bounds not NaN (an infinite bound is allowed).
__host__ inline bool prior_params_ok(int fam, const double* p) {
    auto fin = [](double v) { return std::isfinite(v); };
    auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
    switch (fam) {
        case PRIOR_HOST: return true;
        case PRIOR_UNIFORM: case PRIOR_NORMAL: return fin(p[0]) && pos(p[1]);
        case PRIOR_WEIBULL_MIN: case PRIOR_WEIBULL_MAX: case PRIOR_LOGNORM: case PRIOR_T: case PRIOR_INVGAMMA:
            return pos(p[0]) && fin(p[1]) && pos(p[2]);
        case PRIOR_RANDINT:
            return fin(p[0]) && fin(p[1]) && p[0] == rint(p[0]) && p[1] == rint(p[1]) && p[0] < p[1];
        case PRIOR_TRUNCNORM:
            return !std::isnan(p[0]) && !std::isnan(p[1]) && p[0] < p[1] && fin(p[2]) && pos(p[3]);
        case PRIOR_HALFNORM: case PRIOR_EXPON: case PRIOR_LAPLACE: case PRIOR_CAUCHY: case PRIOR_HALFCAUCHY:
        case PRIOR_LOGISTIC:
            return fin(p[0]) && pos(p[1]);
        case PRIOR_BETA: return pos(p[0]) && pos(p[1]) && fin(p[2]) && pos(p[3]);
        case PRIOR_RECIPROCAL: return pos(p[0]) && fin(p[1]) && p[1] > p[0] && fin(p[2]) && pos(p[3]);
        default: return false;
    }
}

// The per-column table entry {pa, pb, pc, pd, pk} of one prior (p as for prior_params_ok, already
// checked).  Families 1-4 keep psfmc_set_layout's form.  Families 5.. hold pa = loc, pb = scale, two
// shape terms pc, pd and in pk every x-independent term, -log(scale) included, so that the device
// works out y = (x - loc) / scale and at most a log, a log1p and one exp per column.
__host__ inline void prior_prepare(int fam, const double* p, double* out) {
    const double log_pi = 1.14472988584940017414, half_log_2pi = 0.91893853320467274178;
    double pa = 0.0, pb = 0.0, pc = 0.0, pd = 0.0, pk = 0.0;
    switch (fam) {
        case PRIOR_UNIFORM: case PRIOR_NORMAL: case PRIOR_WEIBULL_MIN: case PRIOR_RANDINT:
            pa = p[0]; pb = p[1]; pc = fam == PRIOR_WEIBULL_MIN ? p[2] : 0.0;
            pk = prior_log_norm(fam, pa, pb, pc);
            break;
        case PRIOR_TRUNCNORM:                      // pc, pd = the bounds a, b
            pa = p[2]; pb = p[3]; pc = p[0]; pd = p[1];
            pk = -half_log_2pi - prior_log_gauss_mass(p[0], p[1]) - log(pb);
            break;
        case PRIOR_LOGNORM:                        // pd = 2 s^2
            pa = p[1]; pb = p[2]; pc = p[0]; pd = 2.0 * (p[0] * p[0]);
            pk = -log(p[0] * 2.50662827463100050242) - log(pb);
            break;
        case PRIOR_HALFNORM: case PRIOR_EXPON: case PRIOR_LAPLACE: case PRIOR_CAUCHY: case PRIOR_HALFCAUCHY:
        case PRIOR_LOGISTIC:
            pa = p[0]; pb = p[1];
            pk = -log(pb);
            if (fam == PRIOR_HALFNORM) pk = 0.5 * log(2.0 / M_PI) - log(pb);
            if (fam == PRIOR_CAUCHY) pk = -log_pi - log(pb);
            if (fam == PRIOR_HALFCAUCHY) pk = log(2.0 / M_PI) - log(pb);
            break;
        case PRIOR_T: {                            // pc = df, pd = (df + 1) / 2
            const long double h = 0.5L * (long double)p[0];
            pa = p[1]; pb = p[2]; pc = p[0]; pd = (p[0] + 1.0) / 2.0;
            pk = (double)(lgammal(h + 0.5L) - lgammal(h)) - 0.5 * (log(p[0]) + log_pi) - log(pb);
            break;
        }
        case PRIOR_BETA: {                         // pc = a - 1, pd = b - 1
            const long double a = p[0], b = p[1];
            pa = p[2]; pb = p[3]; pc = p[0] - 1.0; pd = p[1] - 1.0;
            pk = -(double)(lgammal(a) + lgammal(b) - lgammal(a + b)) - log(pb);
            break;
        }
        case PRIOR_RECIPROCAL:                     // pc, pd = the bounds a, b
            pa = p[2]; pb = p[3]; pc = p[0]; pd = p[1];
            pk = -log(log(p[1]) - log(p[0])) - log(pb);
            break;
        case PRIOR_WEIBULL_MAX:                    // pc = c, pd = c - 1
            pa = p[1]; pb = p[2]; pc = p[0]; pd = p[0] - 1.0;
            pk = log(p[0]) - log(pb);
            break;
        case PRIOR_INVGAMMA:                       // pc = a + 1
            pa = p[1]; pb = p[2]; pc = p[0] + 1.0;
            pk = -(double)lgammal((long double)p[0]) - log(pb);
            break;
        default: break;
    }
    out[0] = pa; out[1] = pb; out[2] = pc; out[3] = pd; out[4] = pk;
}

// log-density of one column: families 1-4 with set_layout's parameters here, families 5.. in
// prior_logp_more as scipy's `_logpdf(y) - log(scale)` in scipy's own form (its lazywhere branches and
// support masks: closed, or open for lognorm and invgamma), so that the edges of the support give scipy's
// value.  NaN in, NaN out.
__device__ inline double prior_logp(int fam, double x, double a, double b, double c, double k) {
    const double ninf = -INFINITY;
    switch (fam) {
        case PRIOR_UNIFORM: {                                 // loc a, scale b
            const double y = (x - a) / b;
            return (y >= 0.0 && y <= 1.0) ? k : (y == y ? ninf : y);
        }
        case PRIOR_NORMAL: {                                  // loc a, scale b
            const double z = (x - a) / b;
            return -0.5 * z * z + k;
        }
        case PRIOR_WEIBULL_MIN: {                             // c a, loc b, scale c
            const double y = (x - b) / c;
            if (!(y >= 0.0)) return y == y ? ninf : y;
            if (y == 0.0) return a == 1.0 ? k : (a < 1.0 ? INFINITY : ninf);
            return k + (a - 1.0) * log(y) - pow(y, a);
        }
        case PRIOR_RANDINT: {                                 // low a, high b (exclusive); x already rounded
            return (x >= a && x <= b - 1.0) ? k : ninf;
        }
        default:
            return 0.0;
    }
}

// families 5..: loc a, scale b.  `fam` is the same in every lane (one column at a time): the dispatch is
// scalar, and families 1-4 never reach it (theta_log_prior)
__device__ inline double prior_logp_more(int fam, double x, double a, double b, double c, double d, double k) {
    const double ninf = -INFINITY;
    const double y = (x - a) / b;
    switch (__builtin_amdgcn_readfirstlane(fam)) {
        case PRIOR_TRUNCNORM:                                 // [c, d]
            if (!(y >= c && y <= d)) return y == y ? ninf : y;
            return -0.5 * y * y + k;
        case PRIOR_LOGNORM: {                                 // (0, inf); d = 2 s^2
            if (!(y > 0.0 && y < INFINITY)) return y == y ? ninf : y;
            const double l = log(y);
            return -(l * l) / d - l + k;
        }
        case PRIOR_HALFNORM:                                  // [0, inf]
            if (!(y >= 0.0)) return y == y ? ninf : y;
            return -0.5 * y * y + k;
        case PRIOR_EXPON:
            if (!(y >= 0.0)) return y == y ? ninf : y;
            return -y + k;
        case PRIOR_LAPLACE:                                   // scipy: log(pdf), which underflows past |y| ~ 745
            return log(0.5 * exp(-fabs(y))) + k;
        case PRIOR_CAUCHY: {
            const double ay = fabs(y);
            if (ay < 1.0) return -log1p(ay * ay) + k;
            const double r = 1.0 / ay;
            return -(2.0 * log(ay) + log1p(r * r)) + k;
        }
        case PRIOR_HALFCAUCHY:
            if (!(y >= 0.0)) return y == y ? ninf : y;
            return -log1p(y * y) + k;
        case PRIOR_LOGISTIC: {
            const double t = -fabs(y);
            return t - 2.0 * log1p(exp(t)) + k;
        }
        case PRIOR_T:                                         // c = df, d = (df + 1) / 2
            return -d * log1p(y * y / c) + k;
        case PRIOR_BETA: {                                    // [0, 1]; c = a - 1, d = b - 1 (xlogy, xlog1py)
            if (!(y >= 0.0 && y <= 1.0)) return y == y ? ninf : y;
            const double t1 = d == 0.0 ? 0.0 : d * log1p(-y);
            const double t2 = c == 0.0 ? 0.0 : c * log(y);
            return (t1 + t2) + k;
        }
        case PRIOR_RECIPROCAL:                                // [c, d]
            if (!(y >= c && y <= d)) return y == y ? ninf : y;
            return -log(y) + k;
        case PRIOR_WEIBULL_MAX: {                             // [-inf, 0]; c = shape, d = c - 1
            if (!(y <= 0.0)) return y == y ? ninf : y;
            const double u = -y;
            return (k + (d == 0.0 ? 0.0 : d * log(u))) - pow(u, c);
        }
        case PRIOR_INVGAMMA:                                  // (0, inf); c = a + 1
            if (!(y > 0.0 && y < INFINITY)) return y == y ? ninf : y;
            return (-c * log(y) - 1.0 / y) + k;
        default:
            return 0.0;
    }
}

// The work of one walker is split into independent TASKS that run on different waves
// of the workgroup (blockDim = (64 walkers, n waves)): one walker per thread left the
// whole GPU with two waves crawling through ~9000 dependent fp64 instructions (35 us
// for a 128-walker half-ensemble, a sixth of an MCMC half-step).
//   task 0                       joint log-prior (device families + the host's extra),
//                                support and axis-ratio checks -> lnprior, skip; sky, PSF index
//   tasks 1 + 2k, 2 + 2k         PointSource k: flux and the y / the x axis of its window
//   then 2 per Sersic            the ellipse + flux, and Gamma(2n) + kappa
// after a barrier one wave per Sersic forms Sigma_e and its prep block, and after another
// task 0's wave writes the head of the prep record from the largest peak estimate.
// Walkers outside the prior support get skip = 1; their prep record is scratch.
// The value a table entry stands for in one walker's vector: column `entry` of theta, the constant (-1), or tie
// t = -2 - entry: ratio * theta[source] + offset as two separately rounded operations, product then sum -- the
// roundings of numpy's `ratio * source + offset`, so no FMA contraction.  Every reader of slot_col, aux_col and the
// blocks' columns goes through here.
__device__ inline double theta_value(const ThetaLayout& L, const double* __restrict__ theta, int entry, double konst) {
#pragma clang fp contract(off)
    // a layout without ties decides on a scalar (n_ties comes with the kernel's arguments): its readers do not wait
    // for the table entry before they know that there is no tie to look for
    const double plain = entry >= 0 ? theta[entry] : konst;
    if (L.n_ties == 0 || entry >= -1) return plain;
    // the five table entries are read unconditionally: independent loads, one round trip to global memory (the
    // kernels that come here are chains of latencies)
    const int t = -2 - entry, n = L.n_ties;
    const int sc = L.tie_col[t], rc = L.tie_col[n + t], oc = L.tie_col[2 * n + t];
    const double rk = L.tie_const[t], ok = L.tie_const[n + t];
    const double r = rc >= 0 ? theta[rc] : rk;
    const double o = oc >= 0 ? theta[oc] : ok;
    const double prod = r * theta[sc];
    return prod + o;
}

__device__ inline double theta_slot(const ThetaLayout& L, const double* __restrict__ theta, int s) {
    return theta_value(L, theta, L.slot_col[s], L.slot_const[s]);
}

// Sersic axis-ratio constraint (Sersic.py:41-45): -inf if some component has reff_b > reff, else lp
__device__ inline double theta_axis_ratio(const ThetaLayout& L, const double* __restrict__ theta, double lp) {
    for (int k = 0; k < L.n_sersic; ++k) {
        const int s0 = L.n_sky + 3 * L.n_ps + 7 * k;
        if (theta_slot(L, theta, s0 + 4) > theta_slot(L, theta, s0 + 3)) lp = -INFINITY;
    }
    return lp;
}

__device__ inline double theta_log_prior(const ThetaLayout& L, const double* __restrict__ theta, double extra) {
    double lp = extra;
    for (int p = 0; p < L.n_params; ++p) {
        const int fam = L.family[p];
        if (fam == PRIOR_HOST) continue;
        const double x = fam == PRIOR_RANDINT ? rint(theta[p]) : theta[p];
        if (fam <= PRIOR_RANDINT) lp += prior_logp(fam, x, L.pa[p], L.pb[p], L.pc[p], L.pk[p]);
        else lp += prior_logp_more(fam, x, L.pa[p], L.pb[p], L.pc[p], L.pd[p], L.pk[p]);
    }
    return theta_axis_ratio(L, theta, lp);
}

// row pieces (the caller-row layout of include/psfmc_hip.h)
__device__ inline void theta_ps_row(const ThetaLayout& L, const double* __restrict__ theta, int k,
                                    double* __restrict__ r) {
    const int s0 = L.n_sky + 3 * k;
    r[0] = pow(10.0, -0.4 * (theta_slot(L, theta, s0) - L.mag_zp));
    r[1] = theta_slot(L, theta, s0 + 1);
    r[2] = theta_slot(L, theta, s0 + 2);
    r[3] = (double)L.ps_method[k];
}

// Sersic row in three independent pieces: the ellipse (sincos), kappa (tgamma + the
// incomplete-gamma inversion), and Sigma_e, which needs both.  scratch = {Gamma(2n), flux}.
__device__ inline void theta_sersic_geometry(const ThetaLayout& L, const double* __restrict__ theta, int k,
                                             double* __restrict__ r, double* __restrict__ scratch) {
    const int s0 = L.n_sky + 3 * L.n_ps + 7 * k;
    const double ang = theta_slot(L, theta, s0), mag = theta_slot(L, theta, s0 + 2);
    const double re = theta_slot(L, theta, s0 + 3), rb = theta_slot(L, theta, s0 + 4);
    const double th = (L.sersic_deg[k] ? ang * (M_PI / 180.0) : ang) + 0.5 * M_PI;
    const double sn = sin(th), cs = cos(th);
    r[0] = theta_slot(L, theta, s0 + 5);
    r[1] = theta_slot(L, theta, s0 + 6);
    r[2] = cs / re;
    r[3] = sn / re;
    r[4] = -sn / rb;
    r[5] = cs / rb;
    scratch[1] = pow(10.0, -0.4 * (mag - L.mag_zp));
}

__device__ inline void theta_sersic_kappa(const ThetaLayout& L, const double* __restrict__ theta, int k,
                                          double* __restrict__ r, double* __restrict__ scratch) {
    const double n = theta_slot(L, theta, L.n_sky + 3 * L.n_ps + 7 * k + 1);
    const double tg = tgamma(2.0 * n);
    r[6] = gamma_median(2.0 * n, tg);
    r[7] = 0.5 / n;
    scratch[0] = tg;
}

__device__ inline void theta_sersic_sigma(const ThetaLayout& L, const double* __restrict__ theta, int k,
                                          double* __restrict__ r, const double* __restrict__ scratch) {
    const int s0 = L.n_sky + 3 * L.n_ps + 7 * k;
    r[8] = sersic_sb_eff(scratch[1], theta_slot(L, theta, s0 + 1), theta_slot(L, theta, s0 + 3),
                         theta_slot(L, theta, s0 + 4), r[6], scratch[0]);
}

// Stretch-move proposal formed while the parameter tile is loaded (pos != nullptr):
// q[i] = c[j_i] - z_i (c[j_i] - s_i), s = half `h` of pos, c = the other half
// (Goodman & Weare 2010; emcee 2.2.1 `_propose_stretch`).  No FMA contraction: the
// same three roundings as the numpy expression emcee uses.  The iteration number
// comes from *d_iter when a captured hipGraph of one iteration is replayed, else `it`.
struct StretchIn {
    const double* pos;      // [2 half][P] current positions, or nullptr: theta is given
    double* q;              // [half][P] proposals (kept for the accept step)
    const double* z;        // [n_iter][2][half]
    const int* partner;     // [n_iter][2][half]
    const int* d_iter;
    int it, half, h;
    // Several fields in one launch (contexts of psfmc_ctx_create_fields; blockIdx.y = field): every
    // field is its own ensemble of 2 half walkers with its own random numbers.  Element strides
    // between consecutive fields of pos / q / z (and partner); 0 in a one-field launch.
    size_t pos_stride, q_stride, rand_stride;
    // spec = 1 (small ensembles, one field): ONE launch proposes a whole iteration -- 3 half walkers:
    //   [0, half)        the first half's proposals (as h = 0),
    //   [half, 2 half)   the second half's proposals IF the partner's proposal is accepted (the partner's
    //                    position is then its proposal, formed here again with the same three roundings),
    //   [2 half, 3 half) the second half's proposals if it is rejected (the partner stays where it is).
    // The accept step of the second half picks the row its partner's outcome selects (k_stretch_finish), so the
    // chain is the one of two half-steps run after each other, bit for bit, at one pipeline pass per iteration.
    int spec;
    // n_ens > 0 (parallel tempering, psfmc_pt_run): the launch's records are the half-step proposals of n_ens
    // ensembles of 2 half walkers that share field 0, flattened -- record r belongs to ensemble t = r / half,
    // whose walkers are rows [t 2 half, (t + 1) 2 half) of pos; the random numbers are [n_iter][2][n_ens][half],
    // so record r reads entry ((it 2 + h) n_ens) half + r.  0 everywhere else.
    int n_ens;
};

// the fields of one k_theta_prep launch (gridDim.y > 1): field f takes layouts[f], image sides sides[2 f],
// sides[2 f + 1], walkers [f W, (f + 1) W) of every per-walker array, kernel spectra from f * psf_stride on
struct FieldSegs {
    const ThetaLayout* layouts;   // device array [gridDim.y], or nullptr: one field, the layout passed by value
    const int* sides;             // device array [gridDim.y][2] (fields may differ in image size)
    int psf_stride;
    int shared_theta;             // 1 (joint fits): every field reads the same W vectors of theta / extra
};

__device__ inline double stretch_point(double s, double c, double z) {
#pragma clang fp contract(off)
    const double diff = c - s;
    const double step = z * diff;
    return c - step;
}

// LDS bytes of k_theta_prep: the layout tables, per walker its parameter vector and
// its derived row (the walk through the slots is a long chain of dependent small
// loads: from global memory it cost 45 us per call, from LDS it is a few us), and
// the components' peak estimates
constexpr int kThetaThreads = 64;       // walkers per workgroup
constexpr int kThetaMaxTasks = 8;       // waves per workgroup; further tasks loop
__host__ inline int theta_task_waves(int n_ps, int n_sersic) {
    const int t = 1 + 2 * n_ps + 2 * n_sersic;
    return t > kThetaMaxTasks ? kThetaMaxTasks : t;
}
__host__ inline size_t theta_prep_lds_bytes(int n_sky, int n_ps, int n_sersic, int n_params) {
    const size_t ns = n_slots(n_sky, n_ps, n_sersic);
    const size_t n_int = ((ns + n_ps + n_sersic + n_params + 1) / 2) * 2;           // 8-byte multiple
    const size_t n_dbl = ns + 5 * (size_t)n_params;
    return n_int * sizeof(int) +
           (n_dbl + (size_t)kThetaThreads * (n_params + row_len(n_ps, n_sersic) + n_ps + 3 * n_sersic)) *
               sizeof(double);
}

#if PSFMC_PART == 0          /* not a template: defined in the API part only */
__global__ void __launch_bounds__(kThetaThreads * kThetaMaxTasks)
k_theta_prep(ThetaLayout G, const double* __restrict__ theta,
             const double* __restrict__ extra, double* __restrict__ rows,
             double* __restrict__ prep, double* __restrict__ lnprior,
             uint8_t* __restrict__ skip, int W, int ny, int nx,
             const double* __restrict__ rho, StretchIn sp, int psf_base, FieldSegs segs, AuxOut ax) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    if (segs.layouts) {                                 // (wave-uniform) this workgroup's field
        const int f = blockIdx.y;
        G = segs.layouts[f];
        ny = segs.sides[2 * f];
        nx = segs.sides[2 * f + 1];
        const size_t first = (size_t)f * W;             // its first walker in the per-walker arrays
        const size_t first_in = segs.shared_theta ? 0 : first;
        if (theta) theta += first_in * G.n_params;
        if (extra) extra += first_in;
        if (rows) rows += first * row_len(G.n_ps, G.n_sersic);
        prep += first * prep_len(G.n_ps, G.n_sersic);
        lnprior += first;
        skip += first;
        if (ax.aux) ax.aux += first * ax.stride;
        psf_base += f * segs.psf_stride;
        if (sp.pos) {
            sp.pos += (size_t)f * sp.pos_stride;
            sp.q += (size_t)f * sp.q_stride;
            sp.z += (size_t)f * sp.rand_stride;
            sp.partner += (size_t)f * sp.rand_stride;
        }
    }
    const int ns = n_slots(G.n_sky, G.n_ps, G.n_sersic);
    const int n_int = ((ns + G.n_ps + G.n_sersic + G.n_params + 1) / 2) * 2;
    const int n_dbl = ns + 5 * G.n_params;
    const int rlen = row_len(G.n_ps, G.n_sersic);
    const int P = G.n_params;
    int* li = reinterpret_cast<int*>(lds_raw);
    double* ld = reinterpret_cast<double*>(lds_raw + (size_t)n_int * sizeof(int));
    double* th_tile = ld + n_dbl;
    double* row_tile = th_tile + (size_t)kThetaThreads * P;
    double* peak_tile = row_tile + (size_t)kThetaThreads * rlen;       // [component][walker]
    const int tid = threadIdx.y * kThetaThreads + threadIdx.x, nthr = kThetaThreads * blockDim.y;
    // The four int tables and the six double tables are contiguous in the blob.  The layout
    // tables and the parameter tile are independent: every thread first ISSUES its (first) load
    // of each, then stores them to LDS -- one memory round trip instead of three in a row (the
    // kernel is a chain of latencies: 16 us for a 128-walker half-step whatever the batch).
    const int n_tab_i = ns + G.n_ps + G.n_sersic + P;
    const int w0 = blockIdx.x * kThetaThreads;
    const int n_here = W - w0 < kThetaThreads ? W - w0 : kThetaThreads;
    const int n_tile = n_here * P;
    int first_i = 0;
    double first_d = 0.0, first_t = 0.0;
    if (tid < n_tab_i) first_i = G.slot_col[tid];
    if (tid < n_dbl) first_d = G.slot_const[tid];
    size_t soff = 0;
    double s_own = 0.0, c_other = 0.0, zz = 0.0;
    // element i = lw P + d of the tile in a whole-iteration launch (sp.spec)
    auto propose_spec = [&](int i, size_t off0) -> double {
        const int lw = i / P, d = i - lw * P, w3 = w0 + lw;
        const int seg = w3 / sp.half, w = w3 - seg * sp.half;
        const size_t off1 = off0 + sp.half;
        if (seg == 0)
            return stretch_point(sp.pos[(size_t)w * P + d],
                                 sp.pos[(size_t)(sp.half + sp.partner[off0 + w]) * P + d], sp.z[off0 + w]);
        const int j = sp.partner[off1 + w];                          // a walker of the first half
        double cj = sp.pos[(size_t)j * P + d];
        if (seg == 1)
            cj = stretch_point(cj, sp.pos[(size_t)(sp.half + sp.partner[off0 + j]) * P + d], sp.z[off0 + j]);
        return stretch_point(sp.pos[(size_t)(sp.half + w) * P + d], cj, sp.z[off1 + w]);
    };
    if (sp.pos && sp.spec) {
        const int it = sp.d_iter ? *sp.d_iter : sp.it;
        soff = (size_t)it * 2 * sp.half;
    } else if (sp.pos) {                                            // propose into the tile
        const int it = sp.d_iter ? *sp.d_iter : sp.it;
        soff = ((size_t)it * 2 + sp.h) * sp.half * (sp.n_ens ? sp.n_ens : 1);
        if (tid < n_tile) {
            const int lw = tid / P, d = tid - lw * P, w = w0 + lw;
            const int e = sp.n_ens ? (w / sp.half) * sp.half : 0;   // (n_ens) ensemble t = w / half: t half
            s_own = sp.pos[(size_t)(e + sp.h * sp.half + w) * P + d];
            c_other = sp.pos[(size_t)(2 * e + (1 - sp.h) * sp.half + sp.partner[soff + w]) * P + d];
            zz = sp.z[soff + w];
        }
    } else if (tid < n_tile) {
        first_t = theta[(size_t)w0 * P + tid];
    }
    if (tid < n_tab_i) li[tid] = first_i;
    if (tid < n_dbl) ld[tid] = first_d;
    for (int i = tid + nthr; i < n_tab_i; i += nthr) li[i] = G.slot_col[i];
    for (int i = tid + nthr; i < n_dbl; i += nthr) ld[i] = G.slot_const[i];
    if (sp.pos && sp.spec) {
        for (int i = tid; i < n_tile; i += nthr) {
            const double q = propose_spec(i, soff);
            th_tile[i] = q;
            sp.q[(size_t)w0 * P + i] = q;
        }
    } else if (sp.pos) {
        if (tid < n_tile) {
            const double q = stretch_point(s_own, c_other, zz);
            th_tile[tid] = q;
            sp.q[(size_t)w0 * P + tid] = q;
        }
        for (int i = tid + nthr; i < n_tile; i += nthr) {
            const int lw = i / P, d = i - lw * P, w = w0 + lw;
            const int e = sp.n_ens ? (w / sp.half) * sp.half : 0;
            const double s = sp.pos[(size_t)(e + sp.h * sp.half + w) * P + d];
            const double c = sp.pos[(size_t)(2 * e + (1 - sp.h) * sp.half + sp.partner[soff + w]) * P + d];
            const double q = stretch_point(s, c, sp.z[soff + w]);
            th_tile[i] = q;
            sp.q[(size_t)w0 * P + i] = q;
        }
    } else {
        if (tid < n_tile) th_tile[tid] = first_t;
        for (int i = tid + nthr; i < n_tile; i += nthr)             // coalesced tile load
            th_tile[i] = theta[(size_t)w0 * P + i];
    }
    __syncthreads();
    ThetaLayout L = G;
    L.slot_col = li; L.ps_method = li + ns; L.sersic_deg = li + ns + G.n_ps;
    L.family = li + ns + G.n_ps + G.n_sersic;
    L.slot_const = ld; L.pa = ld + ns; L.pb = ld + ns + P; L.pc = ld + ns + 2 * P; L.pd = ld + ns + 3 * P;
    L.pk = ld + ns + 4 * P;
    const int lw = threadIdx.x, w = w0 + lw;
    const bool active = w < W;
    const double* th = th_tile + (size_t)lw * P;
    double* row = row_tile + (size_t)lw * rlen;
    double* my_prep = prep + (size_t)(active ? w : 0) * prep_len(G.n_ps, G.n_sersic);
    double* sersic_scratch = peak_tile + (size_t)(G.n_ps + G.n_sersic) * kThetaThreads;   // [sersic][2][walker]
    const int n_tasks = 1 + 2 * G.n_ps + 2 * G.n_sersic;
    bool ok = false;
    for (int task = threadIdx.y; task < n_tasks; task += blockDim.y) {      // wave-uniform
        if (!active) continue;
        if (task == 0) {
            double lp = theta_log_prior(L, th, extra ? extra[w] : 0.0);
            if (G.n_aux > 0) {                                              // wave-uniform
                // the walker's auxiliary vector; a boxiness <= -2 or not finite is outside the support (as
                // reff_b > reff is)
                double* a = ax.aux + (size_t)w * ax.stride;
                const int n_base = G.n_aux - G.n_fou - G.n_spi - G.n_rad - G.n_tru - G.n_bnd;
                for (int j = 0; j < n_base; ++j) {
                    const double v = theta_value(L, th, G.aux_col[j], G.aux_const[j]);
                    a[j] = v;
                    if (j >= 2 * G.n_sky && (!(v > -2.0) || !(v < INFINITY))) lp = -INFINITY;
                }
                if (G.n_fou > 0) {                                          // wave-uniform
                    // the Fourier entries, per Sersic 6 x (amplitude, phase); a value that is not finite or
                    // sum |a_m| >= 1 (in mode order) is outside the support
                    for (int j0 = n_base; j0 < n_base + G.n_fou; j0 += 12) {
                        double sum_abs = 0.0;
                        bool fin = true;
                        for (int j = j0; j < j0 + 12; ++j) {
                            const double v = theta_value(L, th, G.aux_col[j], G.aux_const[j]);
                            a[j] = v;
                            fin = fin && fabs(v) < INFINITY;
                            if (!((j - j0) & 1)) sum_abs += fabs(v);
                        }
                        if (!fin || !(sum_abs < 1.0)) lp = -INFINITY;
                    }
                }
                if (G.n_spi > 0) {                                          // wave-uniform
                    // the spiral entries, per Sersic r_in, r_out, winding, alpha, inclination, sky angle; outside
                    // the support: a value not finite, r_in < 0, r_out <= r_in, alpha < 0, |inclination| >= a
                    // right angle in its declared unit
                    int k = 0;
                    for (int j0 = n_base + G.n_fou; j0 < n_base + G.n_fou + G.n_spi; j0 += 6, ++k) {
                        double v6[6];
                        bool fin = true;
                        for (int j = 0; j < 6; ++j) {
                            const double v = theta_value(L, th, G.aux_col[j0 + j], G.aux_const[j0 + j]);
                            a[j0 + j] = v;
                            v6[j] = v;
                            fin = fin && fabs(v) < INFINITY;
                        }
                        const double quarter = L.sersic_deg[k] ? 90.0 : 1.57079632679489661923;
                        if (!fin || !(v6[0] >= 0.0) || !(v6[1] > v6[0]) || !(v6[3] >= 0.0) || !(fabs(v6[4]) < quarter))
                            lp = -INFINITY;
                    }
                }
                if (G.n_rad > 0) {                                          // wave-uniform
                    // the radial laws' entries, per Sersic slot two; outside the support: a Moffat's beta not
                    // finite or <= 1; a Ferrer's alpha or beta not finite, alpha < 0 or beta >= 2
                    int k = 0;
                    for (int j0 = G.n_aux - G.n_bnd - G.n_tru - G.n_rad; j0 < G.n_aux - G.n_bnd - G.n_tru; j0 += 2, ++k) {
                        const double v0 = theta_value(L, th, G.aux_col[j0], G.aux_const[j0]);
                        const double v1 = theta_value(L, th, G.aux_col[j0 + 1], G.aux_const[j0 + 1]);
                        a[j0] = v0;
                        a[j0 + 1] = v1;
                        const int kind = G.rad_kind[k];
                        if (kind == 1 && (!(v0 > 1.0) || !(v0 < INFINITY))) lp = -INFINITY;
                        if (kind == 2 && (!(v0 >= 0.0) || !(v0 < INFINITY) || !(v1 < 2.0) || !(fabs(v1) < INFINITY)))
                            lp = -INFINITY;
                    }
                }
                if (G.n_tru > 0) {                                          // wave-uniform
                    // the truncations' entries, per Sersic slot two pairs (lo, hi); outside the support of a side
                    // present: a value not finite, lo < 0 or hi <= lo
                    int k = 0;
                    for (int j0 = G.n_aux - G.n_bnd - G.n_tru; j0 < G.n_aux - G.n_bnd; j0 += 4, ++k) {
                        const int sides = G.tru_side[k];
                        for (int j = 0; j < 4; j += 2) {
                            const double lo = theta_value(L, th, G.aux_col[j0 + j], G.aux_const[j0 + j]);
                            const double hi = theta_value(L, th, G.aux_col[j0 + j + 1], G.aux_const[j0 + j + 1]);
                            a[j0 + j] = lo;
                            a[j0 + j + 1] = hi;
                            if (((sides >> (j >> 1)) & 1) && (!(lo >= 0.0) || !(hi > lo) || !(hi < INFINITY)))
                                lp = -INFINITY;
                        }
                    }
                }
                if (G.n_bnd > 0) {                                          // wave-uniform
                    // the bending amplitudes, per Sersic slot four (zeros for absent modes); outside the support: a
                    // value not finite
                    for (int j = G.n_aux - G.n_bnd; j < G.n_aux; ++j) {
                        const double v = theta_value(L, th, G.aux_col[j], G.aux_const[j]);
                        a[j] = v;
                        if (!(fabs(v) < INFINITY)) lp = -INFINITY;
                    }
                }
            }
            ok = lp == lp && fabs(lp) != INFINITY;                          // finite
            lnprior[w] = lp;
            skip[w] = ok ? 0 : 1;
            double sky = 0.0;
            for (int k = 0; k < L.n_sky; ++k) sky += theta_slot(L, th, k);
            row[0] = sky;
            double psf = rint(theta_slot(L, th, ns - 1));
            psf = psf < 0.0 ? 0.0 : (psf > (double)(L.n_psf - 1) ? (double)(L.n_psf - 1) : psf);
            row[rlen - 1] = psf;
        } else if (task <= 2 * G.n_ps) {
            // both axis tasks derive the (identical) row piece; each writes its own half of
            // the prep block, the y task also the row and the peak estimate
            const int k = (task - 1) >> 1, axis = (task - 1) & 1;
            double rr[kRowPs];
            theta_ps_row(L, th, k, rr);
            prep_ps_axis(rr, my_prep + kPrepHead + kPrepPs * k, axis, axis ? nx : ny);
            if (axis == 0) {
                double* r = row + kRowSky + kRowPs * k;
                for (int j = 0; j < kRowPs; ++j) r[j] = rr[j];
                peak_tile[k * kThetaThreads + lw] = fabs(rr[0]);
            }
        } else {
            const int j = task - 1 - 2 * G.n_ps, k = j >> 1;
            double* r = row + kRowSky + kRowPs * G.n_ps + kRowSersic * k;
            double scr[2];
            if (j & 1) {
                theta_sersic_kappa(L, th, k, r, scr);
                sersic_scratch[(k * 2 + 0) * kThetaThreads + lw] = scr[0];
            } else {
                theta_sersic_geometry(L, th, k, r, scr);
                sersic_scratch[(k * 2 + 1) * kThetaThreads + lw] = scr[1];
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.y; k < G.n_sersic; k += blockDim.y) {            // wave-uniform
        if (!active) continue;
        double* r = row + kRowSky + kRowPs * G.n_ps + kRowSersic * k;
        const double scr[2] = {sersic_scratch[(k * 2 + 0) * kThetaThreads + lw],
                               sersic_scratch[(k * 2 + 1) * kThetaThreads + lw]};
        theta_sersic_sigma(L, th, k, r, scr);
        peak_tile[(G.n_ps + k) * kThetaThreads + lw] =
            prep_sersic_block(r, my_prep + kPrepHead + kPrepPs * G.n_ps + kPrepSersic * k);
    }
    __syncthreads();
    if (threadIdx.y != 0 || !active) return;
    double peak = fabs(row[0]);
    for (int k = 0; k < G.n_ps + G.n_sersic; ++k) peak = fmax(peak, peak_tile[k * kThetaThreads + lw]);
    // psf_base: first kernel-spectrum index of this walker's field (contexts holding several fields)
    prep_head(my_prep, row[0], psf_base + (int)row[rlen - 1], peak, rho);
    if (rows && ok) {
        double* out = rows + (size_t)w * rlen;
        for (int i = 0; i < rlen; ++i) out[i] = row[i];
    }
}
#endif

// A walker is nf field records, field f's at w + f fstride of the per-record arrays (nf = 1, fstride = 0: an
// ordinary walker).  Its log-likelihood is ((ll_0 + ll_1) + ...) + ll_{nf-1}, each ll_f the one-field sum.  The
// sum is returned unguarded: walker_lnprob and walker_loglike each keep their own skip and finiteness tests, so
// that the product, the sum and the `+ lnprior` compile to what they would standing alone.
__device__ inline double walker_field_sum(const double* __restrict__ partial, int nblk, int w, int lane, int nf,
                                          int fstride) {
    double ll = -0.5 * wave_sum_partials(partial + (size_t)w * nblk, nblk, lane);
    for (int f = 1; f < nf; ++f)
        ll += -0.5 * wave_sum_partials(partial + (w + (size_t)f * fstride) * nblk, nblk, lane);
    return ll;
}

// lnprob = loglike + lnprior, non-finite likelihood -> -inf (models.py:238-243); all
// lanes of the walker's wave get the value.  A joint walker is -inf if any field's record is skipped; lnprior[w]
// (field 0's record) is its joint log-prior.
__device__ inline double walker_lnprob(const double* __restrict__ partial, const uint8_t* __restrict__ skip,
                                       const double* __restrict__ lnprior, int nblk, int w, int lane,
                                       int nf = 1, int fstride = 0) {
    for (int f = 0; f < nf; ++f)
        if (skip[w + (size_t)f * fstride]) return -INFINITY;
    const double ll = walker_field_sum(partial, nblk, w, lane, nf, fstride);
    const bool fin = ll == ll && fabs(ll) != INFINITY;
    return fin ? ll + lnprior[w] : -INFINITY;
}

// one wave per walker (launch: finish_blocks(W) x kFinishThreads); nf, fstride: see walker_lnprob
#if PSFMC_PART == 0          /* not a template: defined in the API part only */
__global__ void k_finish_posterior(const double* __restrict__ partial, const uint8_t* __restrict__ skip,
                                   const double* __restrict__ lnprior, double* __restrict__ lnprob,
                                   int W, int nblk, int nf, int fstride) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (kFinishThreads / 64) + (threadIdx.x >> 6);
    if (w >= W) return;
    const double lp = walker_lnprob(partial, skip, lnprior, nblk, w, lane, nf, fstride);
    if (lane == 0) lnprob[w] = lp;
}
#endif

// ---------------------------------------------------------------------------
// stretch move, second half of a half-step: the proposals' log-posteriors
// (k_finish_posterior's sum), acceptance where lz + newlnp - lnp > ln u (emcee 2.2.1
// `_propose_stretch`), the move, and the chain entry of this half's walkers -- the
// other half's positions do not change during this half-step, so iteration `it` of
// walker g is final after the half-step that owns g.  One wave per walker (launch:
// finish_blocks(half) x kFinishThreads).
// `newlnp_in` (multi-GPU): the proposals' log-posteriors were evaluated in blocks on several
// ranks and gathered; they are read from it instead of being summed here -- the values are the
// ones k_finish_posterior produced from the same partial sums, so the chain is the same bit for bit.
// Joint fits (psfmc_stretch_run_joint; one ensemble, gridDim.y = 1): each proposal is nf field records,
// summed as k_finish_posterior sums them (nf, fstride = half).
// ---------------------------------------------------------------------------
#if PSFMC_PART == 0          /* not a template: defined in the API part only */
__global__ void k_stretch_finish(const double* __restrict__ partial, const uint8_t* __restrict__ skip,
                                 const double* __restrict__ lnprior, int nblk,
                                 const double* __restrict__ newlnp_in,
                                 double* __restrict__ pos, double* __restrict__ lnprob,
                                 const double* __restrict__ q, const double* __restrict__ lz,
                                 const double* __restrict__ log_u, long long* __restrict__ nacc,
                                 double* __restrict__ chain, double* __restrict__ lnchain,
                                 const int* __restrict__ d_iter, int it_val, int n_iter, int half, int h,
                                 int P, size_t rand_stride, uint8_t* __restrict__ acc_out,
                                 const uint8_t* __restrict__ acc_in, const int* __restrict__ partner,
                                 int nf, int fstride) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (kFinishThreads / 64) + (threadIdx.x >> 6);
    if (w >= half) return;                                   // wave-uniform
    if (gridDim.y > 1) {                                     // several fields (psfmc_stretch_run_fields): blockIdx.y's ensemble
        const size_t f = blockIdx.y;
        partial += f * half * nblk;
        skip += f * half;
        lnprior += f * half;
        if (newlnp_in) newlnp_in += f * half;
        pos += f * 2 * half * P;
        lnprob += f * 2 * half;
        q += f * half * P;
        lz += f * rand_stride;
        log_u += f * rand_stride;
        nacc += f * 2 * half;
        if (chain) {
            chain += f * 2 * half * n_iter * P;
            lnchain += f * 2 * half * n_iter;
        }
    }
    const int it = d_iter ? *d_iter : it_val;
    const size_t off = ((size_t)it * 2 + h) * half;
    // whole-iteration launches (StretchIn::spec): the second half's walker takes the proposal row its
    // partner's outcome selects -- half + w if the partner moved, 2 half + w if it stayed
    int row = w;
    if (acc_in) row = w + (acc_in[partner[off + w]] ? half : 2 * half);
    const double newlnp = newlnp_in ? newlnp_in[w] : walker_lnprob(partial, skip, lnprior, nblk, row, lane, nf, fstride);
    const int g = h * half + w;
    double lp = lnprob[g];
    const double diff = (lz[off + w] + newlnp) - lp;
    const bool accept = diff > log_u[off + w];               // the same in every lane
    if (accept) lp = newlnp;
    for (int d = lane; d < P; d += 64) {                     // lane d moves coordinate d
        double v;
        if (accept) {
            v = q[(size_t)row * P + d];
            pos[(size_t)g * P + d] = v;
        } else {
            v = pos[(size_t)g * P + d];
        }
        if (chain) chain[((size_t)g * n_iter + it) * P + d] = v;
    }
    if (lane == 0) {
        if (acc_out) acc_out[w] = accept ? 1 : 0;
        if (accept) {
            lnprob[g] = lp;
            nacc[g] += 1;
        }
        if (chain) lnchain[(size_t)g * n_iter + it] = lp;
    }
}
#endif

// ---------------------------------------------------------------------------
// parallel tempering (psfmc_eval_theta_split, psfmc_pt_run; the contract is sampler.py's
// TemperedEnsembleSampler).  A walker carries its log-likelihood lnL, its log-prior lnpi and its tempered
// log-posterior lnp = beta lnL + lnpi -- exactly that product, then that sum.  A walker whose lnpi or lnL is
// not finite has lnL = lnp = -inf at every beta (no 0 * inf = NaN on the beta = 0 rung).
// ---------------------------------------------------------------------------
// the log-likelihood of walker w: walker_lnprob's sum without the prior, -inf if skipped or not finite
__device__ inline double walker_loglike(const double* __restrict__ partial, const uint8_t* __restrict__ skip,
                                        int nblk, int w, int lane, int nf, int fstride) {
    for (int f = 0; f < nf; ++f)
        if (skip[w + (size_t)f * fstride]) return -INFINITY;
    const double ll = walker_field_sum(partial, nblk, w, lane, nf, fstride);
    return ll == ll && fabs(ll) != INFINITY ? ll : -INFINITY;
}

__device__ inline double tempered_lnp(double beta, double ll, double lp) {
#pragma clang fp contract(off)
    const bool ok = ll == ll && fabs(ll) != INFINITY && lp == lp && fabs(lp) != INFINITY;
    const double bl = beta * ll;
    return ok ? bl + lp : -INFINITY;
}

#if PSFMC_PART == 0          /* not a template: defined in the API part only */
// log-likelihoods of W walkers whose partial sums are in `partial` (their log-priors stay where the record
// derivation wrote them); nf, fstride: see walker_field_sum.  One wave per walker (launch: finish_blocks(W) x
// kFinishThreads).
__global__ void k_split_finish(const double* __restrict__ partial, const uint8_t* __restrict__ skip, int nblk,
                               double* __restrict__ lnlike, int W, int nf, int fstride) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (kFinishThreads / 64) + (threadIdx.x >> 6);
    if (w >= W) return;
    const double ll = walker_loglike(partial, skip, nblk, w, lane, nf, fstride);
    if (lane == 0) lnlike[w] = ll;
}

// the start state of T W walkers (rung t = walkers [t W, (t + 1) W)): lnL made -inf where lnpi or lnL is not
// finite, lnp at each walker's beta.  One thread per walker.
__global__ void k_pt_tempered(const double* __restrict__ betas, double* __restrict__ lnL,
                              const double* __restrict__ lnpi, double* __restrict__ lnp, int TW, int W) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= TW) return;
    const double v = tempered_lnp(betas[i / W], lnL[i], lnpi[i]);
    if (v == -INFINITY) lnL[i] = -INFINITY;
    lnp[i] = v;
}

// accept / move of one tempered half-step: record r = t half + w is walker h half + w of rung t's ensemble,
// its proposal q[r] (formed by k_theta_prep with StretchIn::n_ens = T, by k_joint_propose, or by
// k_pt_move_propose); random numbers [n_iter][2][T][half].  Acceptance as k_stretch_finish's, ((P - 1) ln z + lnp_new) - lnp > ln u, with the
// tempered lnp.  A joint proposal is nf field records (fstride = T half apart, see walker_field_sum), lnprior[r]
// its joint log-prior.  No chain entry here: k_pt_swap writes the iteration's.  One wave per proposal (launch:
// finish_blocks(T half) x kFinishThreads).
// kJoint = false fixes nf = 1 when the kernel is compiled: the one-field tempered run launches this kernel twice
// per iteration, and with nf read at run time it measured 0.5 to 2.4 % slower per iteration
template <bool kJoint>
__global__ void k_pt_finish(const double* __restrict__ partial, const uint8_t* __restrict__ skip,
                            const double* __restrict__ lnprior, int nblk, const double* __restrict__ betas,
                            double* __restrict__ pos, double* __restrict__ lnL, double* __restrict__ lnpi,
                            double* __restrict__ lnp, const double* __restrict__ q, const double* __restrict__ lz,
                            const double* __restrict__ log_u, long long* __restrict__ nacc, int it, int T,
                            int half, int h, int P, int nf, int fstride) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (kFinishThreads / 64) + (threadIdx.x >> 6);
    if (r >= T * half) return;                               // wave-uniform
    const int t = r / half, w = r - t * half;
    const size_t off = ((size_t)it * 2 + h) * T * half + r;
    const double ll = walker_loglike(partial, skip, nblk, r, lane, kJoint ? nf : 1, kJoint ? fstride : 0);
    const double lp = lnprior[r];
    const double newlnp = tempered_lnp(betas[t], ll, lp);
    const size_t g = (size_t)t * 2 * half + (size_t)h * half + w;
    const double diff = (lz[off] + newlnp) - lnp[g];
    if (!(diff > log_u[off])) return;                        // the same in every lane
    for (int d = lane; d < P; d += 64) pos[g * P + d] = q[(size_t)r * P + d];
    if (lane == 0) {
        lnL[g] = newlnp == -INFINITY ? -INFINITY : ll;
        lnpi[g] = lp;
        lnp[g] = newlnp;
        nacc[g] += 1;
    }
}

// the swaps of one iteration, hottest pair first: for t = T-1 ... 1, pair k exchanges walker i[k] of rung t with
// walker j[k] of rung t-1 when ln u[k] < (beta_{t-1} - beta_t) (lnL[t, i[k]] - lnL[t-1, j[k]]) -- positions, lnL
// and lnpi; lnp is recomputed at each walker's new beta.  i and j are permutations, so the pairs of a rung are a
// matching: no two threads touch one walker.  Rungs run one after another (a barrier between them); the rung
// pair's accepted swaps are reduced in LDS and added to nswap[t-1] by one thread.  Then the iteration's chain
// entries: every rung's positions, lnL and lnpi (the host yields a resumable state per iteration), lnp of the
// beta = 1 rung.  ONE workgroup per ladder (launch: 1 x kPtSwapThreads; psfmc_pt_run_fields: F x kPtSwapThreads,
// workgroup f field f's ladder from its offsets into the same arrays, [F] leading every shape but the random
// numbers', which are [n_iter][F][T-1][W]).
// swap_i / swap_j / swap_log_u: [n_iter][T-1][W], entry t-1 the pair (t-1, t).
constexpr int kPtSwapThreads = 256;
__global__ void __launch_bounds__(kPtSwapThreads)
k_pt_swap(const double* __restrict__ betas, double* __restrict__ pos, double* __restrict__ lnL,
          double* __restrict__ lnpi, double* __restrict__ lnp, const int* __restrict__ swap_i,
          const int* __restrict__ swap_j, const double* __restrict__ swap_log_u, long long* __restrict__ nswap,
          double* __restrict__ chain, double* __restrict__ lnprob_chain, double* __restrict__ lnlike_chain,
          double* __restrict__ lnprior_chain, int it, int n_iter, int T, int W, int P) {
#pragma clang fp contract(off)
    __shared__ int count[kPtSwapThreads];
    const int tid = threadIdx.x;
    size_t row0 = (size_t)it * (T - 1);                      // the iteration's first row of the random numbers
    if (gridDim.x > 1) {                                     // several ladders: blockIdx.x's (workgroup-uniform)
        const size_t f = blockIdx.x;
        row0 = ((size_t)it * gridDim.x + f) * (T - 1);
        betas += f * T;
        pos += f * T * W * P;
        lnL += f * T * W;
        lnpi += f * T * W;
        lnp += f * T * W;
        nswap += f * (T - 1);
        if (chain) chain += f * T * W * n_iter * P;
        if (lnprob_chain) lnprob_chain += f * W * n_iter;
        if (lnlike_chain) lnlike_chain += f * T * W * n_iter;
        if (lnprior_chain) lnprior_chain += f * T * W * n_iter;
    }
    for (int t = T - 1; t >= 1; --t) {
        const size_t roff = (row0 + (t - 1)) * W;
        const double b_hot = betas[t], b_cold = betas[t - 1];
        const double dbeta = b_cold - b_hot;
        int mine = 0;
        for (int k = tid; k < W; k += kPtSwapThreads) {
            const size_t a = (size_t)t * W + swap_i[roff + k];
            const size_t b = (size_t)(t - 1) * W + swap_j[roff + k];
            const double dl = lnL[a] - lnL[b];
            const double lr = dbeta * dl;
            if (swap_log_u[roff + k] < lr) {
                for (int d = 0; d < P; ++d) {
                    const double x = pos[a * P + d];
                    pos[a * P + d] = pos[b * P + d];
                    pos[b * P + d] = x;
                }
                const double la = lnL[b], pa = lnpi[b], lb = lnL[a], pb = lnpi[a];
                lnL[a] = la;
                lnpi[a] = pa;
                lnp[a] = tempered_lnp(b_hot, la, pa);
                lnL[b] = lb;
                lnpi[b] = pb;
                lnp[b] = tempered_lnp(b_cold, lb, pb);
                ++mine;
            }
        }
        count[tid] = mine;
        __syncthreads();
        for (int s = kPtSwapThreads / 2; s > 0; s >>= 1) {
            if (tid < s) count[tid] += count[tid + s];
            __syncthreads();
        }
        if (tid == 0) nswap[t - 1] += count[0];
        __syncthreads();                                     // rung t-1 is final; count is free again
    }
    if (chain)
        for (int i = tid; i < T * W * P; i += kPtSwapThreads) {
            const int w = i / P, d = i - w * P;
            chain[((size_t)w * n_iter + it) * P + d] = pos[i];
        }
    if (lnprob_chain)
        for (int w = tid; w < W; w += kPtSwapThreads) lnprob_chain[(size_t)w * n_iter + it] = lnp[w];
    for (int i = tid; i < T * W; i += kPtSwapThreads) {
        if (lnlike_chain) lnlike_chain[(size_t)i * n_iter + it] = lnL[i];
        if (lnprior_chain) lnprior_chain[(size_t)i * n_iter + it] = lnpi[i];
    }
}
#endif

// ---------------------------------------------------------------------------
// joint fits (psfmc_eval_theta_joint, psfmc_stretch_run_joint, psfmc_pt_run_joint): the joint log-prior of a
// parameter vector, ONCE per walker -- every column's prior from the joint table J (J.n_sersic = 0: no slots),
// then the Sersic axis-ratio rule of every field from that field's own slots (fields[f]).  k_theta_prep then
// takes it as `extra`, with every field's own prior columns PRIOR_HOST, so that a walker outside the joint
// support is skipped in every field.
// ---------------------------------------------------------------------------
__device__ inline double joint_log_prior(const ThetaLayout& J, const ThetaLayout* fields, int n_fields,
                                         const double* th) {
    double lp = theta_log_prior(J, th, 0.0);
    for (int f = 0; f < n_fields; ++f) lp = theta_axis_ratio(fields[f], th, lp);
    return lp;
}

#if PSFMC_PART == 0          /* not a template: defined in the API part only */
// the joint log-priors of W given vectors theta [W][P].  One lane per walker (launch: ceil(W / 64) x 64).
__global__ void __launch_bounds__(64)
k_joint_prior(ThetaLayout J, const ThetaLayout* __restrict__ fields, int n_fields, const double* __restrict__ theta,
              double* __restrict__ lnprior, int W) {
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= W) return;
    lnprior[w] = joint_log_prior(J, fields, n_fields, theta + (size_t)w * J.n_params);
}

// the half-step stretch proposals of T ensembles of joint walkers (T = 1: psfmc_stretch_run_joint) and their
// joint log-priors: record r = t half + w is walker h half + w of rung t (rows [t 2 half, (t + 1) 2 half) of
// pos), its partner from the rung's other half; random numbers [n_iter][2][T][half] (StretchIn::n_ens).  The
// proposal is stretch_point's: the roundings of k_theta_prep's proposals.  One lane per record (launch:
// ceil(T half / 64) x 64).
__global__ void __launch_bounds__(64)
k_joint_propose(ThetaLayout J, const ThetaLayout* __restrict__ fields, int n_fields,
                const double* __restrict__ pos, double* __restrict__ q, const double* __restrict__ z,
                const int* __restrict__ partner, int it, int T, int half, int h, double* __restrict__ lnprior) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= T * half) return;
    const int P = J.n_params;
    const int t = r / half, w = r - t * half;
    const size_t off = ((size_t)it * 2 + h) * T * half + r;
    const size_t first = (size_t)t * 2 * half;               // rung t's first walker
    const double* s = pos + (first + (size_t)h * half + w) * P;
    const double* c = pos + (first + (size_t)(1 - h) * half + partner[off]) * P;
    const double zz = z[off];
    double* qr = q + (size_t)r * P;
    for (int d = 0; d < P; ++d) qr[d] = stretch_point(s[d], c[d], zz);
    lnprior[r] = joint_log_prior(J, fields, n_fields, qr);
}
#endif

#if PSFMC_PART == 0          /* not a template: defined in the API part only */
__global__ void k_stretch_next(int* __restrict__ d_iter) { *d_iter += 1; }
#endif

// ---------------------------------------------------------------------------
// proposal moves (psfmc_move_run, psfmc_stretch_set_moves, psfmc_move_run_joint; the contract is sampler.py's
// EnsembleSampler(moves=...)).  kind[it] names the move of BOTH half-steps of iteration it:
//   MOVE_STRETCH  q_i = c[a_i] - z_i (c[a_i] - s_i)          (stretch_point; scal = z, b unread)
//   MOVE_DE       q_i = s_i + g_i (c[a_i] - c[b_i])          (differential evolution; scal = g, a_i != b_i)
// s = half h of pos, c = the other half.  The DE proposal is three roundings -- the difference, the product,
// the sum -- as the numpy expression of the host contract; no FMA contraction.
// ---------------------------------------------------------------------------
constexpr int MOVE_STRETCH = 0, MOVE_DE = 1;
constexpr int kMoveThreads = 256;

__device__ inline double de_point(double s, double ca, double cb, double g) {
#pragma clang fp contract(off)
    const double diff = ca - cb;
    const double step = g * diff;
    return s + step;
}

#if PSFMC_PART == 0          /* not a template: defined in the API part only */
// The proposals q [half][P] of half h at iteration `it`: one thread per (walker, parameter) element, grid-stride
// over half P elements (launch: ceil(half P / kMoveThreads) x kMoveThreads).  a, b, scal: [n_iter][2][half].
__global__ void __launch_bounds__(kMoveThreads)
k_move_propose(const double* __restrict__ pos, double* __restrict__ q, const int* __restrict__ kind,
               const int* __restrict__ a, const int* __restrict__ b, const double* __restrict__ scal,
               int it, int half, int h, int P) {
    const int n = half * P;
    const size_t off = ((size_t)it * 2 + h) * half;
    const int move = kind[it];                                   // the same in every thread
    const double* s = pos + (size_t)h * half * P;
    const double* c = pos + (size_t)(1 - h) * half * P;
    for (int i = blockIdx.x * kMoveThreads + threadIdx.x; i < n; i += gridDim.x * kMoveThreads) {
        const int w = i / P, d = i - w * P;
        const double ca = c[(size_t)a[off + w] * P + d];
        const double g = scal[off + w];
        q[i] = move == MOVE_DE ? de_point(s[i], ca, c[(size_t)b[off + w] * P + d], g) : stretch_point(s[i], ca, g);
    }
}
#endif

// ---------------------------------------------------------------------------
// every field of a set tempered together (psfmc_pt_run_fields): E = F T ensembles of 2 half walkers, ensemble
// e = f T + t rung t of field f's ladder, rows [e 2 half, (e + 1) 2 half) of pos.
// ---------------------------------------------------------------------------
#if PSFMC_PART == 0          /* not a template: defined in the API part only */
// The half-step stretch proposals q [E half][P] of half h at iteration `it`: record r = e half + w is walker
// h half + w of ensemble e, its partner from the ensemble's other half; z and partner [n_iter][2][E][half].  One
// thread per (record, parameter) element, grid-stride over E half P elements (launch: ceil(E half P /
// kMoveThreads) x kMoveThreads).  Each element is stretch_point's: the roundings of k_theta_prep's proposals.
__global__ void __launch_bounds__(kMoveThreads)
k_pt_fields_propose(const double* __restrict__ pos, double* __restrict__ q, const double* __restrict__ z,
                    const int* __restrict__ partner, int it, int E, int half, int h, int P) {
    const size_t n = (size_t)E * half * P;
    const size_t off = ((size_t)it * 2 + h) * E * half;
    for (size_t i = (size_t)blockIdx.x * kMoveThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kMoveThreads) {
        const size_t r = i / P;
        const int d = (int)(i - r * P);
        const size_t e = r / half;
        const int w = (int)(r - e * half);
        const size_t first = e * 2 * half;                       // the ensemble's first walker
        const double s = pos[(first + (size_t)h * half + w) * P + d];
        const double c = pos[(first + (size_t)(1 - h) * half + partner[off + r]) * P + d];
        q[i] = stretch_point(s, c, z[off + r]);
    }
}

// k_pt_fields_propose by kind (psfmc_pt_move_run, psfmc_pt_move_run_joint, psfmc_pt_move_run_fields; the contract
// is sampler.py's TemperedEnsembleSampler.set_moves): ensemble e = l T + t is rung t of ladder l, and kind
// [n_iter][L] names the move of BOTH half-steps of every rung of ladder l at iteration it.  scal, a and b
// [n_iter][2][E][half]: z or g, the first partner, the DE moves' second partner (unread for a stretch element).
// The kind is uniform within a ladder, not within a workgroup: a per-element select.  A stretch element is
// stretch_point's, a DE element de_point's three roundings.  One thread per (record, parameter) element,
// grid-stride over E half P elements (launch: ceil(E half P / kMoveThreads) x kMoveThreads).
__global__ void __launch_bounds__(kMoveThreads)
k_pt_move_propose(const double* __restrict__ pos, double* __restrict__ q, const int* __restrict__ kind,
                  const int* __restrict__ a, const int* __restrict__ b, const double* __restrict__ scal,
                  int it, int E, int T, int half, int h, int P) {
    const size_t n = (size_t)E * half * P;
    const size_t off = ((size_t)it * 2 + h) * E * half;
    const int* kind_it = kind + (size_t)it * (E / T);
    for (size_t i = (size_t)blockIdx.x * kMoveThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kMoveThreads) {
        const size_t r = i / P;
        const int d = (int)(i - r * P);
        const size_t e = r / half;
        const int w = (int)(r - e * half);
        const size_t first = e * 2 * half;                       // the ensemble's first walker
        const double* c = pos + (first + (size_t)(1 - h) * half) * P + d;    // the other half, column d
        const double s = pos[(first + (size_t)h * half + w) * P + d];
        const double ca = c[(size_t)a[off + r] * P];
        const double g = scal[off + r];
        q[i] = kind_it[e / T] == MOVE_DE ? de_point(s, ca, c[(size_t)b[off + r] * P], g) : stretch_point(s, ca, g);
    }
}

// the beta = 1 rungs of F ladders, W walkers each, gathered for the posterior-image sums: out [F][W][P] from
// pos [F][T][W][P].  One thread per element, grid-stride (launch: ceil(F W P / kMoveThreads) x kMoveThreads).
__global__ void __launch_bounds__(kMoveThreads)
k_pt_gather_cold(const double* __restrict__ pos, double* __restrict__ out, int F, int T, int W, int P) {
    const size_t per = (size_t)W * P, n = (size_t)F * per;
    for (size_t i = (size_t)blockIdx.x * kMoveThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kMoveThreads) {
        const size_t f = i / per;
        out[i] = pos[f * T * per + (i - f * per)];
    }
}
#endif

}  // namespace psfmc
