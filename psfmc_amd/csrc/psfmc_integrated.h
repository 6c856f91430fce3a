// psfmc_integrated.h -- the PIXEL-INTEGRATED Sersic profile (`Sersic(..., integrate=True)`), not the reference's.
//
// Definition: psfmc_amd/ModelComponents/Sersic.py `Sersic.integrated_image` (numpy); these kernels are held to it.
// Per walker they write the SUM of its integrated components' images, img[w][ny][nx] doubles at MODEL coordinates
// (the image's own pixels; of an embedded image the top-left ly x lx corner of the transform-shaped slot).  The
// rasterising kernels (k_rows_fwd, k_rows3_fwd, k_raster_sums, k_raster) add that image to what they rasterise
// themselves; for them an integrated component's block of the prep record is replaced by a NEUTRAL one -- surface
// brightness exactly zero, centre off every pixel, so that it adds +0 to every pixel and no NaN -- and their code,
// the record layout and the component count stay what they are for a model without the keyword (the fields of one
// context may differ in which components are integrated).  The component's real block moves to ipar[w][k][9].
//
//   k_integ_split   per (walker, component): move a flagged block to ipar, leave the neutral block
//   k_integ_rows    part 1 of the definition: a wave per image row, every pixel outside the components' boxes
//   k_integ_core    parts 2 and 3: a wave per walker; the box pixel by pixel, a sample per lane, summed in the wave;
//                   the refinement with the 64 lanes = 4 cells x 16 sub-cells of a level, 16 samples each
// The work per walker and component is fixed (the box is clipped to the image, nothing else depends on the
// parameters), the summation order is fixed, there are no atomics: a walker's bits do not depend on its batch.
#pragma once
#include "psfmc_device.h"

namespace psfmc {

// the constants of Sersic.py (INTEG_*)
constexpr int kIntegHalfBox = 3, kIntegGridNear = 8, kIntegNearRing = 1, kIntegGridFar = 4;
constexpr int kIntegSplit = 4, kIntegLevels = 8, kIntegSub = 4;
static_assert(kIntegSplit == 4 && kIntegSub == 4, "k_integ_core maps 4 cells x 16 sub-cells to the lanes of a wave");
static_assert(kIntegGridNear * kIntegGridNear <= 64, "one sample of a box pixel per lane");
constexpr double kIntegMaxCentre = 1073741824.0;        // |centre + 1/2| beyond 2^30: no box, no refinement

// what the plain rasterisers see in place of an integrated component: 0 * finite at every pixel
__device__ inline void integ_neutral_block(double* __restrict__ b) {
    b[0] = -0.5; b[1] = -0.5; b[2] = 1.0; b[3] = 0.0; b[4] = 0.0; b[5] = 1.0; b[6] = 1.0; b[7] = 0.5; b[8] = 0.0;
}

// field of a (not skipped) walker's record, clamped
__device__ __forceinline__ int integ_psf_index(const double* __restrict__ wprep, int n_psf) {
    const int idx = __builtin_amdgcn_readfirstlane((int)wprep[kPrepPsfIdx]);
    return idx < 0 ? 0 : (idx >= n_psf ? n_psf - 1 : idx);
}

__global__ void k_integ_split(double* __restrict__ prep, int plen, const uint8_t* __restrict__ skip,
                              double* __restrict__ ipar, const uint8_t* __restrict__ flags, int n_ps, int n_sersic,
                              int n_psf, int n_psf_field, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * n_sersic) return;
    const int w = i / n_sersic, k = i - w * n_sersic;
    if (skip && skip[w]) return;
    double* rec = prep + (size_t)w * plen;
    int idx = (int)rec[kPrepPsfIdx];
    idx = idx < 0 ? 0 : (idx >= n_psf ? n_psf - 1 : idx);
    if (!flags[(idx / n_psf_field) * n_sersic + k]) return;
    double* b = rec + kPrepHead + kPrepPs * n_ps + kPrepSersic * k;
    double* o = ipar + (size_t)i * kPrepSersic;
    for (int j = 0; j < kPrepSersic; ++j) o[j] = b[j];
    integ_neutral_block(b);
}

// Sigma_e exp(-kappa (rho^(1/n) - 1)); at rho = 0 its finite peak.  log2 / exp2 through the rasteriser's own forms.
struct IntegEval { double f, u, v, q, t; };
__device__ __forceinline__ IntegEval integ_eval(const SersicPar& s, double nkl, double x, double y) {
    IntegEval e;
    const double dx = x - s.x0, dy = y - s.y0;
    e.u = __builtin_fma(s.m00, dx, s.m01 * dy);
    e.v = __builtin_fma(s.m10, dx, s.m11 * dy);
    e.q = __builtin_fma(e.u, e.u, e.v * e.v);
    e.t = e.q > 0.0 ? fast_exp2(s.p * fast_log2(e.q)) : 0.0;
    const double f = s.sbeff * fast_exp2_floor(__builtin_fma(nkl, e.t, -nkl));
    e.f = e.q == e.q ? f : e.q;                       // (the clamps of the exponentials swallow a NaN)
    return e;
}
__device__ __forceinline__ double integ_plain(const SersicPar& s, double nkl, double x, double y) {
    return integ_eval(s, nkl, x, y).f;
}

constexpr double kIntegLog2e = 1.44269504088896340736;

// part 1: f (1 + lap f / (24 f)) at the pixel centres outside every integrated component's own box (which
// k_integ_core fills); grid (ceil(ny / 4), n), 4 waves = 4 rows per workgroup
__global__ void __launch_bounds__(256)
k_integ_rows(const double* __restrict__ prep, int plen, const uint8_t* __restrict__ skip,
             const double* __restrict__ ipar, const uint8_t* __restrict__ flags, int n_sersic, int n_psf,
             int n_psf_field, const WrapDesc* __restrict__ wrap_tab, int ny, int nx, double* __restrict__ img) {
    const int w = blockIdx.y;
    if (skip && skip[w]) return;
    const int lane = threadIdx.x & 63;
    const int iy = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int idx = integ_psf_index(prep + (size_t)w * plen, n_psf);
    const int ly = wrap_tab ? wrap_tab[idx].ly : ny, lx = wrap_tab ? wrap_tab[idx].lx : nx;
    if (iy >= ly || iy >= ny) return;
    const uint8_t* fl = flags + (idx / n_psf_field) * n_sersic;
    double* out = img + ((size_t)w * ny + iy) * nx;
    const double y = (double)iy;
    for (int x0 = 0; x0 < lx && x0 < nx; x0 += 64) {
        const int ix = x0 + lane;
        double acc = 0.0;
        for (int k = 0; k < n_sersic; ++k) {
            if (!fl[k]) continue;                                      // wave-uniform
            const SersicPar s = load_sersic(ipar + ((size_t)w * n_sersic + k) * kPrepSersic);
            const int px = (int)floor(s.x0 + 0.5), py = (int)floor(s.y0 + 0.5);
            const bool boxed = fabs(s.x0 + 0.5) <= kIntegMaxCentre && fabs(s.y0 + 0.5) <= kIntegMaxCentre &&
                               abs(ix - px) <= kIntegHalfBox && abs(iy - py) <= kIntegHalfBox;
            const double nkl = -s.kappa * kIntegLog2e;
            const IntegEval e = integ_eval(s, nkl, (double)ix, y);
            const double ie2 = __builtin_fma(s.m00, s.m00, s.m01 * s.m01);      // 1 / r_e^2
            const double ib2 = __builtin_fma(s.m10, s.m10, s.m11 * s.m11);      // 1 / r_b^2
            const double rq = fast_rcp(e.q);
            const double tt = s.kappa * s.p * e.t * rq;
            const double lap = (tt * tt - tt * (s.p - 1.0) * rq) * 4.0 * (e.u * e.u * ie2 + e.v * e.v * ib2) -
                               2.0 * tt * (ie2 + ib2);
            acc += boxed ? 0.0 : e.f * (1.0 + lap * (1.0 / 24.0));
        }
        if (ix < lx && ix < nx) out[ix] = acc;
    }
}

__device__ __forceinline__ double integ_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// parts 2 and 3; grid (n), one wave per walker, its integrated components one after the other
__global__ void __launch_bounds__(64)
k_integ_core(const double* __restrict__ prep, int plen, const uint8_t* __restrict__ skip,
             const double* __restrict__ ipar, const uint8_t* __restrict__ flags, int n_sersic, int n_psf,
             int n_psf_field, const WrapDesc* __restrict__ wrap_tab, int ny, int nx, double* __restrict__ img) {
    const int w = blockIdx.x;
    if (skip && skip[w]) return;
    const int lane = threadIdx.x;
    const int idx = integ_psf_index(prep + (size_t)w * plen, n_psf);
    int ly = wrap_tab ? wrap_tab[idx].ly : ny, lx = wrap_tab ? wrap_tab[idx].lx : nx;
    ly = ly < ny ? ly : ny;
    lx = lx < nx ? lx : nx;
    const uint8_t* fl = flags + (idx / n_psf_field) * n_sersic;
    double* out = img + (size_t)w * ny * nx;
    for (int k = 0; k < n_sersic; ++k) {
        if (!fl[k]) continue;                                          // wave-uniform
        const SersicPar s = load_sersic(ipar + ((size_t)w * n_sersic + k) * kPrepSersic);
        const double nkl = -s.kappa * kIntegLog2e;
        const double gx = s.x0 + 0.5, gy = s.y0 + 0.5;
        if (!(fabs(gx) <= kIntegMaxCentre && fabs(gy) <= kIntegMaxCentre)) continue;   // (NaN too)
        const double fx = floor(gx), fy = floor(gy);
        const int px = (int)fx, py = (int)fy;
        const bool ex = gx == fx, ey = gy == fy;                       // the centre is on a pixel edge
        // part 2: the box, pixel by pixel; lane = sample (b, a) of the s x s midpoint grid
        for (int j = -kIntegHalfBox; j <= kIntegHalfBox; ++j) {
            const int Y = py + j;
            if (Y < 0 || Y >= ly) continue;
            for (int i = -kIntegHalfBox; i <= kIntegHalfBox; ++i) {
                const int X = px + i;
                if (X < 0 || X >= lx) continue;
                if ((i == 0 || (i == -1 && ex)) && (j == 0 || (j == -1 && ey))) continue;     // part 3
                const int d = max(abs(i), abs(j));
                const int g = d <= kIntegNearRing ? kIntegGridNear : kIntegGridFar;
                const int a = lane % g, b = lane / g;
                const double sx = (double)X + (((double)a + 0.5) / (double)g - 0.5);
                const double sy = (double)Y + (((double)b + 0.5) / (double)g - 0.5);
                const double v = lane < g * g ? integ_plain(s, nkl, sx, sy) : 0.0;
                const double mean = integ_wave_sum(v) / (double)(g * g);
                if (lane == 0) out[(size_t)Y * nx + X] += mean;
            }
        }
        // part 3: level l, pitch h = 4^-l: lane = (cell slot, sub-cell); slot (pdx, pdy) is cell floor(g h^-1) - 1 + pd
        const int slot = lane >> 4, sub = lane & 15;
        const int pdx = slot & 1, pdy = slot >> 1, sa = sub & 3, sb = sub >> 2;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};                          // the pixels (px - 1 + dx, py - 1 + dy)
        double scale = 1.0;
        for (int l = 0; l <= kIntegLevels; ++l, scale *= (double)kIntegSplit) {
            const double hx = gx * scale, hy = gy * scale;
            const double ax = floor(hx), ay = floor(hy);
            const double cx = ax - 1.0 + (double)pdx, cy = ay - 1.0 + (double)pdy;       // this lane's cell
            const bool cell_on = (pdx == 1 || hx == ax) && (pdy == 1 || hy == ay);       // it holds the centre
            const double ix = cx * 4.0 + (double)sa, iy = cy * 4.0 + (double)sb;         // its sub-cell
            const double nhx = hx * 4.0, nhy = hy * 4.0;
            const double nax = floor(nhx), nay = floor(nhy);
            const bool deferred = l < kIntegLevels && (ix == nax || (nhx == nax && ix == nax - 1.0)) &&
                                  (iy == nay || (nhy == nay && iy == nay - 1.0));         // a cell of level l + 1
            const double cw = 1.0 / (scale * 4.0);
            const double bx = ix * cw - 0.5, by = iy * cw - 0.5;
            double sum = 0.0;
#pragma unroll 1
            for (int sy = 0; sy < kIntegSub; ++sy)
#pragma unroll
                for (int sx = 0; sx < kIntegSub; ++sx)
                    sum += integ_plain(s, nkl, bx + (((double)sx + 0.5) / (double)kIntegSub) * cw,
                                       by + (((double)sy + 0.5) / (double)kIntegSub) * cw);
            const double part = (cell_on && !deferred) ? sum * (cw * cw * (1.0 / (kIntegSub * kIntegSub))) : 0.0;
            const int dx = (int)(floor(cx / scale) - fx) + 1, dy = (int)(floor(cy / scale) - fy) + 1;   // its pixel
            const int pix = (dy & 1) * 2 + (dx & 1);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += pix == q ? part : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double total = integ_wave_sum(acc[q]);
            const int X = px - 1 + (q & 1), Y = py - 1 + (q >> 1);
            const bool held = ((q & 1) == 1 || ex) && ((q >> 1) == 1 || ey);
            if (lane == 0 && held && X >= 0 && X < lx && Y >= 0 && Y < ly) out[(size_t)Y * nx + X] += total;
        }
    }
}

}  // namespace psfmc
