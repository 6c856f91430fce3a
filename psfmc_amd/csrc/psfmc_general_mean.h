// psfmc_general_mean.h -- general components rendered as the MEAN OF THEIR LAW OVER EACH PIXEL
// (`Sersic(..., boxiness / fourier / spiral, pixel_mean=True)`, `Moffat(..., pixel_mean=True)`,
// `Ferrer(..., pixel_mean=True)`).  Not the reference's.
//
// Definition: psfmc_amd/ModelComponents/Sersic.py `Sersic.general_point` and `Sersic.general_mean_image` (numpy);
// these kernels are held to them.  The mode adds no per-walker entries: a per (field, Sersic) flag byte
// (psfmc_set_general_mean) says which general components it renders.  k_general_split and k_fourier_prep see such a
// component as any general one (gpar, fpar, spar, rpar are formed as always); k_general_rows gets a flag array with
// the component cleared, so it leaves it out, and the two kernels below ADD it to the walkers' extra images behind it:
//
//   k_general_mean_rows   parts 1 and 2 of the definition: a wave per image row over the field's own ly x lx pixels,
//                         every pixel outside the components' boxes: (2 g(centre) + mean of g at the corners) / 3; a
//                         lane evaluates its pixel's centre and its two LEFT corners and takes the right ones from the
//                         next lane -- three evaluations per pixel, not five.  A chunk is 63 pixels: lane 63 owns none
//                         and holds the right corners of the 63rd (that lane evaluating two more points on its own
//                         would cost the whole wave two more passes).  Ferrer: the pixels the truncation edge crosses are
//                         found by a ballot and sampled one after the other by the whole wave, 64 lanes = the 8 x 8
//                         midpoint grid
//   k_general_mean_core   parts 3 and 4: k_integ_core with g in place of the plain profile -- a wave per walker; the
//                         box pixel by pixel, a sample per lane; the refinement cell by cell (one cell per level
//                         unless the centre is on a pixel edge), the 64 lanes = 16 sub-cells x 4 sample rows
// g is `general_point`: the law without a centroid term, its finite peak at u = v = 0.  It repeats general_pixel's
// coordinate code and its fast_log2 / fast_exp2 forms, with modes, spiral and kind as WAVE-UNIFORM RUNTIME BRANCHES:
// one instantiation serves every context without truncations, and the instantiations of psfmc_general.h are the text
// they were.  TRU: a context with truncations runs the second instantiation of the two kernels, whose g is
// `general_point * inner * outer` (the sides a wave-uniform runtime branch): every scheme below averages the product.
// The TRU = false instantiations are the kernels as they were, with their registers and occupancy.  BND: a context with
// bending modes runs a third instantiation (TRU and BND set), whose g bends v ahead of |u|^e + |v|^e (the modes a
// wave-uniform runtime branch); the BND = false instantiations are the kernels as they were.
// The work per walker and component is fixed but for the Ferrer edge pixels, which depend on that walker's parameters
// alone; every pixel is written by one lane in one fixed summation order (the xor butterfly of integ_wave_sum), there
// are no atomics and no exchange through LDS: a walker's bits do not depend on its batch.
#pragma once
#include "psfmc_general.h"

namespace psfmc {

constexpr int kMeanEdgeGrid = 8;     // Sersic.py MEAN_EDGE_GRID
constexpr int kMeanChunk = 63;       // pixels of a row per pass of k_general_mean_rows: the 64th lane holds their last corners
static_assert(kMeanEdgeGrid * kMeanEdgeGrid == 64, "the 64 lanes of a wave are the samples of a Ferrer edge pixel");

// a component's constants as the kernels of psfmc_general.h left them; F.top == 0: no modes; kind 0: the Sersic law;
// T.sides == 0: not truncated; B.top == 0: not bent
struct MeanPar { GenPar G; FouPar F; SpiPar S; RadPar R; TruPar T; BndPar B; bool wound; int kind; };
__device__ __forceinline__ MeanPar load_mean(const double* __restrict__ gpar, const double* __restrict__ fpar,
                                             const uint8_t* __restrict__ fmasks, const double* __restrict__ spar,
                                             const uint8_t* __restrict__ smasks, const double* __restrict__ rpar,
                                             const uint8_t* __restrict__ rkinds, const double* __restrict__ tpar,
                                             const uint8_t* __restrict__ tmasks, int w, int k, int field,
                                             int n_sersic, const double* __restrict__ bpar = nullptr,
                                             const uint8_t* __restrict__ bmasks = nullptr) {
    MeanPar M{};
    const size_t i = (size_t)w * n_sersic + k;
    M.G = load_general(gpar + i * kGenPar);
    const int modes = fmasks ? fmasks[field * n_sersic + k] & kFouModeBits : 0;             // wave-uniform
    if (modes) {
        const double* f = fpar + i * kFouPar;
#pragma unroll
        for (int m = 0; m < kFouModes; ++m) {
            M.F.a[m] = f[2 * m];
            M.F.b[m] = f[2 * m + 1];
        }
        M.F.top = 32 - __builtin_clz((unsigned)modes);                                      // the highest mode present
    }
    M.wound = smasks ? (smasks[field * n_sersic + k] & kSpiFlag) != 0 : false;              // wave-uniform
    if (M.wound) M.S = load_spiral(spar + i * kSpiPar);
    M.kind = rkinds ? rkinds[field * n_sersic + k] : 0;                                     // wave-uniform
    if (M.kind) M.R = load_radial(rpar + i * kRadPar);
    const int sides = tmasks ? tmasks[field * n_sersic + k] : 0;                            // wave-uniform (TRU only)
    if (sides) M.T = load_trunc(tpar + i * kTruPar, sides);
    const int bends = bmasks ? bmasks[field * n_sersic + k] & kBndModeBits : 0;             // wave-uniform (BND only)
    if (bends) M.B = load_bend(bpar + i * kBndPar, bends);
    return M;
}

// g at the point (x, y); *inside: Ferrer's x < 1 (true at u = v = 0), true for the other laws
template <bool TRU = false, bool BND = false>
__device__ __forceinline__ double general_point(const MeanPar& M, double x, double y, bool* inside) {
    const GenPar& G = M.G;
    const double dx = x - G.s.x0, dy = y - G.s.y0;
    double u, v;
    if (M.wound) {                                                     // wave-uniform
        const SpiPar& S = M.S;
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
    } else {
        u = __builtin_fma(G.s.m00, dx, G.s.m01 * dy);
        v = __builtin_fma(G.s.m10, dx, G.s.m11 * dy);
    }
    if constexpr (BND) {
        if (M.B.top > 0) v = bend_apply(M.B, u, v);                    // wave-uniform
    }
    const double au = fabs(u), av = fabs(v);
    // |u| = 0 gives the term exactly 0 (not log2(0) e)
    const double pu = au > 0.0 ? fast_exp2(G.e * fast_log2(au)) : 0.0;
    const double pv = av > 0.0 ? fast_exp2(G.e * fast_log2(av)) : 0.0;
    const double s = pu + pv;
    double l1e = 0.0;                                                  // log2(1 + eps)
    if (M.F.top > 0) {                                                 // wave-uniform
        const double rinv = general_rsqrt(__builtin_fma(u, u, v * v));
        l1e = fast_log2(1.0 + fourier_eps(M.F, u * rinv, v * rinv));
    }
    const double ls = fast_log2(s);
    double val, chk;
    bool in = true;
    if (M.kind == 0) {                                                 // wave-uniform
        // the peak sb e^kappa at s = 0 comes from t = 0 (a NaN of l1e there is never read)
        const double t = s > 0.0 ? fast_exp2(__builtin_fma(G.pe2, ls, (G.s.p + G.s.p) * l1e)) : 0.0;
        val = G.s.sbeff * fast_exp2_floor(__builtin_fma(G.nkl, t, -G.nkl));
        chk = (u + v) + (G.nkl + G.pe2);               // (the comparisons and the exponentials' clamps swallow a NaN)
    } else {
        const RadPar& R = M.R;
        if (M.kind == kRadMoffat) {
            const double rho2 = fast_exp2(__builtin_fma(G.pe2 + G.pe2, ls, l1e + l1e));      // (p = 1/2: pe2 = 1/e)
            val = G.s.sbeff * fast_exp2(R.b * fast_log2(__builtin_fma(R.a, rho2, 1.0)));
        } else {
            const double xk = fast_exp2(__builtin_fma(R.a, ls, R.b * l1e));
            in = s > 0.0 ? xk < 1.0 : true;
            val = xk < 1.0 ? G.s.sbeff * fast_exp2(R.c * fast_log2(1.0 - xk)) : 0.0;
        }
        val = s > 0.0 ? val : G.s.sbeff;                               // the centre: Sigma_0, finite
        chk = (u + v) + (G.s.sbeff + R.chk);
    }
    if (M.wound) chk += M.S.chk;
    if constexpr (TRU) {
        if (M.T.sides) {                                               // wave-uniform: g times the truncation's factors
            val = trunc_apply(M.T, val, s > 0.0 ? fast_exp2(__builtin_fma(M.T.ie, ls, l1e)) : 0.0);
            chk += M.T.chk;
        }
    }
    *inside = in;
    return chk == chk ? val : chk;
}

// the box of parts 3 and 4 around a component's centre: none where the centre is not finite or beyond 2^30
struct MeanBox { bool any; int px, py; };
__device__ __forceinline__ MeanBox mean_box(const SersicPar& s) {
    const double gx = s.x0 + 0.5, gy = s.y0 + 0.5;
    MeanBox b;
    b.any = fabs(gx) <= kIntegMaxCentre && fabs(gy) <= kIntegMaxCentre;                      // (false for a NaN)
    b.px = b.any ? (int)floor(gx) : 0;
    b.py = b.any ? (int)floor(gy) : 0;
    return b;
}

// parts 1 and 2; grid (ceil(ny / 4), n), 4 waves = 4 rows per workgroup.  Behind k_general_rows, which wrote or added
// to every pixel of the row: this kernel ADDS.  mflags [n_fields][n_sersic]; fpar / fmasks, spar / smasks, rpar / rkinds
// are nullptr in a context without modes, spirals or laws, tpar / tmasks in one without truncations, bpar / bmasks in
// one without bending modes.
template <bool TRU = false, bool BND = false>
__global__ void __launch_bounds__(256)
k_general_mean_rows(const double* __restrict__ prep, int plen, const uint8_t* __restrict__ skip,
                    const double* __restrict__ gpar, const uint8_t* __restrict__ mflags, int n_sersic, int n_psf,
                    int n_psf_field, const WrapDesc* __restrict__ wrap_tab, int ny, int nx, double* __restrict__ img,
                    const double* __restrict__ fpar, const uint8_t* __restrict__ fmasks,
                    const double* __restrict__ spar, const uint8_t* __restrict__ smasks,
                    const double* __restrict__ rpar, const uint8_t* __restrict__ rkinds,
                    const double* __restrict__ tpar = nullptr, const uint8_t* __restrict__ tmasks = nullptr,
                    const double* __restrict__ bpar = nullptr, const uint8_t* __restrict__ bmasks = nullptr) {
    const int w = blockIdx.y;
    if (skip && skip[w]) return;
    const int lane = threadIdx.x & 63;
    const int iy = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int idx = integ_psf_index(prep + (size_t)w * plen, n_psf);
    const int ly = wrap_tab ? wrap_tab[idx].ly : ny, lx = wrap_tab ? wrap_tab[idx].lx : nx;
    if (iy >= ly || iy >= ny) return;                                  // wave-uniform
    const int field = idx / n_psf_field;
    const uint8_t* fl = mflags + field * n_sersic;
    double* out = img + ((size_t)w * ny + iy) * nx;
    const double y = (double)iy;
    const int xn = lx < nx ? lx : nx;
    for (int k = 0; k < n_sersic; ++k) {
        if (!fl[k]) continue;                                          // wave-uniform
        const MeanPar M = load_mean(gpar, fpar, fmasks, spar, smasks, rpar, rkinds, tpar, tmasks, w, k, field,
                                      n_sersic, BND ? bpar : nullptr, BND ? bmasks : nullptr);
        const MeanBox box = mean_box(M.G.s);
        const bool row_boxed = box.any && abs(iy - box.py) <= kIntegHalfBox;
        // (every lane runs every chunk to its end, lane 63 and the ones beyond the row's last pixel included: they
        // hold the right corners of the pixel before them and take part in the shuffles)
        for (int x0 = 0; x0 < xn; x0 += kMeanChunk) {
            const int ix = x0 + lane;
            const double x = (double)ix;
            bool ic, itl, ibl, itr, ibr;
            const double c = general_point<TRU, BND>(M, x, y, &ic);
            const double tl = general_point<TRU, BND>(M, x - 0.5, y - 0.5, &itl);
            const double bl = general_point<TRU, BND>(M, x - 0.5, y + 0.5, &ibl);
            const double tr = __shfl_down(tl, 1, 64), br = __shfl_down(bl, 1, 64);
            itr = __shfl_down((int)itl, 1, 64) != 0;
            ibr = __shfl_down((int)ibl, 1, 64) != 0;
            const bool live = lane < kMeanChunk && ix < xn;
            const bool boxed = row_boxed && abs(ix - box.px) <= kIntegHalfBox;
            double val = (2.0 * c + 0.25 * ((tl + tr) + (bl + br))) / 3.0;
            if (M.kind == kRadFerrer) {                                // wave-uniform
                const int n_in = (int)ic + (int)itl + (int)itr + (int)ibl + (int)ibr;
                unsigned long long edge = __ballot(live && !boxed && n_in > 0 && n_in < 5);
                const int a = lane % kMeanEdgeGrid, b = lane / kMeanEdgeGrid;
                const double ox = ((double)a + 0.5) / (double)kMeanEdgeGrid - 0.5;
                const double oy = ((double)b + 0.5) / (double)kMeanEdgeGrid - 0.5;
                while (edge) {                                         // wave-uniform: one edge pixel per turn
                    const int bit = __ffsll((long long)edge) - 1;
                    edge &= edge - 1;
                    bool unused;
                    const double v = general_point<TRU, BND>(M, (double)(x0 + bit) + ox, y + oy, &unused);
                    const double mean = integ_wave_sum(v) / (double)(kMeanEdgeGrid * kMeanEdgeGrid);
                    if (lane == bit) val = mean;
                }
            }
            if (live) out[ix] += boxed ? 0.0 : val;
        }
    }
}

// parts 3 and 4; grid (n), one wave per walker, its mean components one after the other (k_integ_core with g)
template <bool TRU = false, bool BND = false>
__global__ void __launch_bounds__(64)
k_general_mean_core(const double* __restrict__ prep, int plen, const uint8_t* __restrict__ skip,
                    const double* __restrict__ gpar, const uint8_t* __restrict__ mflags, int n_sersic, int n_psf,
                    int n_psf_field, const WrapDesc* __restrict__ wrap_tab, int ny, int nx, double* __restrict__ img,
                    const double* __restrict__ fpar, const uint8_t* __restrict__ fmasks,
                    const double* __restrict__ spar, const uint8_t* __restrict__ smasks,
                    const double* __restrict__ rpar, const uint8_t* __restrict__ rkinds,
                    const double* __restrict__ tpar = nullptr, const uint8_t* __restrict__ tmasks = nullptr,
                    const double* __restrict__ bpar = nullptr, const uint8_t* __restrict__ bmasks = nullptr) {
    const int w = blockIdx.x;
    if (skip && skip[w]) return;
    const int lane = threadIdx.x;
    const int idx = integ_psf_index(prep + (size_t)w * plen, n_psf);
    int ly = wrap_tab ? wrap_tab[idx].ly : ny, lx = wrap_tab ? wrap_tab[idx].lx : nx;
    ly = ly < ny ? ly : ny;
    lx = lx < nx ? lx : nx;
    const int field = idx / n_psf_field;
    const uint8_t* fl = mflags + field * n_sersic;
    double* out = img + (size_t)w * ny * nx;
    bool unused;
    for (int k = 0; k < n_sersic; ++k) {
        if (!fl[k]) continue;                                          // wave-uniform
        const MeanPar M = load_mean(gpar, fpar, fmasks, spar, smasks, rpar, rkinds, tpar, tmasks, w, k, field,
                                      n_sersic, BND ? bpar : nullptr, BND ? bmasks : nullptr);
        const double gx = M.G.s.x0 + 0.5, gy = M.G.s.y0 + 0.5;
        if (!(fabs(gx) <= kIntegMaxCentre && fabs(gy) <= kIntegMaxCentre)) continue;   // (NaN too)
        const double fx = floor(gx), fy = floor(gy);
        const int px = (int)fx, py = (int)fy;
        const bool ex = gx == fx, ey = gy == fy;                       // the centre is on a pixel edge
        // part 3: the box, pixel by pixel; lane = sample (b, a) of the s x s midpoint grid
        for (int j = -kIntegHalfBox; j <= kIntegHalfBox; ++j) {
            const int Y = py + j;
            if (Y < 0 || Y >= ly) continue;
            for (int i = -kIntegHalfBox; i <= kIntegHalfBox; ++i) {
                const int X = px + i;
                if (X < 0 || X >= lx) continue;
                if ((i == 0 || (i == -1 && ex)) && (j == 0 || (j == -1 && ey))) continue;     // part 4
                const int d = max(abs(i), abs(j));
                const int g = d <= kIntegNearRing ? kIntegGridNear : kIntegGridFar;
                const int a = lane % g, b = lane / g;
                const double sx = (double)X + (((double)a + 0.5) / (double)g - 0.5);
                const double sy = (double)Y + (((double)b + 0.5) / (double)g - 0.5);
                const double pv = general_point<TRU, BND>(M, sx, sy, &unused);
                const double v = lane < g * g ? pv : 0.0;
                const double mean = integ_wave_sum(v) / (double)(g * g);
                if (lane == 0) out[(size_t)Y * nx + X] += mean;
            }
        }
        // part 4: level l, pitch h = 4^-l.  The (up to four) cells that hold the centre -- slot (pdx, pdy) is cell
        // floor(g h^-1) - 1 + pd; slot (1, 1) always, the others where the centre is on their edge -- are taken one
        // after the other (wave-uniform), lane = (sample row, sub-cell): 16 sub-cells x 4 rows of 4 samples each
        const int sub = lane & 15, srow = lane >> 4, sa = sub & 3, sb = sub >> 2;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};                          // the pixels (px - 1 + dx, py - 1 + dy)
        double scale = 1.0;
#pragma unroll 1
        for (int l = 0; l <= kIntegLevels; ++l, scale *= (double)kIntegSplit) {
            const double hx = gx * scale, hy = gy * scale;
            const double ax = floor(hx), ay = floor(hy);
            const double nhx = hx * 4.0, nhy = hy * 4.0;
            const double nax = floor(nhx), nay = floor(nhy);
            const double cw = 1.0 / (scale * 4.0);
#pragma unroll 1
            for (int slot = 0; slot < 4; ++slot) {
                const int pdx = slot & 1, pdy = slot >> 1;
                if (!((pdx == 1 || hx == ax) && (pdy == 1 || hy == ay))) continue;       // wave-uniform: not holding
                const double cx = ax - 1.0 + (double)pdx, cy = ay - 1.0 + (double)pdy;   // the cell
                const double ix = cx * 4.0 + (double)sa, iy = cy * 4.0 + (double)sb;     // this lane's sub-cell
                const bool deferred = l < kIntegLevels && (ix == nax || (nhx == nax && ix == nax - 1.0)) &&
                                      (iy == nay || (nhy == nay && iy == nay - 1.0));     // a cell of level l + 1
                const double bx = ix * cw - 0.5, by = iy * cw - 0.5;
                const double sy = by + (((double)srow + 0.5) / (double)kIntegSub) * cw;
                double sum = 0.0;
#pragma unroll 1
                for (int sx = 0; sx < kIntegSub; ++sx)
                    sum += general_point<TRU, BND>(M, bx + (((double)sx + 0.5) / (double)kIntegSub) * cw, sy, &unused);
                const double part = deferred ? 0.0 : sum * (cw * cw * (1.0 / (kIntegSub * kIntegSub)));
                const int dx = (int)(floor(cx / scale) - fx) + 1, dy = (int)(floor(cy / scale) - fy) + 1;   // its pixel
                const int pix = (dy & 1) * 2 + (dx & 1);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] += pix == q ? part : 0.0;
            }
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
