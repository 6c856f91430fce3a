// psfmc_fisher.h -- Fisher matrix and gradient of the log-likelihood from a central-difference stencil of images
// (psfmc_fisher_rows, include/psfmc_hip.h; the definition: psfmc_amd/mode.py fisher_from_stencil).
//
// A stencil of K differentiated columns is 2K + 1 walkers: the base, then theta +- h_k e_k.  With the base's
// r = sci - conv and w = 1 / (model_var + obs_var), per good pixel
//     a_k = sqrt(w) (conv[1+2k] - conv[2+2k]) inv2h_k          c = sqrt(w) r
//     b_k = (w / sqrt 2) (mvar[1+2k] - mvar[2+2k]) inv2h_k     d = (r^2 w - 1) / sqrt 2
//     F = sum_pix (a a^T + b b^T)       g_k = sum_pix (a_k c + b_k d)
// i.e. ONE Gram matrix of the K + 1 extended vectors (a; c) and (b; d): F is its leading K x K block, g its last column.
//
// Three kernels, none of which depends on the image side (part 0 of the split build holds the one copy):
//   k_fisher_stash   after each pass: the image windows of the pass's convolved models and model variances into the
//                    resident [walker][2][pixel] stash (a stencil's +- walkers may fall in different passes)
//   k_fisher_gram    one wave per 64 pixels and stencil: the pixels are the k-dimension of v_mfma_f64_16x16x4_f64, four
//                    per instruction, a 16 x 16 tile of the Gram matrix stays in 8 VGPRs; upper-triangle tiles only
//   k_fisher_finish  adds the waves' partial tiles in index order and mirrors the triangle: no atomics, so a stencil's
//                    F and g are the same bits wherever in a batch it stands
// Stencils of different fields in one call (psfmc_fisher_rows_fields, psfmc_fisher_rows_joint): a third source for the
// Gram kernel, FisherFieldStencils, takes each stencil's pixels, window, wave count and offsets from a device table
// (FisherFieldRec, psfmc_fisher_plan.h); k_fisher_stash_fields and k_fisher_finish_fields read the same table, and
// k_fisher_link adds the fields' matrices into a joint fit's.  A stencil's arithmetic is the one-field kernels' on its
// own record, so its bits are those of a psfmc_fisher_rows call on it alone.
// Fragment map of v_mfma_f64_16x16x4_f64 (one f64 per lane in, 4 per lane out): A[i][k] and B[k][j] on lane
// i + 16 k resp. j + 16 k; D[row][col] in register `row >> 2` of lane (row & 3) * 16 + col (fisher_tile_slot).
#pragma once

#include "psfmc_fisher_plan.h"

namespace psfmc {

using fisher_acc = __attribute__((ext_vector_type(4))) double;

// the image windows of n walkers' convolved model and model variance (walker w of the pass: image stride * w of
// `conv`, image stride * w + var_c of `mvar`, each S pixels of the transform's shape) -> stash[w][2][ly lx]
__global__ void __launch_bounds__(256)
k_fisher_stash(const double* __restrict__ conv, const double* __restrict__ mvar, double* __restrict__ stash, int S,
               int stride, int var_c, ImgWindow win) {
    const int w = blockIdx.y;
    const double* src_c = conv + (size_t)(stride * w) * S;
    const double* src_v = mvar + (size_t)(stride * w + var_c) * S;
    const int n_pix = win.ly * win.lx;
    double* dst = stash + (size_t)w * 2 * n_pix;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += gridDim.x * blockDim.x) {
        const int y = i / win.lx, x = i - y * win.lx;
        const int j = (y + win.ay) * win.nx + x + win.ax;
        dst[i] = src_c[j];
        dst[n_pix + i] = src_v[j];
    }
}

// what the Gram kernel forms its per-pixel vectors from
struct FisherStencil {           // a stash of stencils and the field's pixels (transform shape, window `win`)
    const double* stash;         // [n_base][2K+1][2][n_pix]
    const double* inv2h;         // [n_base][K]
    const double *sci, *obs_var;
    const uint8_t* bad;
    ImgWindow win;
};
struct FisherVectors {           // the vectors themselves (psfmc_debug_fisher_gram)
    const double *a, *b;         // [K][n_pix]
    const double *c, *d;         // [n_pix]
};
struct FisherFieldStencils {     // stencils of different fields (psfmc_fisher_rows_fields / _joint): all from the table
    const FisherFieldRec* recs;  // [n_stencils] (psfmc_fisher_plan.h)
    const double* stash;         // the stencils' images at recs[s].stash
    const double* inv2h;         // [n_stencils][K]
    const double *sci, *obs_var; // the context's pixel arrays: a field's at recs[s].px
    const uint8_t* bad;
};

// a stencil's pixels, waves and the place of its partial tiles: the launch's for the first two sources, the
// record's for the third
struct FisherGeom { int n_pix, units; size_t partial; };
template <class Src>
__device__ inline FisherGeom fisher_geom(const Src&, int base, int n_pix, int units, int n_tiles) {
    return FisherGeom{n_pix, units, (size_t)base * units * n_tiles * kFisherTileDoubles};
}
__device__ inline FisherGeom fisher_geom(const FisherFieldStencils& s, int base, int, int, int) {
    const FisherFieldRec& r = s.recs[base];
    return FisherGeom{r.n_pix, r.units, (size_t)r.partial};
}

// The (a; c) and (b; d) entries `e` = 16 t + (lane & 15), t < T, of pixel p (any valid pixel where !on: the entries
// are then zeros, which is how a slab's tail past n_pix is padded).
template <int T>
__device__ inline void fisher_entries(const FisherStencil& s, int base, int K, int n_pix, int p, bool on, int col,
                                      double* va, double* vb) {
    const int y = p / s.win.lx, x = p - y * s.win.lx;
    const int j = (y + s.win.ay) * s.win.nx + x + s.win.ax;
    const size_t img = (size_t)2 * n_pix;
    const double* st = s.stash + (size_t)base * (2 * K + 1) * img + p;
    const double w = 1.0 / (st[n_pix] + s.obs_var[j]);
    // the pixels the likelihood counts: not masked, a finite weight (a NaN sci under a masked pixel stays out)
    const bool good = on && !s.bad[j] && fabs(w) <= 1.79769313486231570815e308;
    const double r = s.sci[j] - st[0];
    const double sw = sqrt(w), w2 = w * 0.70710678118654752440;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int e = t * kFisherTile + col;
        double pa = 0.0, pb = 0.0;
        if (good && e < K) {
            const double* plus = st + (size_t)(1 + 2 * e) * img;
            const double* minus = plus + img;
            const double i2h = s.inv2h[(size_t)base * K + e];
            pa = (plus[0] - minus[0]) * i2h * sw;
            pb = (plus[n_pix] - minus[n_pix]) * i2h * w2;
        } else if (good && e == K) {
            pa = sw * r;
            pb = (r * r * w - 1.0) * 0.70710678118654752440;
        }
        va[t] = pa;
        vb[t] = pb;
    }
}
// stencil `base` of a table: the one-field form on that stencil's own images, pixels, window and steps
template <int T>
__device__ inline void fisher_entries(const FisherFieldStencils& s, int base, int K, int n_pix, int p, bool on, int col,
                                      double* va, double* vb) {
    const FisherFieldRec& r = s.recs[base];
    const FisherStencil one{s.stash + r.stash, s.inv2h + r.inv2h, s.sci + r.px, s.obs_var + r.px, s.bad + r.px,
                            ImgWindow{r.nx, r.ly, r.lx, r.ay, r.ax}};
    fisher_entries<T>(one, 0, K, n_pix, p, on, col, va, vb);
}
template <int T>
__device__ inline void fisher_entries(const FisherVectors& s, int, int K, int n_pix, int p, bool on, int col,
                                      double* va, double* vb) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int e = t * kFisherTile + col;
        double pa = 0.0, pb = 0.0;
        if (on && e < K) {
            pa = s.a[(size_t)e * n_pix + p];
            pb = s.b[(size_t)e * n_pix + p];
        } else if (on && e == K) {
            pa = s.c[p];
            pb = s.d[p];
        }
        va[t] = pa;
        vb[t] = pb;
    }
}

// grid ((units + 3) / 4, n_base) x 256 threads: wave u of stencil `base` sums pixels [64 u, 64 u + 64) -- pixel
// slot k = lane >> 4 of step s is pixel 64 u + 4 s + k -- and leaves its T (T + 1) / 2 tiles in
// partial[base][u][tile][reg][lane].
template <int T, class Src>
__global__ void __launch_bounds__(256)
k_fisher_gram(Src src, int K, int n_pix, int units, double* __restrict__ partial) {
    const int lane = threadIdx.x & 63, col = lane & 15, slot = lane >> 4;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6), base = blockIdx.y;
    constexpr int NT = fisher_tiles(T);
    const FisherGeom gm = fisher_geom(src, base, n_pix, units, NT);
    if (u >= gm.units) return;                                     // wave-uniform (a stencil's own count in a table)
    fisher_acc acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = fisher_acc{0.0, 0.0, 0.0, 0.0};
    const int p0 = u * kFisherUnitPx + slot;
#pragma unroll 4
    for (int s = 0; s < kFisherUnitPx / 4; ++s) {
        const int p = p0 + 4 * s;
        const bool on = p < gm.n_pix;
        double va[T], vb[T];
        fisher_entries<T>(src, base, K, gm.n_pix, on ? p : 0, on, col, va, vb);
#pragma unroll
        for (int ti = 0; ti < T; ++ti)
#pragma unroll
            for (int tj = ti; tj < T; ++tj) {
                const int i = fisher_tile_index(T, ti, tj);
                acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[ti], va[tj], acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(vb[ti], vb[tj], acc[i], 0, 0, 0);
            }
    }
    double* out = partial + gm.partial + (size_t)u * NT * kFisherTileDoubles + lane;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) out[(size_t)i * kFisherTileDoubles + reg * 64] = acc[i][reg];
}

// F[base][K][K] and g[base][K] from the waves' partial tiles.  grid (n_base, tiles) x 1024 threads: thread
// (q, slot) adds slot `slot` of the tile over the units u = q, q + 4, ... in that order, the four sums are added in
// the order of q, and the owner of the slot writes element (r, c) and its mirror (c, r) from the one value.
constexpr int kFisherFinishSplit = 4;
// one block's work: tile `tile` of the stencil whose `units` waves' tiles start at `tiles` -> F[K][K], g[K]
__device__ inline void fisher_finish_tile(const double* __restrict__ tiles, int K, int units, int tile,
                                          double* __restrict__ F, double* __restrict__ g) {
    __shared__ double part_sum[kFisherFinishSplit][kFisherTileDoubles];
    const int T = fisher_tile_rows(K), NT = fisher_tiles(T);
    const int slot = threadIdx.x % kFisherTileDoubles, q = threadIdx.x / kFisherTileDoubles;
    const double* p = tiles + (size_t)tile * kFisherTileDoubles + slot;
    double s = 0.0;
#pragma unroll 8
    for (int u = q; u < units; u += kFisherFinishSplit) s += p[(size_t)u * NT * kFisherTileDoubles];
    part_sum[q][slot] = s;
    __syncthreads();
    if (q != 0) return;
    double v = part_sum[0][slot];
    for (int i = 1; i < kFisherFinishSplit; ++i) v += part_sum[i][slot];
    int ti = 0, first = 0;                                         // the tile's place in the triangle: rows ti <= tj
    while (tile >= first + (T - ti)) { first += T - ti; ++ti; }
    const int tj = ti + (tile - first);
    const int lane = slot & 63, reg = slot >> 6;
    const int r = ti * kFisherTile + (lane >> 4) + 4 * reg, c = tj * kFisherTile + (lane & 15);
    if (r >= K || c > K || (ti == tj && r > c)) return;            // padding, or the lower half of a diagonal tile
    if (c == K) {
        g[r] = v;
    } else {
        F[(size_t)r * K + c] = v;
        F[(size_t)c * K + r] = v;
    }
}
__global__ void __launch_bounds__(kFisherFinishSplit * kFisherTileDoubles)
k_fisher_finish(const double* __restrict__ partial, int K, int units, double* __restrict__ F, double* __restrict__ g) {
    const int base = blockIdx.x;
    fisher_finish_tile(partial + (size_t)base * units * fisher_tiles(fisher_tile_rows(K)) * kFisherTileDoubles, K, units,
                       blockIdx.y, F + (size_t)base * K * K, g + (size_t)base * K);
}
// the same for stencils of a table (grid (n_stencils, tiles)): stencil s's own waves, its tiles at recs[s].partial
__global__ void __launch_bounds__(kFisherFinishSplit * kFisherTileDoubles)
k_fisher_finish_fields(const FisherFieldRec* __restrict__ recs, const double* __restrict__ partial, int K,
                       double* __restrict__ F, double* __restrict__ g) {
    const int s = blockIdx.x;
    fisher_finish_tile(partial + recs[s].partial, K, recs[s].units, blockIdx.y, F + (size_t)s * K * K, g + (size_t)s * K);
}

// The stash of a pass whose walkers belong to different stencils: walker w of the pass is walker w0 + w of the call,
// place (w0 + w) % n_st of stencil (w0 + w) / n_st, whose window and stash offset are the table's.  conv / mvar:
// image w of each, S pixels of the transform's shape.  grid (16, n) x 256.
__global__ void __launch_bounds__(256)
k_fisher_stash_fields(const double* __restrict__ conv, const double* __restrict__ mvar, double* __restrict__ stash, int S,
                      const FisherFieldRec* __restrict__ recs, int w0, int n_st) {
    const int w = blockIdx.y, gw = w0 + w;
    const FisherFieldRec& r = recs[fisher_walker_stencil(gw, n_st)];
    const double* src_c = conv + (size_t)w * S;
    const double* src_v = mvar + (size_t)w * S;
    const int n_pix = r.n_pix;
    double* dst = stash + r.stash + (size_t)fisher_walker_place(gw, n_st) * 2 * n_pix;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += gridDim.x * blockDim.x) {
        const int y = i / r.lx, x = i - y * r.lx;
        const int j = (y + r.ay) * r.nx + x + r.ax;
        dst[i] = src_c[j];
        dst[n_pix + i] = src_v[j];
    }
}

// The joint fit's matrix: element e = (b, r, c) of the launch (fisher_link_elem) starts at +0.0 and adds, for
// f = 0 ... n_fields - 1 in that order, field f's F[kr][kc] (c == K_joint: g[kr]) of stencil b n_fields + f, where
// kr, kc = field_col[f][r], field_col[f][c]; a field that does not read both is skipped.  One thread per element, no
// atomics: F_joint is symmetric because every field's F is.
__global__ void __launch_bounds__(256)
k_fisher_link(const double* __restrict__ F, const double* __restrict__ g, const int* __restrict__ field_col,
              int n_base, int n_fields, int K_joint, int K, size_t n_elems, double* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_elems) return;
    int b, r, c;
    fisher_link_elem(e, K_joint, &b, &r, &c);
    double v = 0.0;
    for (int f = 0; f < n_fields; ++f) {
        const int kr = field_col[(size_t)f * K_joint + r];
        const int kc = c < K_joint ? field_col[(size_t)f * K_joint + c] : 0;
        if (kr < 0 || kc < 0) continue;
        const size_t s = (size_t)b * n_fields + f;
        v += c < K_joint ? F[(s * K + kr) * K + kc] : g[s * K + kr];
    }
    out[c < K_joint ? fisher_link_F_at(K_joint, b, r, c) : fisher_link_g_at(n_base, K_joint, b, r)] = v;
}

// the Gram and finish kernels of n_base stencils on `st`
template <class Src>
inline void launch_fisher_gram(const Src& src, int n_base, int K, int n_pix, const FisherPlan& plan, double* partial,
                               double* F, double* g, hipStream_t st) {
    const dim3 grid((plan.units + 3) / 4, n_base), block(256);
    switch (plan.tile_rows) {
        case 1: hipLaunchKernelGGL((k_fisher_gram<1, Src>), grid, block, 0, st, src, K, n_pix, plan.units, partial); break;
        case 2: hipLaunchKernelGGL((k_fisher_gram<2, Src>), grid, block, 0, st, src, K, n_pix, plan.units, partial); break;
        case 3: hipLaunchKernelGGL((k_fisher_gram<3, Src>), grid, block, 0, st, src, K, n_pix, plan.units, partial); break;
        default: hipLaunchKernelGGL((k_fisher_gram<4, Src>), grid, block, 0, st, src, K, n_pix, plan.units, partial); break;
    }
    hipLaunchKernelGGL(k_fisher_finish, dim3(n_base, plan.tiles), dim3(kFisherFinishSplit * kFisherTileDoubles), 0, st, partial,
                       K, plan.units, F, g);
}

// ONE Gram and ONE finish launch for the stencils of a table, whatever their fields: the grid's x extent is the
// largest wave count of the call, and waves past a stencil's own count return
inline void launch_fisher_gram_fields(const FisherFieldStencils& src, int K, const FisherFieldsPlan& plan,
                                      double* partial, double* F, double* g, hipStream_t st) {
    using Src = FisherFieldStencils;
    const dim3 grid((plan.max_units + 3) / 4, plan.n_stencils), block(256);
    switch (plan.tile_rows) {
        case 1: hipLaunchKernelGGL((k_fisher_gram<1, Src>), grid, block, 0, st, src, K, 0, 0, partial); break;
        case 2: hipLaunchKernelGGL((k_fisher_gram<2, Src>), grid, block, 0, st, src, K, 0, 0, partial); break;
        case 3: hipLaunchKernelGGL((k_fisher_gram<3, Src>), grid, block, 0, st, src, K, 0, 0, partial); break;
        default: hipLaunchKernelGGL((k_fisher_gram<4, Src>), grid, block, 0, st, src, K, 0, 0, partial); break;
    }
    hipLaunchKernelGGL(k_fisher_finish_fields, dim3(plan.n_stencils, plan.tiles),
                       dim3(kFisherFinishSplit * kFisherTileDoubles), 0, st, src.recs, partial, K, F, g);
}

}  // namespace psfmc
