// psfmc_fisher_plan.h -- the host arithmetic of psfmc_fisher_rows: argument checks, tile counts and buffer sizes.
// Plain C++ with no HIP in it, so that a stand-alone program can compile it under the host sanitizers
// (tests/host/fisher_plan_check.cpp); psfmc_fisher.h's kernels index their tiles with the same functions.
#pragma once

#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSFMC_HD __host__ __device__
#else
#define PSFMC_HD
#endif

namespace psfmc {

constexpr int kFisherTile = 16;        // side of a v_mfma_f64_16x16x4_f64 result tile
constexpr int kFisherMaxTiles = 4;     // tile rows the Gram kernel is built for
// differentiated columns of one stencil: K + 1 vectors (the K derivative pairs and the gradient's column) in
// kFisherMaxTiles tile rows
constexpr int kFisherMaxK = kFisherTile * kFisherMaxTiles - 1;
// pixels of one wave: the 4 pixel slots of the MFMA k-dimension x 16 steps.  (256 pixels per wave left a 256^2 image
// to 256 waves, one per compute unit, each waiting out 64 rounds of loads: 67 us a call; measured)
constexpr int kFisherUnitPx = 64;
constexpr int kFisherTileDoubles = 256;   // a tile in the registers of one wave: 4 per lane

// tile rows of K columns: the extended Gram matrix has K + 1 rows and columns
PSFMC_HD constexpr int fisher_tile_rows(int K) { return (K + 1 + kFisherTile - 1) / kFisherTile; }
// tiles of the upper triangle of T tile rows, and the place of tile (ti <= tj) among them (row-major)
PSFMC_HD constexpr int fisher_tiles(int T) { return T * (T + 1) / 2; }
PSFMC_HD constexpr int fisher_tile_index(int T, int ti, int tj) { return ti * T - ti * (ti - 1) / 2 + (tj - ti); }

struct FisherPlan {
    int W = 0;                 // walkers of the call: n_base (2K + 1)
    int tile_rows = 0, tiles = 0;
    int units = 0;             // waves (partial sums) per stencil
    size_t stash_doubles = 0;  // [W][2][n_pix] convolved model and model variance of every stencil walker
    size_t partial_doubles = 0;   // [n_base][units][tiles][256]
    size_t io_doubles = 0;     // [n_base] x (K step reciprocals, K K + K results)
};

// nullptr and a filled plan, or what is wrong with the arguments
inline const char* fisher_plan(int n_base, int K, int max_walkers, size_t n_pix, FisherPlan* out) {
    if (n_base < 1) return "n_base must be at least 1";
    if (K < 1 || K > kFisherMaxK) return "K outside [1, 63]";
    if (n_pix < 1 || n_pix > (size_t)1 << 30) return "pixel count outside [1, 2^30]";
    const long long W = (long long)n_base * (2 * K + 1);
    if (W > max_walkers) return "n_base (2K + 1) exceeds max_walkers";
    FisherPlan p;
    p.W = (int)W;
    p.tile_rows = fisher_tile_rows(K);
    p.tiles = fisher_tiles(p.tile_rows);
    p.units = (int)((n_pix + kFisherUnitPx - 1) / kFisherUnitPx);
    p.stash_doubles = (size_t)W * 2 * n_pix;
    p.partial_doubles = (size_t)n_base * p.units * p.tiles * kFisherTileDoubles;
    p.io_doubles = (size_t)n_base * ((size_t)K + (size_t)K * K + K);
    if (out) *out = p;
    return nullptr;
}

// where element (row, col) of a result tile sits in a wave: f64 results are 4 per lane with
// col = lane & 15, row = (lane >> 4) + 4 reg -- NOT the f32 shapes' row = 4 (lane >> 4) + reg
PSFMC_HD constexpr int fisher_tile_slot(int row, int col) { return (row >> 2) * 64 + (row & 3) * 16 + col; }

}  // namespace psfmc
