// psfmc_fisher_plan.h -- the host arithmetic of psfmc_fisher_rows, psfmc_fisher_rows_fields and
// psfmc_fisher_rows_joint: argument checks, tile counts, per-stencil offsets and buffer sizes.
// Plain C++ with no HIP in it, so that a stand-alone program can compile it under the host sanitizers
// (tests/host/fisher_plan_check.cpp, tests/host/fisher_fields_plan_check.cpp); psfmc_fisher.h's kernels index their
// tiles, stencils and linked elements with the same functions.
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

// ---------------------------------------------------------------------------
// psfmc_fisher_rows_fields / psfmc_fisher_rows_joint: stencils of DIFFERENT fields in one call.  Every stencil has K
// columns; its pixel count, and so its wave count and the size of its stash and partial tiles, are its field's.
// ---------------------------------------------------------------------------
// what the stash, Gram and finish kernels read of stencil s (a device table, one record per stencil)
struct FisherFieldRec {
    long long px;              // the field's first pixel in the context's sci / obs_var / bad arrays
    long long stash;           // the stencil's [2K+1][2][n_pix] images in the stash (doubles)
    long long partial;         // its [units][tiles][256] partial tiles (doubles)
    long long inv2h;           // its K step reciprocals
    int n_pix, units;          // the field's pixels; ceil(n_pix / 64) waves
    int nx, ly, lx, ay, ax;    // the field's ImgWindow (psfmc_device.h)
    int field;
};

// a field's pixels as the caller of fisher_fields_plan knows them
struct FisherFieldShape {
    long long px;              // FisherFieldRec::px
    int ny, nx, ly, lx, ay, ax;   // rows and row length of the pixel arrays, the image's window in them
};

struct FisherFieldsPlan {
    int W = 0;                 // walkers of the call: n_stencils (2K + 1)
    int tile_rows = 0, tiles = 0;
    int max_units = 0;         // the Gram grid's x extent in waves: the largest unit count of the call
    size_t stash_doubles = 0, partial_doubles = 0;
    size_t io_doubles = 0;     // [n_stencils] x (K step reciprocals, K K + K results)
    int n_stencils = 0;
    FisherFieldRec* recs = nullptr;   // [n_stencils], the caller's array, filled
};

// where stencil s's results stand in the io buffer: inv2h [n][K], then F [n][K][K], then g [n][K]
PSFMC_HD constexpr size_t fisher_fields_F_at(int n_stencils, int K, int s) {
    return (size_t)n_stencils * K + (size_t)s * K * K;
}
PSFMC_HD constexpr size_t fisher_fields_g_at(int n_stencils, int K, int s) {
    return (size_t)n_stencils * K + (size_t)n_stencils * K * K + (size_t)s * K;
}

// nullptr, a filled plan and `recs` [n_stencils] filled (prefix offsets in stencil order), or what is wrong with the
// arguments.  field [n_stencils] names each stencil's field, shapes [n_fields] the fields.
inline const char* fisher_fields_plan(int n_stencils, int K, int max_walkers, int n_fields, const int* field,
                                      const FisherFieldShape* shapes, FisherFieldRec* recs, FisherFieldsPlan* out) {
    if (n_stencils < 1) return "n_stencils must be at least 1";
    if (K < 1 || K > kFisherMaxK) return "K outside [1, 63]";
    if (n_fields < 1 || !field || !shapes || !recs) return "NULL field list";
    const long long W = (long long)n_stencils * (2 * K + 1);
    if (W > max_walkers) return "n_stencils (2K + 1) exceeds max_walkers";
    FisherFieldsPlan p;
    p.W = (int)W;
    p.n_stencils = n_stencils;
    p.tile_rows = fisher_tile_rows(K);
    p.tiles = fisher_tiles(p.tile_rows);
    p.recs = recs;
    size_t stash = 0, partial = 0;
    for (int s = 0; s < n_stencils; ++s) {
        if (field[s] < 0 || field[s] >= n_fields) return "a stencil's field is outside the context's fields";
        const FisherFieldShape& sh = shapes[field[s]];
        if (sh.ly < 1 || sh.lx < 1 || sh.ay < 0 || sh.ax < 0 || (long long)sh.ax + sh.lx > sh.nx ||
            (long long)sh.ay + sh.ly > sh.ny || sh.px < 0)
            return "a field's image window is not inside its pixel rows";
        const size_t n_pix = (size_t)sh.ly * (size_t)sh.lx;
        if (n_pix > (size_t)1 << 30) return "pixel count outside [1, 2^30]";
        FisherFieldRec& r = recs[s];
        r.px = sh.px;
        r.stash = (long long)stash;
        r.partial = (long long)partial;
        r.inv2h = (long long)s * K;
        r.n_pix = (int)n_pix;
        r.units = (int)((n_pix + kFisherUnitPx - 1) / kFisherUnitPx);
        r.nx = sh.nx; r.ly = sh.ly; r.lx = sh.lx; r.ay = sh.ay; r.ax = sh.ax;
        r.field = field[s];
        if (r.units > p.max_units) p.max_units = r.units;
        stash += (size_t)(2 * K + 1) * 2 * n_pix;
        partial += (size_t)r.units * p.tiles * kFisherTileDoubles;
    }
    p.stash_doubles = stash;
    p.partial_doubles = partial;
    p.io_doubles = (size_t)n_stencils * ((size_t)K + (size_t)K * K + K);
    if (out) *out = p;
    return nullptr;
}

// the stencil and the place in it of walker w of a call whose stencils have n_st = 2K + 1 walkers each
PSFMC_HD constexpr int fisher_walker_stencil(int w, int n_st) { return w / n_st; }
PSFMC_HD constexpr int fisher_walker_place(int w, int n_st) { return w % n_st; }

// ---------------------------------------------------------------------------
// The joint fit's matrix (k_fisher_link): field f's columns kr stand at joint columns col_of[f][kr].  The kernel reads
// the inverse map, field_col[f][joint column] = the field's column or -1; element (r, c) of F_joint[b] sums the
// fields that read both, in field order.
// ---------------------------------------------------------------------------
struct FisherJointPlan {
    int n_stencils = 0;        // n_base n_fields; stencil b n_fields + f is field f's of base b
    size_t link_doubles = 0;   // [n_base] x (K_joint K_joint + K_joint) results
    size_t link_elems = 0;     // threads of the link launch: n_base K_joint (K_joint + 1)
};

// nullptr, the plan and field_col [n_fields][K_joint] filled, or what is wrong
inline const char* fisher_joint_plan(int n_base, int n_fields, int K_joint, int K_field, int max_walkers,
                                     const int* col_of, int* field_col, FisherJointPlan* out) {
    if (n_base < 1) return "n_base must be at least 1";
    if (n_fields < 1) return "n_fields must be at least 1";
    if (K_field < 1 || K_field > kFisherMaxK) return "K_field outside [1, 63]";
    if (K_joint < K_field || K_joint > (1 << 20)) return "K_joint outside [K_field, 2^20]";
    if (!col_of || !field_col) return "NULL column map";
    const long long n_st = (long long)n_base * n_fields;
    if (n_st * (2 * K_field + 1) > max_walkers) return "n_base n_fields (2 K_field + 1) exceeds max_walkers";
    const unsigned long long per_base = (unsigned long long)K_joint * ((unsigned long long)K_joint + 1);
    if (per_base > (1ull << 40) / (unsigned long long)n_base) return "n_base K_joint (K_joint + 1) exceeds 2^40";
    for (long long i = 0; i < (long long)n_fields * K_joint; ++i) field_col[i] = -1;
    for (int f = 0; f < n_fields; ++f)
        for (int k = 0; k < K_field; ++k) {
            const int j = col_of[(size_t)f * K_field + k];
            if (j < 0 || j >= K_joint) return "col_of names a column outside [0, K_joint)";
            int& slot = field_col[(size_t)f * K_joint + j];
            if (slot >= 0) return "col_of is not injective: two columns of a field at one joint column";
            slot = k;
        }
    FisherJointPlan p;
    p.n_stencils = (int)n_st;
    p.link_elems = (size_t)(per_base * (unsigned long long)n_base);
    p.link_doubles = p.link_elems;
    if (out) *out = p;
    return nullptr;
}

// element e of the link launch: base b, row r < K_joint, column c <= K_joint (c == K_joint: the gradient)
PSFMC_HD inline void fisher_link_elem(size_t e, int K_joint, int* b, int* r, int* c) {
    const size_t per_row = (size_t)K_joint + 1, per_base = (size_t)K_joint * per_row;
    *b = (int)(e / per_base);
    const size_t rem = e - (size_t)*b * per_base;
    *r = (int)(rem / per_row);
    *c = (int)(rem - (size_t)*r * per_row);
}
// where the link leaves F_joint[b][r][c] and g_joint[b][r]: F [n_base][K_joint][K_joint], then g [n_base][K_joint]
PSFMC_HD constexpr size_t fisher_link_F_at(int K_joint, int b, int r, int c) {
    return ((size_t)b * K_joint + r) * K_joint + c;
}
PSFMC_HD constexpr size_t fisher_link_g_at(int n_base, int K_joint, int b, int r) {
    return (size_t)n_base * K_joint * K_joint + (size_t)b * K_joint + r;
}

}  // namespace psfmc
