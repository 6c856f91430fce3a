// A field's auxiliary table on the host: the record of what the field registered, and the one function that
// composes the table the device reads from it.  No HIP call in this file.
//
// The table: the base entries (psfmc_set_aux_layout: 2 n_sky + n_sersic), then the blocks in the order of kAuxBlocks
// -- Fourier modes, spiral arms, radial laws, truncations, bending modes -- each with the entries of psfmc_set_*_layout.  A table index is the
// entry's place in the walker's auxiliary vector, so a present block forces every block before it to be present:
// where the field registered none, that block is PADDED with entries no kernel reads (column -1 and the block's
// pad constants, inside the support of what would read them).
#pragma once
#include <vector>

#include "../../include/psfmc_hip.h"
#include "psfmc_general.h"

namespace psfmc {

enum { kBlkFou = 0, kBlkSpi, kBlkRad, kBlkTru, kBlkBnd, kAuxBlocks };

// A block's facts, in table order: its name in messages, its sizes, how a registration's per-Sersic tag becomes the
// mask byte the kernels read, and which blocks' buffers a context that has it carries.
struct AuxBlockFacts {
    const char *name, *what, *excl;      // psfmc_set_<name>_layout; "components that have <what>"; "<excl> and integrate"
    int in;                              // table entries per Sersic
    int par;                             // per-walker device constants per Sersic
    int flag, deg_bit;                   // mask byte: flag (0: the tag itself) | deg_bit where the angles are in degrees
    int any_bits;                        // the bits of a mask byte that say "registered"
    int first;                           // a context with this block carries the buffers of blocks first ... this one
};
// mask bytes: mode mask (bit m - 1), bit 6: the phases are in degrees | bit 0: the component has a spiral, bit 1:
// angles in degrees | the kind, 0: the Sersic law, 1: Moffat, 2: Ferrer | bit 0: inner, bit 1: outer | bending mode
// mask (bit m - 1)
constexpr AuxBlockFacts kAuxBlock[kAuxBlocks] = {
    {"fourier", "modes", "fourier", kFouPar, kFouPar, 0, kFouDegrees, kFouModeBits, kBlkFou},
    {"spiral", "a spiral", "spiral", kSpiIn, kSpiPar, kSpiFlag, kSpiDegrees, kSpiFlag, kBlkSpi},
    {"radial", "a radial law", "a radial law", kRadIn, kRadPar, 0, 0, 0xff, kBlkFou},
    {"truncation", "a truncation", "truncation", kTruIn, kTruPar, 0, 0, kTruInner | kTruOuter, kBlkFou},
    {"bending", "bending modes", "bending", kBndIn, kBndPar, 0, 0, kBndModeBits, kBlkFou},
};
static_assert(kFouModes == PSFMC_FOURIER_MODES && kAuxBlock[kBlkFou].in == 2 * PSFMC_FOURIER_MODES,
              "mode count of include/psfmc_hip.h");
static_assert(kAuxBlock[kBlkSpi].in == PSFMC_SPIRAL_PARAMS, "spiral parameter count of include/psfmc_hip.h");
static_assert(kAuxBlock[kBlkRad].in == PSFMC_RADIAL_PARAMS, "radial parameter count of include/psfmc_hip.h");
static_assert(kAuxBlock[kBlkTru].in == PSFMC_TRUNC_PARAMS, "truncation parameter count of include/psfmc_hip.h");
static_assert(kBndModes == PSFMC_BEND_MODES && kAuxBlock[kBlkBnd].in == PSFMC_BEND_MODES,
              "bending mode count of include/psfmc_hip.h");

// entries of block b for n_sersic components
inline int aux_block_len(int b, int n_sersic) { return kAuxBlock[b].in * n_sersic; }

// what one registration call passed: the per-Sersic tags (mode masks, spiral flags, radial kinds, truncation sides,
// bending mode masks) and the entries.
// Empty: never registered, dropped, or registered with all-zero tags.
struct AuxBlockRecord {
    std::vector<int> tags, col;
    std::vector<double> konst;
    bool empty() const { return tags.empty(); }
    void clear() { tags.clear(); col.clear(); konst.clear(); }
    void store(int n_sersic, int len, const int* t, const int* cl, const double* k) {
        clear();
        bool any = false;
        for (int i = 0; i < n_sersic; ++i) any = any || t[i];
        if (!any) return;
        tags.assign(t, t + n_sersic);
        col.assign(cl, cl + len);
        konst.assign(k, k + len);
    }
};

struct FieldAuxRecord {
    std::vector<int> sersic_degrees;     // psfmc_set_layout's, [n_sersic]
    std::vector<int> base_col;           // psfmc_set_aux_layout's aux_col / aux_const
    std::vector<double> base_const;
    AuxBlockRecord block[kAuxBlocks];
};

// the table in upload order: konst | col | kinds | sides.  kinds (the radial kinds, [n_sersic]) is empty without a radial
// block (zeros where the block is only padding in front of the truncations or the bending modes).
struct AuxTable {
    std::vector<double> konst;
    // sides: the truncation sides, [n_sersic], empty without a truncation block (zeros where it is only padding in
    // front of the bending modes); bends: the bending mode masks, [n_sersic], empty without bending modes (no kernel
    // reads them from the table: the support needs no mask)
    std::vector<int> col, kinds, sides, bends;
    int n_aux = 0, n_fou = 0, n_spi = 0, n_rad = 0, n_tru = 0, n_bnd = 0;
};

inline AuxTable compose_aux_table(const FieldAuxRecord& r, int n_sky, int n_sersic) {
    AuxTable t;
    if ((int)r.base_col.size() != aux_len(n_sky, n_sersic) || r.base_col.empty()) return t;   // no aux layout, no table
    t.col = r.base_col;
    t.konst = r.base_const;
    int last = -1;                       // the last block the field registered
    for (int b = 0; b < kAuxBlocks; ++b)
        if (!r.block[b].empty()) last = b;
    int n[kAuxBlocks] = {0, 0, 0, 0, 0};
    for (int b = 0; b <= last; ++b) {
        const AuxBlockRecord& blk = r.block[b];
        const size_t at = t.col.size();
        n[b] = aux_block_len(b, n_sersic);
        if (!blk.empty()) {
            t.col.insert(t.col.end(), blk.col.begin(), blk.col.end());
            t.konst.insert(t.konst.end(), blk.konst.begin(), blk.konst.end());
            continue;
        }
        t.col.resize(at + n[b], -1);
        t.konst.resize(at + n[b], 0.0);
        if (b == kBlkSpi)
            for (int k = 0; k < n_sersic; ++k) t.konst[at + kSpiIn * k + 1] = 1.0;   // r_out > r_in = 0
    }
    if (last >= kBlkRad) {
        t.kinds = r.block[kBlkRad].tags;
        if (t.kinds.empty()) t.kinds.assign(n_sersic, 0);
    }
    if (last >= kBlkTru) {
        t.sides = r.block[kBlkTru].tags;
        if (t.sides.empty()) t.sides.assign(n_sersic, 0);
    }
    if (last == kBlkBnd) t.bends = r.block[kBlkBnd].tags;
    t.n_aux = (int)t.col.size();
    t.n_fou = n[kBlkFou]; t.n_spi = n[kBlkSpi]; t.n_rad = n[kBlkRad]; t.n_tru = n[kBlkTru];
    t.n_bnd = n[kBlkBnd];
    return t;
}

}  // namespace psfmc
