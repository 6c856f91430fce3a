// psfmc_sides.h -- THE list of transform sides the fused kernels are built for.  One row per side, ascending:
//     TWO(N, P, T)   a side with a two-stage shape N = P * T (psfmc_fft.h FftShape<N>: T lanes hold P points each)
//     THREE(N)       a side above 1024, which no two-stage shape (P, T <= 32) reaches: three-stage row and column
//                    kernels only (psfmc_fft.h fft3g_pick, psfmc_rows3_path.h rows3_pick)
// Everything that needs the sides expands this list or reads kFusedSides below: the FftShape specialisations, the
// dispatch and its error messages (psfmc_hip.hip DISPATCH_LEN), the embedding's candidates (choose_embedding).
// The per-side picks next to the kernels (fft3g_pick, rows3_pick, rows3_inv_default, row_two_waves_side) and the
// generated cost table (psfmc_side_costs.h) are held to it by static_assert; psfmc_amd/engine.py FUSED_SIDES, the one
// Python copy, by tests/test_host_glue.py.  Why a side has the shape it has: psfmc_fft.h, above the expansion.
// Adding a side: DESIGN.md, "Adding a side".
#pragma once

#define PSFMC_SIDES(TWO, THREE) \
    TWO(64, 8, 8) \
    TWO(84, 7, 12) \
    TWO(88, 11, 8) \
    TWO(96, 12, 8) \
    TWO(98, 7, 14) \
    TWO(100, 10, 10) \
    TWO(104, 13, 8) \
    TWO(110, 10, 11) \
    TWO(112, 14, 8) \
    TWO(120, 15, 8) \
    TWO(126, 9, 14) \
    TWO(128, 16, 8) \
    TWO(130, 10, 13) \
    TWO(132, 11, 12) \
    TWO(140, 10, 14) \
    TWO(144, 12, 12) \
    TWO(150, 10, 15) \
    TWO(156, 12, 13) \
    TWO(160, 10, 16) \
    TWO(168, 12, 14) \
    TWO(176, 11, 16) \
    TWO(180, 12, 15) \
    TWO(192, 12, 16) \
    TWO(196, 14, 14) \
    TWO(200, 20, 10) \
    TWO(208, 13, 16) \
    TWO(210, 14, 15) \
    TWO(220, 11, 20) \
    TWO(224, 14, 16) \
    TWO(240, 15, 16) \
    TWO(250, 25, 10) \
    TWO(252, 14, 18) \
    TWO(256, 16, 16) \
    TWO(260, 13, 20) \
    TWO(264, 22, 12) \
    TWO(280, 14, 20) \
    TWO(286, 22, 13) \
    TWO(288, 24, 12) \
    TWO(294, 14, 21) \
    TWO(300, 15, 20) \
    TWO(308, 11, 28) \
    TWO(312, 24, 13) \
    TWO(320, 16, 20) \
    TWO(330, 22, 15) \
    TWO(336, 16, 21) \
    TWO(350, 25, 14) \
    TWO(352, 22, 16) \
    TWO(360, 18, 20) \
    TWO(364, 13, 28) \
    TWO(384, 16, 24) \
    TWO(390, 15, 26) \
    TWO(392, 14, 28) \
    TWO(400, 20, 20) \
    TWO(416, 26, 16) \
    TWO(420, 20, 21) \
    TWO(440, 20, 22) \
    TWO(448, 16, 28) \
    TWO(480, 20, 24) \
    TWO(484, 22, 22) \
    TWO(500, 20, 25) \
    TWO(504, 21, 24) \
    TWO(512, 32, 16) \
    TWO(520, 20, 26) \
    TWO(528, 22, 24) \
    TWO(560, 20, 28) \
    TWO(572, 22, 26) \
    TWO(576, 24, 24) \
    TWO(600, 24, 25) \
    TWO(616, 22, 28) \
    TWO(624, 24, 26) \
    TWO(630, 21, 30) \
    TWO(640, 20, 32) \
    TWO(650, 25, 26) \
    TWO(660, 22, 30) \
    TWO(672, 24, 28) \
    TWO(676, 26, 26) \
    TWO(700, 25, 28) \
    TWO(704, 22, 32) \
    TWO(720, 24, 30) \
    TWO(728, 26, 28) \
    TWO(768, 24, 32) \
    TWO(780, 26, 30) \
    TWO(784, 28, 28) \
    TWO(800, 25, 32) \
    TWO(832, 26, 32) \
    TWO(840, 28, 30) \
    TWO(896, 28, 32) \
    TWO(900, 30, 30) \
    TWO(960, 30, 32) \
    TWO(1024, 32, 32) \
    THREE(1152) \
    THREE(1280) \
    THREE(1536) \
    THREE(2048)

namespace psfmc {

#define PSFMC_SIDE_N_(N, ...) N,
#define PSFMC_SIDE_P_(N, P, T) P,
#define PSFMC_SIDE_NO_P_(N) 0,
constexpr int kFusedSides[] = {PSFMC_SIDES(PSFMC_SIDE_N_, PSFMC_SIDE_N_)};          // ascending
constexpr int kFusedSideP[] = {PSFMC_SIDES(PSFMC_SIDE_P_, PSFMC_SIDE_NO_P_)};       // P of the two-stage shape, 0: none
#undef PSFMC_SIDE_N_
#undef PSFMC_SIDE_P_
#undef PSFMC_SIDE_NO_P_
constexpr int kNumFusedSides = sizeof(kFusedSides) / sizeof(kFusedSides[0]);
constexpr int kMaxFusedSide = kFusedSides[kNumFusedSides - 1];

constexpr bool fused_sides_ascend() {
    for (int i = 1; i < kNumFusedSides; ++i)
        if (kFusedSides[i - 1] >= kFusedSides[i]) return false;
    return true;
}
static_assert(fused_sides_ascend(), "psfmc_sides.h: the rows are in ascending order, each side once");

// the row of a side, -1: not built (a table, so that the compile-time checks over every length stay cheap)
struct FusedSideRows { short row[kMaxFusedSide + 1]; };
constexpr FusedSideRows fused_side_rows() {
    FusedSideRows r{};
    for (int n = 0; n <= kMaxFusedSide; ++n) r.row[n] = -1;
    for (int i = 0; i < kNumFusedSides; ++i) r.row[kFusedSides[i]] = (short)i;
    return r;
}
constexpr FusedSideRows kFusedSideRows = fused_side_rows();
constexpr int fused_side_index(int n) { return n >= 0 && n <= kMaxFusedSide ? kFusedSideRows.row[n] : -1; }
constexpr bool fused_side(int n) { return fused_side_index(n) >= 0; }
constexpr bool fused_side_has_two_stage_shape(int n) { return fused_side(n) && kFusedSideP[fused_side_index(n)] > 0; }

// for the static_asserts next to the per-side picks: `ok(n)` holds for every length 1 ... the largest side
template <class Pred> constexpr bool for_all_lengths(Pred ok) {
    for (int n = 1; n <= kMaxFusedSide; ++n)
        if (!ok(n)) return false;
    return true;
}

}  // namespace psfmc
