// Stand-alone check of the host arithmetic of psfmc_fisher_rows (psfmc_amd/csrc/psfmc_fisher_plan.h: argument checks,
// tile indices, buffer sizes).  No HIP in it: build with the host compiler and its sanitizers,
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all fisher_plan_check.cpp -o fisher_plan_check
// It fills buffers of exactly the planned sizes through the kernels' own index functions, so that an index past a
// planned size is an AddressSanitizer report, and an overflow in the size arithmetic an UBSan one.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../psfmc_amd/csrc/psfmc_fisher_plan.h"

using namespace psfmc;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

int main() {
    FisherPlan p;
    // refusals
    CHECK(fisher_plan(0, 3, 100, 64, &p) != nullptr);
    CHECK(fisher_plan(1, 0, 100, 64, &p) != nullptr);
    CHECK(fisher_plan(1, kFisherMaxK + 1, 1000, 64, &p) != nullptr);
    CHECK(fisher_plan(1, 3, 6, 64, &p) != nullptr);                    // 7 walkers > 6
    CHECK(fisher_plan(1, 3, 7, 0, &p) != nullptr);
    CHECK(fisher_plan(1 << 30, 63, 1 << 30, 64, &p) != nullptr);       // n_base (2K + 1) overflows an int: refused
    CHECK(fisher_plan(1, 3, 7, 64, nullptr) == nullptr);

    const int Ks[] = {1, 3, 15, 16, 17, 31, 33, 47, 63};
    const size_t pixels[] = {1, 3, 4, 255, 256, 257, 4099, 70 * 64};
    for (int K : Ks)
        for (size_t n_pix : pixels)
            for (int n_base : {1, 3}) {
                CHECK(fisher_plan(n_base, K, n_base * (2 * K + 1), n_pix, &p) == nullptr);
                CHECK(p.W == n_base * (2 * K + 1));
                CHECK(p.tile_rows >= 1 && p.tile_rows <= kFisherMaxTiles);
                CHECK(p.tile_rows * kFisherTile >= K + 1 && (p.tile_rows - 1) * kFisherTile < K + 1);
                CHECK((size_t)p.units * kFisherUnitPx >= n_pix && (size_t)(p.units - 1) * kFisherUnitPx < n_pix);
                // every upper-triangle tile has its own place
                std::vector<int> seen(p.tiles, 0);
                for (int ti = 0; ti < p.tile_rows; ++ti)
                    for (int tj = ti; tj < p.tile_rows; ++tj) ++seen[fisher_tile_index(p.tile_rows, ti, tj)];
                for (int s : seen) CHECK(s == 1);
                // the stash as the stash kernel writes it and the Gram kernel reads it
                std::vector<double> stash(p.stash_doubles, 0.0);
                for (int w = 0; w < p.W; ++w)
                    for (int ch = 0; ch < 2; ++ch) stash[((size_t)w * 2 + ch) * n_pix + (n_pix - 1)] += 1.0;
                for (int b = 0; b < n_base; ++b)
                    for (int e = 0; e < K; ++e) {
                        const size_t img = 2 * n_pix;
                        const size_t plus = (size_t)b * (2 * K + 1) * img + (size_t)(1 + 2 * e) * img;
                        CHECK(stash[plus + n_pix - 1] == 1.0 && stash[plus + img + n_pix + n_pix - 1] == 1.0);
                    }
                // the partial tiles as the Gram kernel writes them, read back as the finish kernel reads them
                std::vector<double> part(p.partial_doubles, 0.0);
                for (int b = 0; b < n_base; ++b)
                    for (int u = 0; u < p.units; ++u)
                        for (int i = 0; i < p.tiles; ++i)
                            for (int reg = 0; reg < 4; ++reg)
                                for (int lane = 0; lane < 64; ++lane)
                                    part[(((size_t)b * p.units + u) * p.tiles + i) * kFisherTileDoubles + reg * 64 + lane] =
                                        (lane >> 4) + 4 * reg + 100.0 * (lane & 15);       // row + 100 col of the f64 map
                for (int r = 0; r < K; ++r)
                    for (int c = r; c <= K; ++c) {
                        const size_t at = ((size_t)(n_base - 1) * p.units + (p.units - 1)) * p.tiles * kFisherTileDoubles +
                                          (size_t)fisher_tile_index(p.tile_rows, r >> 4, c >> 4) * kFisherTileDoubles +
                                          fisher_tile_slot(r & 15, c & 15);
                        CHECK(part[at] == (r & 15) + 100.0 * (c & 15));
                    }
                // step reciprocals and results
                std::vector<double> io(p.io_doubles, 0.0);
                io[(size_t)n_base * K + (size_t)n_base * K * K + (size_t)n_base * K - 1] = 1.0;
            }
    if (failures) return 1;
    std::printf("fisher plan ok\n");
    return 0;
}
