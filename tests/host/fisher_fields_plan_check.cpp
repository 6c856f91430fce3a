// Stand-alone check of the host arithmetic of psfmc_fisher_rows_fields and psfmc_fisher_rows_joint
// (psfmc_amd/csrc/psfmc_fisher_plan.h: fisher_fields_plan, fisher_joint_plan and the link's index functions).  No HIP
// in it: build with the host compiler and its sanitizers,
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all fisher_fields_plan_check.cpp -o fisher_fields_plan_check
// It fills buffers of exactly the planned sizes through the index functions the kernels use, walking them as the stash,
// Gram, finish and link kernels do, so that an index past a planned size is an AddressSanitizer report and an overflow
// in the size arithmetic an UBSan one.
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

// three fields in a 72 x 72 transform: 62 x 66 = 4092 pixels (not whole waves), 70 x 64 = 4480, 64 x 64 = 4096
static const int kS = 72 * 72;
static const FisherFieldShape kShapes[3] = {
    {0 * kS, 72, 72, 62, 66, 5, 3}, {1 * kS, 72, 72, 70, 64, 1, 4}, {2 * kS, 72, 72, 64, 64, 0, 0}};
static const int kPixels[3] = {4092, 4480, 4096};

static void check_fields(int K, const std::vector<int>& field) {
    const int n = (int)field.size(), n_st = 2 * K + 1;
    std::vector<FisherFieldRec> recs(n);
    FisherFieldsPlan p;
    CHECK(fisher_fields_plan(n, K, n * n_st, 3, field.data(), kShapes, recs.data(), &p) == nullptr);
    CHECK(p.W == n * n_st && p.n_stencils == n && p.recs == recs.data());
    CHECK(p.tile_rows * kFisherTile >= K + 1 && (p.tile_rows - 1) * kFisherTile < K + 1);
    CHECK(p.tiles == fisher_tiles(p.tile_rows));
    size_t stash = 0, partial = 0;
    int max_units = 0;
    for (int s = 0; s < n; ++s) {                                       // prefix offsets in stencil order
        const FisherFieldRec& r = recs[s];
        const int n_pix = kPixels[field[s]];
        CHECK(r.field == field[s] && r.n_pix == n_pix && r.px == (long long)field[s] * kS);
        CHECK(r.units == (n_pix + 63) / 64);
        CHECK((size_t)r.stash == stash && (size_t)r.partial == partial && r.inv2h == (long long)s * K);
        CHECK(r.ly * r.lx == n_pix && r.nx == 72);
        stash += (size_t)n_st * 2 * n_pix;
        partial += (size_t)r.units * p.tiles * kFisherTileDoubles;
        if (r.units > max_units) max_units = r.units;
    }
    CHECK(p.stash_doubles == stash && p.partial_doubles == partial && p.max_units == max_units);
    CHECK(kPixels[0] % 64 != 0 && (kPixels[0] + 63) / 64 == 64 && kPixels[1] / 64 == 70 && kPixels[2] / 64 == 64);
    // the stash as k_fisher_stash_fields writes it (walker w of the call) and the Gram kernel reads it
    std::vector<double> st(p.stash_doubles, 0.0);
    std::vector<double> pixels((size_t)3 * kS, 0.0);                    // the context's pixel arrays
    for (int w = 0; w < p.W; ++w) {
        const FisherFieldRec& r = recs[fisher_walker_stencil(w, n_st)];
        const size_t dst = (size_t)r.stash + (size_t)fisher_walker_place(w, n_st) * 2 * r.n_pix;
        for (int i = 0; i < r.n_pix; ++i) {
            const int y = i / r.lx, x = i - y * r.lx;
            pixels[(size_t)r.px + (size_t)(y + r.ay) * r.nx + x + r.ax] += 1.0;      // the window stays inside the field
            st[dst + i] += 1.0;
            st[dst + r.n_pix + i] += 1.0;
        }
    }
    for (double v : st) CHECK(v == 1.0);                               // every double written once: no overlap, no gap
    for (int s = 0; s < n; ++s)
        for (int e = 0; e < K; ++e) {
            const size_t img = 2 * (size_t)recs[s].n_pix;
            const size_t plus = (size_t)recs[s].stash + (size_t)(1 + 2 * e) * img;
            CHECK(st[plus + recs[s].n_pix - 1] == 1.0 && st[plus + img + img - 1] == 1.0);
        }
    // the partial tiles: wave u < its stencil's units of a grid max_units wide writes, the finish reads them back
    std::vector<double> part(p.partial_doubles, 0.0);
    for (int s = 0; s < n; ++s)
        for (int u = 0; u < p.max_units; ++u) {
            if (u >= recs[s].units) continue;
            for (int i = 0; i < p.tiles; ++i)
                for (int slot = 0; slot < kFisherTileDoubles; ++slot)
                    part[(size_t)recs[s].partial + ((size_t)u * p.tiles + i) * kFisherTileDoubles + slot] += 1.0;
        }
    for (double v : part) CHECK(v == 1.0);
    // step reciprocals and results
    std::vector<double> io(p.io_doubles, 0.0);
    for (int s = 0; s < n; ++s) {
        io[(size_t)recs[s].inv2h + K - 1] += 1.0;
        io[fisher_fields_F_at(n, K, s) + (size_t)K * K - 1] += 1.0;
        io[fisher_fields_g_at(n, K, s) + K - 1] += 1.0;
    }
    CHECK(fisher_fields_g_at(n, K, n - 1) + K == p.io_doubles);
}

static void check_joint(int n_base, int n_fields, int K_field, int n_shared) {
    // field f reads the n_shared shared joint columns and K_field - n_shared of its own, in an interleaved order
    const int K_joint = n_shared + n_fields * (K_field - n_shared) + 1;      // (+ 1: a joint column no field reads)
    std::vector<int> col_of((size_t)n_fields * K_field), field_col((size_t)n_fields * K_joint);
    for (int f = 0; f < n_fields; ++f)
        for (int k = 0; k < K_field; ++k)
            col_of[(size_t)f * K_field + k] =
                k < K_field - n_shared ? n_shared + (K_field - n_shared) * f + k : k - (K_field - n_shared);
    FisherJointPlan p;
    const int W = n_base * n_fields * (2 * K_field + 1);
    CHECK(fisher_joint_plan(n_base, n_fields, K_joint, K_field, W, col_of.data(), field_col.data(), &p) == nullptr);
    CHECK(p.n_stencils == n_base * n_fields);
    CHECK(p.link_elems == (size_t)n_base * K_joint * (K_joint + 1) && p.link_doubles == p.link_elems);
    for (int f = 0; f < n_fields; ++f) {
        int read = 0;
        for (int j = 0; j < K_joint; ++j) {
            const int k = field_col[(size_t)f * K_joint + j];
            CHECK(k >= -1 && k < K_field);
            if (k >= 0) { ++read; CHECK(col_of[(size_t)f * K_field + k] == j); }
        }
        CHECK(read == K_field && field_col[(size_t)f * K_joint + K_joint - 1] == -1);
    }
    // the link: every element of the results written once, from reads inside the fields' results
    std::vector<double> F((size_t)p.n_stencils * K_field * K_field, 1.0), g((size_t)p.n_stencils * K_field, 1.0);
    std::vector<double> out(p.link_doubles, -1.0);
    for (size_t e = 0; e < p.link_elems; ++e) {
        int b, r, c;
        fisher_link_elem(e, K_joint, &b, &r, &c);
        CHECK(b >= 0 && b < n_base && r >= 0 && r < K_joint && c >= 0 && c <= K_joint);
        double v = 0.0;
        for (int f = 0; f < n_fields; ++f) {
            const int kr = field_col[(size_t)f * K_joint + r];
            const int kc = c < K_joint ? field_col[(size_t)f * K_joint + c] : 0;
            if (kr < 0 || kc < 0) continue;
            const size_t s = (size_t)b * n_fields + f;
            v += c < K_joint ? F[(s * K_field + kr) * K_field + kc] : g[s * K_field + kr];
        }
        const size_t at = c < K_joint ? fisher_link_F_at(K_joint, b, r, c) : fisher_link_g_at(n_base, K_joint, b, r);
        CHECK(out[at] == -1.0);
        out[at] = v;
        const bool shared_r = r < n_shared, shared_c = c < n_shared, none = r == K_joint - 1 || c == K_joint - 1;
        if (c == K_joint) CHECK(v == (r == K_joint - 1 ? 0.0 : shared_r ? (double)n_fields : 1.0));
        else if (none) CHECK(v == 0.0);
        else if (shared_r && shared_c) CHECK(v == (double)n_fields);
    }
    for (double v : out) CHECK(v >= 0.0);
}

int main() {
    FisherFieldsPlan p;
    FisherFieldRec recs[4];
    const int f012[] = {0, 1, 2}, bad_hi[] = {0, 3, 1}, bad_lo[] = {-1, 0, 1};
    // refusals
    CHECK(fisher_fields_plan(0, 3, 100, 3, f012, kShapes, recs, &p) != nullptr);
    CHECK(fisher_fields_plan(3, 0, 100, 3, f012, kShapes, recs, &p) != nullptr);
    CHECK(fisher_fields_plan(3, kFisherMaxK + 1, 1000, 3, f012, kShapes, recs, &p) != nullptr);
    CHECK(fisher_fields_plan(3, 3, 20, 3, f012, kShapes, recs, &p) != nullptr);          // 21 walkers > 20
    CHECK(fisher_fields_plan(3, 3, 21, 3, f012, kShapes, recs, nullptr) == nullptr);
    CHECK(fisher_fields_plan(3, 3, 21, 3, bad_hi, kShapes, recs, &p) != nullptr);
    CHECK(fisher_fields_plan(3, 3, 21, 3, bad_lo, kShapes, recs, &p) != nullptr);
    CHECK(fisher_fields_plan(3, 3, 21, 3, nullptr, kShapes, recs, &p) != nullptr);
    CHECK(fisher_fields_plan(3, 3, 21, 3, f012, nullptr, recs, &p) != nullptr);
    CHECK(fisher_fields_plan(3, 3, 21, 3, f012, kShapes, nullptr, &p) != nullptr);
    CHECK(fisher_fields_plan(1 << 30, 63, 1 << 30, 3, f012, kShapes, recs, &p) != nullptr);   // the walker count overflows an int
    {
        FisherFieldShape outside[3] = {kShapes[0], kShapes[1], kShapes[2]};
        outside[1].ax = 72 - 64 + 1;                                    // one pixel past the row
        CHECK(fisher_fields_plan(3, 3, 21, 3, f012, outside, recs, &p) != nullptr);
        outside[1] = kShapes[1];
        outside[1].ay = 72 - 70 + 1;                                    // one row past the array
        CHECK(fisher_fields_plan(3, 3, 21, 3, f012, outside, recs, &p) != nullptr);
    }
    const int Ks[] = {1, 11, 15, 16, 31, 32, 47, 48, 62, 63};
    for (int K : Ks) {
        check_fields(K, {0, 1, 2});
        check_fields(K, {2, 0, 1, 0});
        check_fields(K, {1});
    }

    // the joint plan
    FisherJointPlan jp;
    std::vector<int> fc(3 * 8);
    const int inj[] = {0, 1, 2, 3, 4, 5}, twice[] = {0, 1, 2, 2, 4, 5}, past[] = {0, 1, 2, 3, 4, 8}, neg[] = {0, 1, -1, 3, 4, 5};
    CHECK(fisher_joint_plan(1, 3, 8, 2, 15, inj, fc.data(), &jp) == nullptr);
    CHECK(fisher_joint_plan(1, 3, 8, 2, 15, twice, fc.data(), &jp) != nullptr);          // field 1 reads column 2 twice
    CHECK(fisher_joint_plan(1, 3, 8, 2, 15, past, fc.data(), &jp) != nullptr);
    CHECK(fisher_joint_plan(1, 3, 8, 2, 15, neg, fc.data(), &jp) != nullptr);
    CHECK(fisher_joint_plan(0, 3, 8, 2, 15, inj, fc.data(), &jp) != nullptr);
    CHECK(fisher_joint_plan(1, 0, 8, 2, 15, inj, fc.data(), &jp) != nullptr);
    CHECK(fisher_joint_plan(1, 3, 8, 0, 15, inj, fc.data(), &jp) != nullptr);
    CHECK(fisher_joint_plan(1, 3, 8, kFisherMaxK + 1, 1000, inj, fc.data(), &jp) != nullptr);
    CHECK(fisher_joint_plan(1, 3, 1, 2, 15, inj, fc.data(), &jp) != nullptr);            // K_joint < K_field
    CHECK(fisher_joint_plan(1, 3, 8, 2, 14, inj, fc.data(), &jp) != nullptr);            // 15 walkers > 14
    CHECK(fisher_joint_plan(1, 3, 8, 2, 15, nullptr, fc.data(), &jp) != nullptr);
    CHECK(fisher_joint_plan(1, 3, 8, 2, 15, inj, nullptr, &jp) != nullptr);
    CHECK(fisher_joint_plan(1 << 30, 3, 8, 63, 1 << 30, inj, fc.data(), &jp) != nullptr);
    CHECK(fisher_joint_plan(1 << 24, 1, 1 << 20, 2, 1 << 30, inj, fc.data(), &jp) != nullptr);   // 2^64 elements
    check_joint(1, 3, 11, 5);                                           // K_joint = 24
    check_joint(2, 3, 25, 0);                                           // K_joint = 76 > 63, nothing shared
    check_joint(2, 1, 63, 63);                                          // one field, everything "shared"
    check_joint(1, 4, 15, 14);
    check_joint(1, 2, 16, 1);
    if (failures) return 1;
    std::printf("fisher fields plan ok\n");
    return 0;
}
