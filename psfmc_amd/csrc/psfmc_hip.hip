// psfmc_hip.hip -- C ABI of libpsfmc_hip.so (see include/psfmc_hip.h).
// gfx950 only.  Build: psfmc_amd/csrc/Makefile (hipcc --offload-arch=gfx950).
#include "../../include/psfmc_hip.h"
#include "psfmc_side_costs.h"

// The file compiles either as one translation unit (PSFMC_NPARTS undefined: everything) or as
// PSFMC_NPARTS = 4 of them built in parallel (csrc/Makefile): every part instantiates the per-side
// kernels of its share of the sides behind psfmc_size_call_part<k>; part 0 is also the API.
#ifndef PSFMC_NPARTS
#define PSFMC_NPARTS 1
#define PSFMC_PART 0
#endif

#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "psfmc_device.h"
#if PSFMC_PART == 0
#include "psfmc_hipfft_path.h"
#endif
#include "psfmc_fused_path.h"
#include "psfmc_rows3_path.h"
#include "psfmc_theta.h"
#include "psfmc_fisher_plan.h"   // (every part: the context holds a table of its records)
#if PSFMC_PART == 0
#include "psfmc_integrated.h"
#include "psfmc_general.h"
#include "psfmc_general_mean.h"
#include "psfmc_aux_table.h"
#include "psfmc_fisher.h"
#endif

using namespace psfmc;

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
#define PSFMC_NOT_MINE (-1000)          /* a part's answer for a side another part builds */

int psfmc_fail_(int code, const char* fmt, ...);
#define fail psfmc_fail_
#if PSFMC_PART == 0
static thread_local std::string g_err;

int psfmc_fail_(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#endif

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(e_ == hipErrorOutOfMemory ? PSFMC_ENOMEM : PSFMC_EHIP,          \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                      \
    } while (0)

#define FFT_TRY(expr)                                                                  \
    do {                                                                               \
        hipfftResult r_ = (expr);                                                      \
        if (r_ != HIPFFT_SUCCESS)                                                      \
            return fail(PSFMC_EHIP, "%s failed: hipfftResult %d (%s:%d)", #expr,       \
                        (int)r_, __FILE__, __LINE__);                                  \
    } while (0)

#define RC_TRY(expr)                     \
    do {                                 \
        int rc_ = (expr);                \
        if (rc_ != PSFMC_OK) return rc_; \
    } while (0)

// the built sides, as the error messages list them (psfmc_sides.h: the one list everything here derives from)
#define PSFMC_SIDE_STR_(N, ...) " " #N
#define PSFMC_FUSED_SIDES PSFMC_SIDES(PSFMC_SIDE_STR_, PSFMC_SIDE_STR_)
#define PSFMC_UNKNOWN_SIDE(n) fail(PSFMC_EINVAL, "fused backend: side %d is not one of" PSFMC_FUSED_SIDES, n)

// Run BODY with `N_` a compile-time copy of the length n; in a split build only for this part's sides: side i of
// the list belongs to part i mod PSFMC_NPARTS, a side of another part answers PSFMC_NOT_MINE.  BODY sits in a generic
// lambda and the switch in a template on the part, so that a part instantiates the launchers -- hence the kernels --
// of its own sides only (in a plain function a discarded `if constexpr` branch is still instantiated).
template <int PART, class Body> static int dispatch_side(int n, Body& body) {
    switch (n) {
#define PSFMC_SIDE_CASE_(N, ...)                                                                                   \
    case N:                                                                                                        \
        if constexpr (fused_side_index(N) % PSFMC_NPARTS == PART) return body(std::integral_constant<int, N>{});  \
        else return PSFMC_NOT_MINE;
        PSFMC_SIDES(PSFMC_SIDE_CASE_, PSFMC_SIDE_CASE_)
#undef PSFMC_SIDE_CASE_
        default: return PSFMC_NPARTS == 1 ? PSFMC_UNKNOWN_SIDE(n) : PSFMC_NOT_MINE;
    }
}
#define DISPATCH_LEN(n, BODY)                                                                                    \
    do {                                                                                                         \
        auto body_ = [&](auto n_) -> int { constexpr int N_ = decltype(n_)::value; BODY; return PSFMC_OK; };     \
        const int rc_ = dispatch_side<PSFMC_PART>(n, body_);                                                     \
        if (rc_ != PSFMC_OK) return rc_;                                                                         \
    } while (0)

// the measured cost table has exactly the built sides, in their order
constexpr bool side_costs_match_sides() {
    if (sizeof(kSideCosts) / sizeof(kSideCosts[0]) != (size_t)kNumFusedSides) return false;
    for (int i = 0; i < kNumFusedSides; ++i)
        if (kSideCosts[i].side != kFusedSides[i]) return false;
    return true;
}
static_assert(side_costs_match_sides(), "psfmc_side_costs.h: regenerate it (tools/gen_side_costs.py) for the sides of psfmc_sides.h");

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
namespace psfmc { struct FieldAuxRecord; }   // psfmc_aux_table.h: complete in part 0, the only part that makes contexts
struct psfmc_ctx {
    int device = 0;
    int ny = 0, nx = 0, nxh = 0, S = 0, F = 0;
    int nyp = 0;                  // column length of the T layout: ny rounded up to whole row groups
    // An image side the transforms are not built for is EMBEDDED in a built side >= side + PSF side - 1
    // (psfmc_device.h WrapDesc): ny, nx above are then the TRANSFORM's sides, each field's wraps[f].ly, .lx its
    // image's; every pixel array that crosses the C ABI has its field's image shape, every internal one the
    // transform's.  The fields of one context may differ in image and PSF size: they share the transform.
    bool embed = false;           // some field's descriptor is not the identity
    std::vector<WrapDesc> wraps;  // [n_fields] each field's image inside the transform (identity: l = e = side, a = 0)
    WrapDesc* d_wrap = nullptr;   // [n_psf] the same per kernel spectrum (embedded contexts: walker_wrap)
    int n_psf = 0, n_ps = 0, n_sersic = 0;   // n_psf: kernel spectra in all (fields x PSFs per field)
    int n_fields = 1, n_psf_field = 0;       // observed fields of this context (psfmc_ctx_create_fields), PSFs of each
    size_t field_len = 0;                    // packed pixels (FieldPx) of one field
    int max_walkers = 0, chunk = 0, backend = 0;
    // the records now in d_prep have their power tables behind them (k_pow_tables ran); false: small batch,
    // the forward row waves form the entries they need themselves (psfmc_device.h raster_row)
    bool prep_tabs_built = false;
    // every writer of d_prep clears this, launch_pow_tables sets it: a forward launch that rasterises from
    // records whose table mode was not decided for THIS batch is an error, not wrong pixels
    bool prep_tabs_valid = false;
    // false: this context's rasterising kernels evaluate log2 + exp2 per pixel (row lengths up to 256:
    // psfmc_device.h pow_tabs_side) and nothing builds tables
    bool use_pow_tabs = true;
    int single_cap = 0;                               // walkers T buffer 0 holds (>= chunk)
    int rlen = 0, plen = 0;
    int nblk = 0;                 // chi^2 partial sums per walker
    hipStream_t stream = nullptr;
    // shared field arrays (SURVEY row Cfg)
    double *d_sci = nullptr, *d_var = nullptr;
    uint8_t* d_bad = nullptr;
    // per-call staging
    double *d_rows = nullptr, *d_prep = nullptr, *d_like = nullptr, *d_partial = nullptr;
    uint8_t* d_skip = nullptr;
    // hipFFT path
    double2 *d_pspec = nullptr, *d_vspec = nullptr;   // [n_psf][ny][nxh] == numpy rfft2
    double* d_real = nullptr;                         // [2*chunk][S]
    double2* d_spec = nullptr;                        // [2*chunk][F]
    std::map<int, std::pair<hipfftHandle, hipfftHandle>> plans;   // batch -> (D2Z, Z2D)
    hipfftHandle plan_fwd = 0, plan_inv = 0;                      // the pair in use
    // fused path
    // [chunk][nxh][ny/RG][2][RG] half-spectra of one pass; pass i uses buffer and
    // side stream i % n_streams so neighbouring passes overlap
    static constexpr int kMaxStreams = 4;
    cd* d_Ts[kMaxStreams] = {nullptr, nullptr, nullptr, nullptr};
    cd* d_T = nullptr;        // = d_Ts[0]
    hipStream_t side[kMaxStreams] = {nullptr, nullptr, nullptr, nullptr};   // side[0] unused
    hipEvent_t ev_fork = nullptr, ev_join[kMaxStreams] = {nullptr, nullptr, nullptr, nullptr};
    int n_streams = 2;
    int stagger = 0;          // the second lane starts one forward-row kernel late (run_pipeline); set per shape
    hipEvent_t ev_stagger[kMaxStreams] = {nullptr, nullptr, nullptr, nullptr};
    // "exclusive" kernels (set_option "exclusive", bit 0 forward rows, bit 1 columns, bit 2 inverse rows): a kernel of
    // that kind of pass i + 1 (the other lane) waits for the same kind of pass i, so that the two lanes never run two
    // like kernels side by side -- a VALU-bound forward kernel then always meets the other lane's memory-bound ones.
    // Measured (round 4, profiles/r4_exclusive.txt): SLOWER in every combination, 1024^2 50.3 k -> 43.7 ... 46.4 k
    // evals/s, 512^2 268 k -> 249 ... 266 k: the lanes spend half their time like against like by themselves
    // (profiles/r4_lane_timeline_*.txt: forward + forward alone 32 % of the wall time at 1024^2) and that is the
    // better state -- two forward launches side by side are three whole rounds of row waves.  Off.
    int exclusive = 0;
    hipEvent_t ev_excl[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    bool t_f32 = false;       // T stored as complex64 (set_option "storage_f32"); arithmetic stays fp64
    bool plain_shape = false; // both sides power-of-two shapes (what storage_f32 is built for)
    bool row_fast = false;    // nx a power-of-two shape and ny a whole number of its row workgroups
    // which row kernels are the one-row-per-wave three-stage ones (psfmc_rows3_path.h): both above 1024, the inverse
    // one at the sides of rows3_inv_default; PSFMC_ROWS3 = 1 / 0 in the environment forces every built one / none
    bool rows3_fwd = false, rows3_inv = false;
    long long speculated_runs = 0;   // psfmc_stretch_run calls that took the whole-iteration route
    int speculate = -1;       // device sampler: ensembles of up to 2 x this many walkers run ONE pipeline pass per iteration (0 = never, -1 = the default rule)
    int cols3 = 1;            // column kernel (set_option "cols3"; decided by col_engine alone): 0 the two-stage k_cols (sides <= 1024 only), 1 the defaults (k_cols3f at 512 / 1024 / 1536 / 2048, k_cols3g at the other sides of fft3g_pick), 2 k_cols3g at those four as well, 3 round 3's k_cols3 at 512 / 1024 (elsewhere as 2), 4 the same as 1; f32 storage takes k_cols3 at 512 / 1024 unless 0
    bool use_graph = false;   // psfmc_stretch_run replays a captured iteration (set_option "graph"; measured: no gain,
                              // the iteration is kernel-time- not launch-bound)
    long long graph_launches = 0;
    int min_split = 1 << 30;  // split a single-pass batch over both streams from this size (off: no gain measured)
    // optional per-kernel timing with HIP events (set_option "profile")
    bool profile = false;
    struct ProfRec { int kind; hipEvent_t a, b; };
    std::vector<ProfRec> prof_pending;
    double prof_ms[3] = {0, 0, 0};
    long prof_n[3] = {0, 0, 0};
    cd* d_Kraw = nullptr;     // [n_psf][2][nxh][ny] kernel spectra, unscaled
    cd* d_Kt = nullptr;       // same * (-1)^(kx+ky) / S
    cd *d_twx = nullptr, *d_twy = nullptr;            // exp(-2 pi i k/n) tables
    double* d_rho = nullptr;  // [n_psf] power-of-two scale of the variance channel
    FieldPx* d_field = nullptr;   // [S] {sci|NaN, obs_var} in rows_inv lane order
    int rg_log2 = 0;          // log2(rows per wave of the row kernels)
    double *d_img0 = nullptr, *d_img1 = nullptr;      // [chunk][S] staging for eval_images
    int img_cap = 0;
    // raw-vector path (psfmc_set_layout[_field]), [n_fields] each: a field's layout (the same structure for every
    // field, own priors / constants), whether it has been set, and the one allocation behind its pointers
    std::vector<ThetaLayout> layouts;
    std::vector<char> has_layout;
    std::vector<void*> layout_blobs;
    size_t theta_lds = 0;
    ThetaLayout* d_field_layouts = nullptr;  // [n_fields] device copies of the layouts (launches that span several fields)
    int* d_field_sides = nullptr;            // [n_fields][2] each field's image sides (ly, lx), for the same launches
    // joint fits (psfmc_set_joint_priors): one parameter vector per walker for every field
    struct Joint {
        bool ready = false;                  // set by psfmc_set_joint_priors, cleared by a new field layout
        ThetaLayout prior{};                 // the joint prior table (n_params columns, no slots)
        std::vector<ThetaLayout> fields;     // each field's layout with every prior column PRIOR_HOST
        std::vector<void*> blobs;            // [0]: the prior table's, [1 + f]: field f's copy of its layout blob
        ThetaLayout* d_fields = nullptr;     // device copies of `fields`
        double* d_lp = nullptr;              // [max_walkers] joint log-priors (k_joint_prior)
    } joint;
    double *d_theta = nullptr, *d_extra = nullptr, *d_lnprior = nullptr;
    double* d_acc = nullptr;  // [n_fields][4][S] sums: raw, conv, model variance, PS-only conv
    // fused path: samples are first added to three LINEAR sums per PSF -- raw, raw^2, PS-only raw --
    // (k_raster_sums) and convolved into d_acc only when the images are asked for (flush_linear_sums)
    double* d_lin = nullptr;      // [n_psf][3][S]
    double* d_linpart = nullptr;  // [lin_groups][n_psf][3][S] partial sums of one call
    int lin_groups = 0;
    long long lin_pending = 0;    // samples in d_lin not yet convolved into d_acc
    bool linear_acc = true;       // set_option "linear_accumulation" 0: every sample through the full pipeline (round 1's way)
    double* d_rawstage = nullptr;   // [img_cap][S] raw-model staging for the sums
    std::vector<long long> acc_count;   // [n_fields] samples in each field's sums
    int cols_grid = 0;
    // device-resident sampler state (psfmc_stretch_*): grow-only buffers
    struct Stretch {
        double *pos = nullptr, *lnp = nullptr, *q = nullptr, *newlnp = nullptr, *rand = nullptr;
        double *chain = nullptr, *lnchain = nullptr;
        int *partner = nullptr, *iter = nullptr;
        long long* nacc = nullptr;
        uint8_t* accflag = nullptr;        // whole-iteration launches: which first-half proposals were accepted
        size_t cap_acc = 0;
        bool spec = false;                 // this run proposes whole iterations (stretch_run_impl)
        size_t cap_pos = 0, cap_lnp = 0, cap_q = 0, cap_new = 0, cap_rand = 0, cap_chain = 0, cap_lnchain = 0,
               cap_partner = 0, cap_iter = 0, cap_nacc = 0;
        int W = 0, n_iter = 0;
        int F = 1;                // ensembles in the run (psfmc_stretch_run_fields: one per field)
        bool store = false, open = false;
        // proposal moves (psfmc_move_run, psfmc_stretch_set_moves): the move of every iteration and the DE
        // moves' second partner; `moves`: this run forms its proposals with k_move_propose
        int *kind = nullptr, *partner_b = nullptr;
        size_t cap_kind = 0, cap_pb = 0;
        bool moves = false;
    } stretch;
    // parallel-tempering state (psfmc_pt_run): one grow-only allocation carved per call
    unsigned char* pt_blob = nullptr;
    size_t pt_cap = 0;
    // pixel-integrated Sersic components (psfmc_set_sersic_integrate, psfmc_integrated.h); nothing is allocated and
    // no kernel changes until a flag is set
    bool integ_any = false;
    std::vector<uint8_t> integ_flags;    // [n_fields][n_sersic]
    uint8_t* d_integ_flags = nullptr;
    double* d_integ_par = nullptr;       // [max_walkers][n_sersic][9] the integrated components' real blocks
    // the walkers' EXTRA IMAGES, model coordinates: what the kernels of psfmc_integrated.h and psfmc_general.h
    // produce and the EXTRA instantiations of the rasterising kernels add (one buffer, any producer)
    double* d_extra_img = nullptr;       // [max_walkers][S]
    // auxiliary parameters, general Sersic components and tilted skies (psfmc_set_aux_layout, psfmc_general.h);
    // nothing is allocated and no kernel changes until a field registers an aux layout with a flag set
    bool gen_any = false;
    // doubles per walker of d_aux, the same for every field: the longest table a field of the context ever had
    // (apply_aux_record; 2 n_sky + n_sersic, + 12 / 18 / 20 / 24 / 28 n_sersic from the first modes / spiral / law /
    // truncation / bending on)
    int aux_stride = 0, aux_n_sky = 0;
    std::vector<uint8_t> gen_flags;      // [n_fields][n_sersic] general components, then [n_fields][n_sky] tilted skies
    uint8_t* d_gen_flags = nullptr;
    double* d_gen_par = nullptr;         // [max_walkers][n_sersic][kGenPar] the general components' real blocks
    double* d_aux = nullptr;             // [max_walkers][aux_stride]
    std::vector<void*> aux_blobs;        // [n_fields] the allocations behind the layouts' aux_col / aux_const
    // ties (psfmc_set_ties), [n_fields] each or empty (a context that never had a tie): src | ratio | offset columns,
    // ratio | offset constants and their device copy (konst, then col).  ties_live: what the field's layout points to;
    // ties_next: what psfmc_set_ties registered since (ties_dirty), made live by the field's next psfmc_set_layout --
    // a layout and the tables behind it always stand on the ties they were checked against.
    struct TieRecord {
        std::vector<int> col;
        std::vector<double> konst;
        int n = 0;
        void* blob = nullptr;
    };
    std::vector<TieRecord> ties_live, ties_next;
    std::vector<char> ties_dirty;
    // [n_fields] what each field registered (psfmc_set_layout's degrees, the arguments of psfmc_set_aux_layout and
    // of the three block layouts): apply_aux_record composes the field's table and mask rows from it
    std::vector<psfmc::FieldAuxRecord> aux_records;
    int aux_rows_w = -1;                 // walkers whose aux rows psfmc_set_aux_rows left in d_aux for the next row-based call
    int aux_base = 0;                    // 2 n_sky + n_sersic: the entries of psfmc_set_aux_layout, in front of the blocks
    // [kAuxBlocks] the blocks behind them, in table order (psfmc_aux_table.h kAuxBlock: Fourier modes, spiral arms,
    // radial laws, truncations, bending modes; psfmc_set_<name>_layout, psfmc_general.h).  Nothing is allocated and no kernel changes
    // until a field registers a block.  The first registration of block b allocates the masks and per-walker
    // constants, all clear, of blocks kAuxBlock[b].first ... b -- a law, a truncation or bending those of every block
    // before it, a spiral only its own -- and aux_stride grows to the end of block b in a walker's vector (aux_base +
    // 12 / 18 / 20 / 24 / 28 n_sersic): a block's entries sit behind those of every block before it, zeros or padding where no
    // field has them.  `any` follows the fields' registrations; general_launch reads what a launch carries from it.
    struct AuxBlockState {
        bool any = false;                // some field has the block registered now
        std::vector<uint8_t> masks;      // [n_fields][n_sersic] mask bytes; empty until the context meets the block
        uint8_t* d_masks = nullptr;
        double* d_par = nullptr;         // [max_walkers][n_sersic][kAuxBlock[b].par] (+ 1)
    };
    std::vector<AuxBlockState> blk;      // (sized at creation, like aux_records: kAuxBlocks is part 0's to know)
    // general components rendered as the mean over each pixel (psfmc_set_general_mean, psfmc_general_mean.h): flags
    // only, no per-walker entries; nothing is allocated, nothing more is launched and every kernel gets the arguments
    // it got until a field registers a flag
    bool mean_any = false;
    std::vector<uint8_t> mean_flags;     // [n_fields][n_sersic]
    // [n_fields][n_sersic] the flags, then [n_fields][n_sersic] the general flags with the mean components cleared
    // (what k_general_rows reads in a context with mean components)
    uint8_t* d_mean_flags = nullptr;
    // psfmc_fisher_rows (psfmc_fisher.h): the stencil walkers' stashed images, the Gram kernel's partial tiles and the
    // step reciprocals / results; grow-only, nothing is allocated until the first call
    // psfmc_fisher_rows_fields / _joint add the stencils' table, the joint column map and the linked results, on
    // their first call
    struct Fisher {
        double *stash = nullptr, *partial = nullptr, *io = nullptr;
        size_t cap_stash = 0, cap_partial = 0, cap_io = 0;
        FisherFieldRec* recs = nullptr;
        int* field_col = nullptr;
        double* link = nullptr;
        size_t cap_recs = 0, cap_field_col = 0, cap_link = 0;
    } fisher;
};

// the extra image of the walker whose record `prep` points at (nullptr: none to add)
static const double* extra_image_of(const psfmc_ctx* c, const double* prep) {
    if ((!c->integ_any && !c->gen_any) || !prep) return nullptr;
    return c->d_extra_img + (size_t)((prep - c->d_prep) / c->plen) * c->S;
}

// a field's image window inside the transform-shaped pixel arrays (all of them unless the image is embedded)
static ImgWindow img_window(const psfmc_ctx* c, int field) {
    const WrapDesc& w = c->wraps[field];
    return ImgWindow{c->nx, w.ly, w.lx, w.ay, w.ax};
}
// pixels of a field's own image (the shape of its arrays at the C ABI)
static size_t img_pixels(const psfmc_ctx* c, int field) { return (size_t)c->wraps[field].ly * c->wraps[field].lx; }

// per-side constants of the row kernels
struct RowShape { int rg, fast_waves, fast_rg_log2, regs; bool plain; };

// ---------------------------------------------------------------------------
// fused path launchers
// ---------------------------------------------------------------------------
// Which kernel a launch takes is decided ONCE, by the three constexpr choice functions below (column engine,
// forward rows, inverse rows): the launchers switch on their answers and psfmc_get_option reports them
// ("column_engine", "raster_group").  A new kernel family goes into its choice function and its launcher's switch.
// f32: the T element type is cf (complex64 STORAGE, set_option "storage_f32"; built for the power-of-two shapes
// only) instead of cd (complex128)
template <int N> constexpr bool plain_side() {
    if constexpr (two_stage_side(N)) return FftShape<N>::kPlain;
    else return false;
}
template <int N> constexpr bool storage_built(bool f32) { return !f32 || plain_side<N>(); }

// the launch-relevant facts of a context.  t_f32 is the storage of THIS launch: the context's for a batch of walkers,
// complex128 for the kernel spectra at set-up and for the convolution of the posterior sums
struct LaunchFacts {
    int cols3, rg_log2;
    bool t_f32, embed, rows3_fwd, rows3_inv, row_fast, multi;      // multi: n_fields > 1
};
static LaunchFacts launch_facts(const psfmc_ctx* c, bool t_f32) {
    return LaunchFacts{c->cols3, c->rg_log2, t_f32, c->embed, c->rows3_fwd, c->rows3_inv, c->row_fast, c->n_fields > 1};
}

// what a choice answers instead of a kernel, and the launcher returns
enum Refusal { REFUSE_NOT, REFUSE_F32_SIDE, REFUSE_F32_GUARDED, REFUSE_F32_EMBED, REFUSE_F32_FIELDS, REFUSE_NO_ROWS3,
               REFUSE_COLS3_ONLY };
static int refuse(Refusal why, int side) {
    switch (why) {
        case REFUSE_F32_SIDE: return fail(PSFMC_EINVAL, "single-precision storage is built for power-of-two sides only");
        case REFUSE_F32_GUARDED: return fail(PSFMC_EINVAL, "single-precision storage needs the unguarded row kernels");
        case REFUSE_F32_EMBED: return fail(PSFMC_EINVAL, "single-precision storage does not serve embedded images");
        case REFUSE_F32_FIELDS: return fail(PSFMC_EINVAL, "single-precision storage serves contexts of one field");
        case REFUSE_NO_ROWS3: return fail(PSFMC_EINVAL, "side %d has no three-stage row kernels", side);
        case REFUSE_COLS3_ONLY:
            return fail(PSFMC_EINVAL, "side %d has only the three-stage column kernel (option cols3 = 0 and row groups "
                        "other than 4 do not apply)", side);
        case REFUSE_NOT: break;
    }
    return fail(PSFMC_EINVAL, "internal: side %d was chosen a kernel it is not built with", side);
}

// ---- the column engine; the values are what get_option("column_engine") reports ----
enum ColEngine { COL_REFUSED = -1, COL_COLS = 0, COL_COLS3 = 1, COL_COLS3G = 2, COL_COLS3F = 3 };
// whether side NY has the engine for this storage: what the choice may answer, and what launch_cols instantiates
template <int NY> constexpr bool col_engine_built(ColEngine e, bool f32) {
    switch (e) {
        case COL_COLS: return two_stage_side(NY);
        case COL_COLS3: return NY == 512 || NY == 1024;                       // long power-of-two columns, wave-wide
        case COL_COLS3G: return cols3g_side<NY>() && !f32;                    // the sides of psfmc_fft.h fft3g_pick
        case COL_COLS3F: return cols3f_shape<Fft3gShape<NY>>() && !f32;       // ny = 8 m x 64: 512, 1024, 1536, 2048
        default: return false;
    }
}
template <int NY> constexpr ColEngine col_engine(const LaunchFacts& f) {
    // k_cols3f: the general three-stage engine run forward both ways (round 4).
    // In the flow (same box, whole step): 512^2 +1.6 %, 1536^2 +18 %, 2048^2 +2 % (+5.4 % more with its load
    // pipeline, cols3f_prefetch); at 1024 its third wave per SIMD measured SLOWER than k_cols3 (57.5 vs 52.7 us
    // per 6-walker pass, step -0.8 %: 6 MB of columns in flight per XCD against a 4-MiB L2 that also has to hold
    // the kernel-spectrum columns), with the load pipeline at two waves per SIMD it is the faster one (51.4 vs
    // 52.6 us in the flow, step +0.5 %).  cols3 = 3 asks for k_cols3 at 512 / 1024; f32 storage takes it whenever
    // cols3 is not 0
    if (col_engine_built<NY>(COL_COLS3F, f.t_f32) && (f.cols3 == 1 || f.cols3 == 4)) return COL_COLS3F;
    if (col_engine_built<NY>(COL_COLS3, f.t_f32) && (f.cols3 == 3 || (f.cols3 && f.t_f32))) return COL_COLS3;
    // (so cols3 = 3 acts as 2 away from 512 / 1024); a row group the engine's layout does not serve falls back
    if (col_engine_built<NY>(COL_COLS3G, f.t_f32) && f.cols3 && cols3g_layout_ok<Fft3gShape<NY>>(f.rg_log2))
        return COL_COLS3G;
    return col_engine_built<NY>(COL_COLS, f.t_f32) ? COL_COLS : COL_REFUSED;
}

// ---- the row kernels ----
// ROWS3: one row per wave, three stages (psfmc_rows3_path.h); ROWS2_*: the two-stage kernels of psfmc_fused_path.h,
// FAST the unguarded power-of-two ones (ny a whole number of their workgroups), GUARDED the general code path of
// the same shape
enum RowFamily { ROWS_REFUSED, ROWS3, ROWS2_FAST, ROWS2_GUARDED };
struct RowChoice {
    RowFamily family;
    bool flag;          // forward: WRAP, the rasteriser wraps its coordinates; inverse: MULTI, chi^2 summed per field
    Refusal why;
};
constexpr RowChoice row_refused(Refusal why) { return RowChoice{ROWS_REFUSED, false, why}; }
// whether side NX has the family's forward / inverse kernel for this storage, and the kernel with the flag set: what
// the choices may answer, and what the launchers instantiate
template <int NX> constexpr bool row_family_built(RowFamily fam, bool f32, bool forward) {
    switch (fam) {
        case ROWS3: return !f32 && (forward ? rows3_fwd_built(NX) : rows3_side<NX>());
        case ROWS2_FAST: return plain_side<NX>();
        case ROWS2_GUARDED: return two_stage_side(NX) && !f32;
        default: return false;
    }
}
// WRAP: records rasterised into complex128 storage (images from memory -- the PSF canvases at set-up, the posterior
// sums -- are in transform coordinates already)
constexpr bool wrap_built(bool from_image, bool f32) { return !from_image && !f32; }
// MULTI: every three-stage side; on the two-stage kernels from 1024 with complex128 storage (below, one text tells
// the fields apart at run time)
template <int NX> constexpr bool multi_built(RowFamily fam, bool f32) { return fam == ROWS3 || (!f32 && NX >= 1024); }

template <int NX> constexpr RowChoice rows_fwd_choice(const LaunchFacts& f, bool from_image) {
    if (!storage_built<NX>(f.t_f32)) return row_refused(REFUSE_F32_SIDE);
    const bool wrap = !from_image && f.embed;              // the rasteriser of an embedded image wraps its coordinates
    if (!two_stage_side(NX) || (f.rows3_fwd && !f.t_f32))
        return row_family_built<NX>(ROWS3, f.t_f32, true) ? RowChoice{ROWS3, wrap, REFUSE_NOT} : row_refused(REFUSE_NO_ROWS3);
    const bool fast = plain_side<NX>() && f.row_fast;
    if (f.t_f32 && !fast) return row_refused(REFUSE_F32_GUARDED);
    if (wrap && !wrap_built(from_image, f.t_f32)) return row_refused(REFUSE_F32_EMBED);
    return RowChoice{fast ? ROWS2_FAST : ROWS2_GUARDED, wrap, REFUSE_NOT};
}
template <int NX> constexpr RowChoice rows_inv_choice(const LaunchFacts& f) {
    if (!storage_built<NX>(f.t_f32)) return row_refused(REFUSE_F32_SIDE);
    if (!two_stage_side(NX) || (f.rows3_inv && !f.t_f32))
        return row_family_built<NX>(ROWS3, f.t_f32, false) ? RowChoice{ROWS3, f.multi, REFUSE_NOT} : row_refused(REFUSE_NO_ROWS3);
    const bool fast = plain_side<NX>() && f.row_fast;
    if (f.t_f32 && !fast) return row_refused(REFUSE_F32_GUARDED);
    if (f.t_f32 && f.multi) return row_refused(REFUSE_F32_FIELDS);
    const RowFamily fam = fast ? ROWS2_FAST : ROWS2_GUARDED;
    return RowChoice{fam, f.multi && multi_built<NX>(fam, f.t_f32), REFUSE_NOT};
}
// the G of the raster_row the chosen forward kernel runs (get_option("raster_group")); 0: log2 + exp2 per pixel
template <int NX> constexpr int raster_group_of(const RowChoice& ch) {
    if constexpr (two_stage_side(NX)) {
        if (ch.family == ROWS2_FAST || ch.family == ROWS2_GUARDED)
            return ch.flag ? fwd_raster_group<NX, true>() : fwd_raster_group<NX, false>();
    }
    return rows3_raster_group(ch.flag);
}

// The choices pinned to the literal values the device tests assert through get_option (tests/test_gpu_variants.py
// COLUMN_CASES, the raster-form table of tests/helpers.py): rows of 64 pixels come in groups of 8, of 96 / 100 in
// groups of 4 (of 1024 in groups of 2)
constexpr LaunchFacts col_facts(int cols3, int row_group, bool f32 = false) {
    return LaunchFacts{cols3, row_group == 8 ? 3 : row_group == 4 ? 2 : 1, f32, false, false, false, true, false};
}
#define PSFMC_PIN_COLS(NY, cols3, engine) \
    static_assert(col_engine<NY>(col_facts(cols3, 4)) == engine && col_engine<NY>(col_facts(cols3, 8)) == engine, #NY " " #cols3)
PSFMC_PIN_COLS(512, 0, COL_COLS);   PSFMC_PIN_COLS(512, 1, COL_COLS3F);  PSFMC_PIN_COLS(512, 2, COL_COLS3G);
PSFMC_PIN_COLS(512, 3, COL_COLS3);  PSFMC_PIN_COLS(512, 4, COL_COLS3F);
PSFMC_PIN_COLS(1024, 0, COL_COLS);  PSFMC_PIN_COLS(1024, 1, COL_COLS3F); PSFMC_PIN_COLS(1024, 2, COL_COLS3G);
PSFMC_PIN_COLS(1024, 3, COL_COLS3); PSFMC_PIN_COLS(1024, 4, COL_COLS3F);
PSFMC_PIN_COLS(1536, 1, COL_COLS3F); PSFMC_PIN_COLS(1536, 2, COL_COLS3G); PSFMC_PIN_COLS(1536, 3, COL_COLS3G);
PSFMC_PIN_COLS(1536, 4, COL_COLS3F); PSFMC_PIN_COLS(2048, 2, COL_COLS3G);
PSFMC_PIN_COLS(384, 0, COL_COLS);   PSFMC_PIN_COLS(500, 0, COL_COLS);    PSFMC_PIN_COLS(640, 0, COL_COLS);
PSFMC_PIN_COLS(900, 0, COL_COLS);   PSFMC_PIN_COLS(384, 1, COL_COLS3G);
#undef PSFMC_PIN_COLS
// 520 = 10 x 52: k_cols3g's L = 52 lanes are a multiple of 4 but not of 8 (cols3g_layout_ok)
static_assert(col_engine<520>(col_facts(1, 4)) == COL_COLS3G && col_engine<520>(col_facts(2, 4)) == COL_COLS3G);
static_assert(col_engine<520>(col_facts(1, 8)) == COL_COLS && col_engine<520>(col_facts(2, 8)) == COL_COLS);
// f32 storage: k_cols3 whenever cols3 is not 0
static_assert(col_engine<512>(col_facts(1, 8, true)) == COL_COLS3 && col_engine<512>(col_facts(1, 4, true)) == COL_COLS3 &&
              col_engine<1024>(col_facts(2, 8, true)) == COL_COLS3 && col_engine<512>(col_facts(0, 4, true)) == COL_COLS &&
              col_engine<128>(col_facts(1, 2, true)) == COL_COLS);
// the transform of an embedded 530-pixel image; no engine: cols3 = 0 above 1024 (set_option refuses it there)
static_assert(col_engine<576>(col_facts(1, 4)) == COL_COLS3G && col_engine<576>(col_facts(0, 4)) == COL_COLS &&
              col_engine<1152>(col_facts(1, 4)) == COL_COLS3G && col_engine<1536>(col_facts(0, 4)) == COL_REFUSED);
// the raster group (embedded: WRAP): an image of 170 pixels is embedded in 192, one of 270 in 294, one of 1100 in 1152
template <int NX> constexpr int raster_group_pin(bool embed) {
    return raster_group_of<NX>(rows_fwd_choice<NX>(LaunchFacts{1, 2, false, embed, !two_stage_side(NX), !two_stage_side(NX),
                                                               false, false}, false));
}
static_assert(raster_group_pin<64>(false) == 0 && raster_group_pin<256>(false) == 0 && raster_group_pin<264>(false) == 1 &&
              raster_group_pin<288>(false) == 4 && raster_group_pin<512>(false) == 2 && raster_group_pin<1152>(false) == 1);
static_assert(raster_group_pin<1152>(true) == 1 && raster_group_pin<294>(true) == 1 && raster_group_pin<192>(true) == 0);
// MULTI and WRAP where they apply, and the refusal of several fields in f32 storage
static_assert(rows_inv_choice<64>(LaunchFacts{1, 3, true, false, false, false, true, true}).why == REFUSE_F32_FIELDS &&
              !rows_inv_choice<512>(LaunchFacts{1, 2, false, false, false, false, true, true}).flag &&
              rows_inv_choice<1024>(LaunchFacts{1, 1, false, false, false, false, true, true}).flag &&
              rows_inv_choice<676>(LaunchFacts{1, 2, false, false, false, true, false, true}).flag &&
              rows_inv_choice<676>(LaunchFacts{1, 2, false, false, false, true, false, true}).family == ROWS3 &&
              rows_fwd_choice<676>(LaunchFacts{1, 2, false, false, false, true, false, true}, false).family == ROWS2_GUARDED &&
              !rows_fwd_choice<576>(LaunchFacts{1, 2, false, true, false, false, false, false}, true).flag);

// per-side answers about the row kernels, and everything a size-erased call carries (below)
struct RowFamilies { bool two_stage, rows3_inv, rows3_fwd, rows3_inv_default; };
struct SizeCall {
    psfmc_ctx* c = nullptr;
    int n = 0;                              // walkers
    const double* prep = nullptr;
    const uint8_t* skip = nullptr;
    void* T = nullptr;
    int ps_only = 0;
    const double *img = nullptr, *img_scale = nullptr;
    double *raw_out = nullptr, *partial = nullptr, *conv_out = nullptr, *var_out = nullptr;
    hipStream_t st = nullptr;
    bool from_image = false, convolve = true, f32 = false, rows3 = false;
    int field = 0, groups = 0, group_size = 0, ny = 0, per_field = 0;
    RowShape* shape = nullptr;
    RowFamilies* families = nullptr;
    size_t* len = nullptr;
    int* code = nullptr;
};

// ---- one launch body per direction ----
// raise kernel K's dynamic-LDS limit once per device (and thread) where it asks for more than every launch's 64 KiB
template <auto K, size_t LDS> static int raise_lds_limit(const psfmc_ctx* c) {
    if constexpr (LDS > 64 * 1024) {
        static thread_local int attr_device = -1;
        if (attr_device != c->device) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)LDS));
            attr_device = c->device;
        }
    }
    return PSFMC_OK;
}
// a row family's kernels for the template flags, its LDS bytes, block size and grid.x
template <int NX> struct Rows3Family {
    using S = typename Rows3<NX>::S;
    static constexpr RowFamily kFamily = ROWS3;
    static constexpr size_t kLds = rows3_lds_bytes<S>();
    static constexpr int kThreads = rows3_threads(NX);
    template <bool FROM_IMAGE, bool WRAP, bool EXTRA, typename TS> static constexpr auto fwd() {
        return &k_rows3_fwd<NX, FROM_IMAGE, WRAP, S, EXTRA>;
    }
    template <bool MULTI, typename TS> static constexpr auto inv() { return &k_rows3_inv<NX, MULTI>; }
    static int grid_x(const psfmc_ctx* c) { return (c->ny + rows3_waves(NX) - 1) / rows3_waves(NX); }
};
template <int NX, bool FAST> struct Rows2Family {
    static constexpr RowFamily kFamily = FAST ? ROWS2_FAST : ROWS2_GUARDED;
    static constexpr size_t kLds = fused_row_lds_bytes<NX, FAST>();
    static constexpr int kThreads = row_threads<NX, FAST>();
    template <bool FROM_IMAGE, bool WRAP, bool EXTRA, typename TS> static constexpr auto fwd() {
        return &k_rows_fwd<NX, FROM_IMAGE, TS, FAST, WRAP, EXTRA>;
    }
    template <bool MULTI, typename TS> static constexpr auto inv() { return &k_rows_inv<NX, TS, FAST, MULTI>; }
    static int grid_x(const psfmc_ctx* c) { return (c->nblk + row_waves<NX, FAST>() - 1) / row_waves<NX, FAST>(); }
};
// `launch` on the chosen family's traits: the choice's run-time answer as a template argument.  A family the side is
// not built with for this storage (forward or inverse kernel) is never named
template <int NX, bool F32, bool FORWARD, class Launch> static int with_row_family(const RowChoice& ch, Launch launch) {
    switch (ch.family) {
        case ROWS3:
            if constexpr (row_family_built<NX>(ROWS3, F32, FORWARD)) return launch(Rows3Family<NX>{});
            break;
        case ROWS2_FAST:
            if constexpr (row_family_built<NX>(ROWS2_FAST, F32, FORWARD)) return launch(Rows2Family<NX, true>{});
            break;
        case ROWS2_GUARDED:
            if constexpr (row_family_built<NX>(ROWS2_GUARDED, F32, FORWARD)) return launch(Rows2Family<NX, false>{});
            break;
        case ROWS_REFUSED: break;
    }
    return refuse(ch.why, NX);
}

template <class Fam, bool FROM_IMAGE, bool WRAP, typename TS, bool EXTRA = false>
static int launch_fwd_kernel(const SizeCall& a, const double* img) {
    psfmc_ctx* c = a.c;
    if constexpr (!FROM_IMAGE && !EXTRA) {
        // pixel-integrated components: the same kernel with their image added (its own instantiation)
        if (const double* extra = a.ps_only ? nullptr : extra_image_of(c, a.prep))
            return launch_fwd_kernel<Fam, false, WRAP, TS, true>(a, extra);
    }
    constexpr auto K = Fam::template fwd<FROM_IMAGE, WRAP, EXTRA, TS>();
    RC_TRY((raise_lds_limit<K, Fam::kLds>(c)));
    if (!FROM_IMAGE && !c->prep_tabs_valid)
        return fail(PSFMC_EINVAL, "internal: forward rows launched on prep records without a power-table decision");
    hipLaunchKernelGGL(K, dim3(Fam::grid_x(c), a.n), dim3(Fam::kThreads), Fam::kLds, a.st, a.prep, a.skip, c->d_twx,
                       static_cast<TS*>(a.T), c->n_ps, c->n_sersic, c->ny, a.ps_only, img, a.img_scale, a.raw_out,
                       c->d_wrap, c->prep_tabs_built ? kPowTabsBuilt : kPowTabsInWave);
    return PSFMC_OK;
}
template <int NX, bool FROM_IMAGE, typename TS = cd> static int launch_rows_fwd(const SizeCall& a) {
    constexpr bool F32 = sizeof(TS) != sizeof(cd);
    const RowChoice ch = rows_fwd_choice<NX>(launch_facts(a.c, F32), FROM_IMAGE);
    return with_row_family<NX, F32, true>(ch, [&](auto fam) -> int {
        using Fam = decltype(fam);
        if constexpr (wrap_built(FROM_IMAGE, F32))
            if (ch.flag) return launch_fwd_kernel<Fam, FROM_IMAGE, true, TS>(a, a.img);
        return launch_fwd_kernel<Fam, FROM_IMAGE, false, TS>(a, a.img);
    });
}

template <class Fam, bool MULTI, typename TS> static int launch_inv_kernel(const SizeCall& a) {
    psfmc_ctx* c = a.c;
    constexpr auto K = Fam::template inv<MULTI, TS>();
    RC_TRY((raise_lds_limit<K, Fam::kLds>(c)));
    hipLaunchKernelGGL(K, dim3(Fam::grid_x(c), a.n), dim3(Fam::kThreads), Fam::kLds, a.st, static_cast<const TS*>(a.T),
                       a.skip, c->d_twx, c->d_field, a.partial, c->ny, a.prep, c->plen, a.conv_out, a.var_out,
                       c->n_fields > 1 ? c->n_psf_field : 0, (unsigned)c->field_len);
    return PSFMC_OK;
}
template <int NX, typename TS = cd> static int launch_rows_inv(const SizeCall& a) {
    constexpr bool F32 = sizeof(TS) != sizeof(cd);
    const RowChoice ch = rows_inv_choice<NX>(launch_facts(a.c, F32));
    return with_row_family<NX, F32, false>(ch, [&](auto fam) -> int {
        using Fam = decltype(fam);
        if constexpr (multi_built<NX>(Fam::kFamily, F32))
            if (ch.flag) return launch_inv_kernel<Fam, true, TS>(a);
        return launch_inv_kernel<Fam, false, TS>(a);
    });
}

// the grid of the wave-wide column kernels: a wave per column, per_block of them in a workgroup
static int cols3_grid(const psfmc_ctx* c, int n_cols, int per_block) {
    const int blocks = (n_cols + per_block - 1) / per_block;
    return blocks < 4 * c->cols_grid ? blocks : 4 * c->cols_grid;
}
template <auto K, size_t LDS, typename TS> static int launch_col_kernel(const SizeCall& a, int grid, int threads) {
    psfmc_ctx* c = a.c;
    RC_TRY((raise_lds_limit<K, LDS>(c)));
    hipLaunchKernelGGL(K, dim3(grid), dim3(threads), LDS, a.st, static_cast<TS*>(a.T), c->d_Kt, a.prep, a.skip, c->d_twy,
                       c->plen, c->nxh, a.n, c->rg_log2);
    return PSFMC_OK;
}
template <int NY, bool CONVOLVE, typename TS = cd> static int launch_cols(const SizeCall& a) {
    constexpr bool F32 = sizeof(TS) != sizeof(cd);
    if constexpr (!storage_built<NY>(F32)) {
        return refuse(REFUSE_F32_SIDE, NY);
    } else {
        psfmc_ctx* c = a.c;
        using S3 = Fft3gShape<NY>;
        const int n_cols = a.n * 2 * c->nxh;
        switch (col_engine<NY>(launch_facts(c, F32))) {
            case COL_COLS3F:
                if constexpr (col_engine_built<NY>(COL_COLS3F, F32))
                    return launch_col_kernel<&k_cols3f<NY, CONVOLVE>, fused_col3f_lds_bytes<S3>(), TS>(
                        a, cols3_grid(c, n_cols, cols3f_waves<S3>()), cols3f_threads<S3>());
                break;
            case COL_COLS3:
                if constexpr (col_engine_built<NY>(COL_COLS3, F32))
                    return launch_col_kernel<&k_cols3<NY, CONVOLVE, TS>, fused_col3_lds_bytes<NY>(), TS>(
                        a, cols3_grid(c, n_cols, kColThreads / 64), kColThreads);
                break;
            case COL_COLS3G:
                if constexpr (col_engine_built<NY>(COL_COLS3G, F32))
                    return launch_col_kernel<&k_cols3g<NY, CONVOLVE>, fused_col3g_lds_bytes<S3>(), TS>(
                        a, cols3_grid(c, n_cols, cols3g_waves<S3>()), cols3g_threads<S3>());
                break;
            case COL_COLS:                  // persistent: a workgroup takes col_ffts_per_block columns at a time
                if constexpr (col_engine_built<NY>(COL_COLS, F32)) {
                    const int groups = (n_cols + col_ffts_per_block<NY>() - 1) / col_ffts_per_block<NY>();
                    return launch_col_kernel<&k_cols<NY, CONVOLVE, TS>, fused_col_lds_bytes<NY>(), TS>(
                        a, groups < c->cols_grid ? groups : c->cols_grid, kColThreads);
                }
                break;
            case COL_REFUSED: break;
        }
        return refuse(REFUSE_COLS3_ONLY, NY);
    }
}

template <int NX> static int pack_field(psfmc_ctx* c, int f) {
    const size_t px = (size_t)f * c->S;
    if constexpr (rows3_side<NX>()) {
        if (c->rows3_inv) {
            hipLaunchKernelGGL((k_pack_field3<NX>), dim3(256), dim3(256), 0, c->stream, c->d_sci + px, c->d_var + px,
                               c->d_bad + px, c->d_field + (size_t)f * c->field_len, c->ny);
            return PSFMC_OK;
        }
    }
    if constexpr (two_stage_side(NX)) {
        hipLaunchKernelGGL((k_pack_field<NX>), dim3(256), dim3(256), 0, c->stream, c->d_sci + px, c->d_var + px,
                           c->d_bad + px, c->d_field + (size_t)f * c->field_len, c->ny);
        return PSFMC_OK;
    } else {
        return fail(PSFMC_EINVAL, "side %d needs the three-stage row kernels", NX);
    }
}
// per-side constants of the row kernels the context will launch (rows3: the three-stage family)
template <int NX> static RowShape row_shape_of(bool rows3) {
    if constexpr (rows3_side<NX>()) {
        if (rows3 || !two_stage_side(NX)) return RowShape{1, rows3_waves(NX), rows3_rg_log2(NX), Rows3<NX>::S::R1, false};
    }
    if constexpr (two_stage_side(NX))
        return RowShape{row_group<NX>(), row_waves<NX, true>(), layout_rg_log2<NX, true>(), FftShape<NX>::R,
                        FftShape<NX>::kPlain};
    else
        return RowShape{1, rows3_waves(NX), rows3_rg_log2(NX), 0, false};
}
// which row kernels the side is built with: a two-stage family, the three-stage inverse kernel, the forward one, and
// whether the three-stage inverse kernel is the default
template <int NX> constexpr RowFamilies row_families() {
    return RowFamilies{two_stage_side(NX), rows3_side<NX>(), rows3_fwd_built(NX), rows3_side<NX>() && rows3_inv_default(NX)};
}
template <int NX> static size_t field_len_of(int ny, bool rows3) {
    if constexpr (rows3_side<NX>()) {
        if (rows3 || !two_stage_side(NX)) return rows3_field_len<NX>(ny);
    }
    if constexpr (two_stage_side(NX)) return fused_field_len<NX>(ny);
    else return 0;
}

// one launch: the kernel is chosen by WRAP (an embedded image) and EXTRA (pixel-integrated components: their image
// is added, one more argument)
template <int NX> static int launch_raster_sums(const SizeCall& a) {
    psfmc_ctx* c = a.c;
    constexpr int RG = RasterShape<NX>::TPW;
    auto launch = [&](auto kernel, auto... extra) {
        hipLaunchKernelGGL(kernel, dim3((c->ny + RG - 1) / RG, a.groups), dim3(64), 0, a.st, a.prep, c->plen, a.n,
                           a.group_size, c->n_ps, c->n_sersic, c->ny, c->n_psf, c->d_linpart, a.per_field, a.field,
                           c->n_psf_field, c->d_wrap, extra...);
    };
    if (const double* extra = extra_image_of(c, a.prep))
        launch(c->embed ? &k_raster_sums_extra<NX, true> : &k_raster_sums_extra<NX, false>, extra);
    else
        launch(c->embed ? &k_raster_sums<NX, true> : &k_raster_sums<NX, false>);
    return PSFMC_OK;
}


// ---------------------------------------------------------------------------
// size-erased entry to the per-side launchers: what crosses the boundary between the parts
// ---------------------------------------------------------------------------
enum SizeOp { SZ_ROW_SHAPE, SZ_FIELD_LEN, SZ_PACK_FIELD, SZ_ROWS_FWD, SZ_COLS, SZ_ROWS_INV, SZ_RASTER_SUMS, SZ_COL_ENGINE, SZ_RASTER_GROUP };

static int size_call_here(int op, int side, SizeCall& a) {
    psfmc_ctx* c = a.c;
    switch (op) {
        case SZ_ROW_SHAPE:
            // (a.rows3: the caller asks for the three-stage row family where the side has both)
            DISPATCH_LEN(side, (*a.shape = row_shape_of<N_>(a.rows3), *a.families = row_families<N_>()));
            return PSFMC_OK;
        case SZ_FIELD_LEN:
            DISPATCH_LEN(side, *a.len = field_len_of<N_>(a.ny, a.rows3));
            return PSFMC_OK;
        case SZ_PACK_FIELD:
            DISPATCH_LEN(side, RC_TRY(pack_field<N_>(c, a.field)));
            return PSFMC_OK;
        case SZ_ROWS_FWD:
            if (a.from_image) {
                DISPATCH_LEN(side, RC_TRY((launch_rows_fwd<N_, true>(a))));
            } else if (a.f32) {
                DISPATCH_LEN(side, RC_TRY((launch_rows_fwd<N_, false, cf>(a))));
            } else {
                DISPATCH_LEN(side, RC_TRY((launch_rows_fwd<N_, false>(a))));
            }
            return PSFMC_OK;
        case SZ_COLS:
            if (!a.convolve) {
                DISPATCH_LEN(side, RC_TRY((launch_cols<N_, false>(a))));
            } else if (a.f32) {
                DISPATCH_LEN(side, RC_TRY((launch_cols<N_, true, cf>(a))));
            } else {
                DISPATCH_LEN(side, RC_TRY((launch_cols<N_, true>(a))));
            }
            return PSFMC_OK;
        case SZ_ROWS_INV:
            if (a.f32) {
                DISPATCH_LEN(side, RC_TRY((launch_rows_inv<N_, cf>(a))));
            } else {
                DISPATCH_LEN(side, RC_TRY((launch_rows_inv<N_>(a))));
            }
            return PSFMC_OK;
        case SZ_RASTER_SUMS:
            DISPATCH_LEN(side, RC_TRY(launch_raster_sums<N_>(a)));
            return PSFMC_OK;
        // what get_option reports: the choices' answers for the context's own storage (no column engine: 0, as ever)
        case SZ_COL_ENGINE:
            DISPATCH_LEN(side, *a.code = std::max<int>(COL_COLS, col_engine<N_>(launch_facts(c, c->t_f32))));
            return PSFMC_OK;
        case SZ_RASTER_GROUP:
            DISPATCH_LEN(side, *a.code = raster_group_of<N_>(rows_fwd_choice<N_>(launch_facts(c, c->t_f32), false)));
            return PSFMC_OK;
    }
    return fail(PSFMC_EINVAL, "unknown size operation %d", op);
}

#define PSFMC_PART_FN_(k) psfmc_size_call_part##k
#define PSFMC_PART_FN(k) PSFMC_PART_FN_(k)
int psfmc_size_call_part0(int op, int side, void* args);
#if PSFMC_NPARTS > 1
int psfmc_size_call_part1(int op, int side, void* args);
int psfmc_size_call_part2(int op, int side, void* args);
int psfmc_size_call_part3(int op, int side, void* args);
#endif
int PSFMC_PART_FN(PSFMC_PART)(int op, int side, void* args) { return size_call_here(op, side, *static_cast<SizeCall*>(args)); }

#if PSFMC_PART == 0
static int size_call(int op, int side, SizeCall& a) {
#if PSFMC_NPARTS == 1
    return size_call_here(op, side, a);
#else
    int (*const parts[])(int, int, void*) = {psfmc_size_call_part0, psfmc_size_call_part1, psfmc_size_call_part2,
                                             psfmc_size_call_part3};
    for (auto fn : parts) {
        const int rc = fn(op, side, &a);
        if (rc != PSFMC_NOT_MINE) return rc;
    }
    return PSFMC_UNKNOWN_SIDE(side);
#endif
}

// rows3_wanted: the shape of the three-stage row family where the side has both; *families: which it is built with
static int row_shape_for(int nx, RowShape* out, bool rows3_wanted = false, RowFamilies* families = nullptr) {
    SizeCall a;
    RowFamilies fam{};
    a.shape = out;
    a.rows3 = rows3_wanted;
    a.families = families ? families : &fam;
    return size_call(SZ_ROW_SHAPE, nx, a);
}

static int flush_linear_sums(psfmc_ctx* c);   // posterior-image sums: see psfmc_reset_accumulated

// ---------------------------------------------------------------------------
// hipFFT plans, cached per batch size (a half-ensemble call and a full-ensemble
// call use different sizes)
// ---------------------------------------------------------------------------
static int use_plans(psfmc_ctx* c, int batch) {
    auto it = c->plans.find(batch);
    if (it == c->plans.end()) {
        if (c->plans.size() >= 8) {
            for (auto& kv : c->plans) {
                hipfftDestroy(kv.second.first);
                hipfftDestroy(kv.second.second);
            }
            c->plans.clear();
        }
        int n[2] = {c->ny, c->nx};
        hipfftHandle f = 0, b = 0;
        FFT_TRY(hipfftPlanMany(&f, 2, n, nullptr, 1, 0, nullptr, 1, 0, HIPFFT_D2Z, batch));
        FFT_TRY(hipfftPlanMany(&b, 2, n, nullptr, 1, 0, nullptr, 1, 0, HIPFFT_Z2D, batch));
        it = c->plans.emplace(batch, std::make_pair(f, b)).first;
    }
    c->plan_fwd = it->second.first;
    c->plan_inv = it->second.second;
    return PSFMC_OK;
}

static void free_work(psfmc_ctx* c) {
    void** bufs[] = {(void**)&c->d_real, (void**)&c->d_spec, (void**)&c->d_Ts[0], (void**)&c->d_Ts[1],
                     (void**)&c->d_Ts[2], (void**)&c->d_Ts[3]};
    for (void** p : bufs)
        if (*p) {
            (void)hipFree(*p);
            *p = nullptr;
        }
    c->d_T = nullptr;
}

static int alloc_work(psfmc_ctx* c) {
    free_work(c);
    if (c->backend == PSFMC_BACKEND_HIPFFT) {
        const size_t nimg = (size_t)2 * c->chunk;
        HIP_TRY(hipMalloc(&c->d_real, nimg * c->S * sizeof(double)));
        HIP_TRY(hipMalloc(&c->d_spec, nimg * c->F * sizeof(double2)));
        return use_plans(c, (int)nimg);
    }
    // buffer 0 also serves batches of up to two chunks that run as ONE pass (run_pipeline)
    c->single_cap = 2 * c->chunk < c->max_walkers ? 2 * c->chunk : c->max_walkers;
    if (c->single_cap < c->chunk) c->single_cap = c->chunk;
    for (int i = 0; i < c->n_streams; ++i)
        HIP_TRY(hipMalloc(&c->d_Ts[i], (size_t)(i ? c->chunk : c->single_cap) * 2 * c->nxh * c->nyp *
                                           (c->t_f32 ? sizeof(cf) : sizeof(cd))));
    c->d_T = c->d_Ts[0];
    return PSFMC_OK;
}

// Walkers per internal pass of the fused path: the transposed half-spectra of one pass
// (two passes in flight, together just under the 256 MiB Infinity Cache: measured
// best at 256^2 -- 104..120 walkers; 136 and more fall off -- see DESIGN.md).
// Never rounded UP past that budget: 32 walkers at 512^2 (2 x 135 MB) ran 6 % slower than
// 24, 16 at 1024^2 8 % slower than 6 (gpurun_out r2i sweep).
static int fused_pass_walkers(const psfmc_ctx* c) {
    const double per_walker = 2.0 * c->nxh * c->nyp * (c->t_f32 ? 8.0 : 16.0);
    // Up to 1024^2: 112 MiB per pass, two passes in flight (rounds 1-3, swept per size).  Above, the kernel spectra
    // and the packed field pixels -- each the size of one walker's T -- are a third of the Infinity Cache and count:
    // two passes + the two shared arrays inside 224 MiB (round 4, same box: 1536^2 2 walkers per pass 21.1 k
    // evals/s, 3: 18.2 k, 4: 17.3 k; 2048^2 1: 7.86 k, 2: 7.60 k; 1152^2 4: 28.4 k, 6: 25.4 k)
    const double t64 = 2.0 * c->nxh * c->nyp * 16.0;
    const int fit = t64 <= 17.0e6 ? (int)(112.0 * 1048576.0 / per_walker)
                                  : (int)((224.0 * 1048576.0 - 2.0 * t64) / (2.0 * per_walker));
    int chunk = fit >= 64 ? ((fit + 4) & ~7) : fit >= 16 ? (fit & ~7) : fit >= 4 ? (fit & ~1) : fit;
    // (sides above 1024: 2 walkers per pass at 1536^2, ONE at 2048^2 -- 67 MB of T each, two passes in flight)
    return chunk < 1 ? 1 : chunk;
}

// per-kernel timing: bracket a launch with events on its own stream
enum { PROF_ROWS_FWD = 0, PROF_COLS = 1, PROF_ROWS_INV = 2 };
struct ProfScope {
    psfmc_ctx* c; int kind; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(psfmc_ctx* c_, int kind_, hipStream_t st_) : c(c_), kind(kind_), st(st_) {
        if (c->profile && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess)
            (void)hipEventRecord(a, st);
    }
    ~ProfScope() {
        if (c->profile && a && b) {
            (void)hipEventRecord(b, st);
            c->prof_pending.push_back({kind, a, b});
        }
    }
};

static void prof_collect(psfmc_ctx* c) {
    for (auto& r : c->prof_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            c->prof_ms[r.kind] += ms;
            c->prof_n[r.kind] += 1;
        }
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    c->prof_pending.clear();
}

// rasterise + both convolutions of `n` walkers; results stay in d_T (spectral
// rows after the column pass).  rows_inv is launched by the caller.
static int fused_rows_fwd(psfmc_ctx* c, int n, cd* Tbuf, const double* prep, const uint8_t* skip,
                          int ps_only, double* raw_out, hipStream_t st) {
    ProfScope ps(c, PROF_ROWS_FWD, st);
    SizeCall a;
    a.c = c; a.n = n; a.prep = prep; a.skip = skip; a.T = Tbuf; a.ps_only = ps_only; a.raw_out = raw_out; a.st = st;
    a.f32 = c->t_f32;
    return size_call(SZ_ROWS_FWD, c->nx, a);
}

static int fused_cols(psfmc_ctx* c, int n, cd* Tbuf, const double* prep, const uint8_t* skip, hipStream_t st) {
    ProfScope ps(c, PROF_COLS, st);
    SizeCall a;
    a.c = c; a.n = n; a.prep = prep; a.skip = skip; a.T = Tbuf; a.st = st; a.f32 = c->t_f32;
    return size_call(SZ_COLS, c->ny, a);
}

static int fused_forward(psfmc_ctx* c, int n, cd* Tbuf, const double* prep, const uint8_t* skip,
                         int ps_only, double* raw_out, hipStream_t st) {
    RC_TRY(fused_rows_fwd(c, n, Tbuf, prep, skip, ps_only, raw_out, st));
    return fused_cols(c, n, Tbuf, prep, skip, st);
}

static int fused_inverse(psfmc_ctx* c, int n, const cd* Tbuf, const double* prep, const uint8_t* skip,
                         double* partial, double* conv_out, double* var_out, hipStream_t st) {
    ProfScope ps(c, PROF_ROWS_INV, st);
    SizeCall a;
    a.c = c; a.n = n; a.prep = prep; a.skip = skip; a.T = const_cast<cd*>(Tbuf); a.partial = partial;
    a.conv_out = conv_out; a.var_out = var_out; a.st = st; a.f32 = c->t_f32;
    return size_call(SZ_ROWS_INV, c->nx, a);
}

static std::vector<cd> twiddle_table(int n) {
    std::vector<cd> t(n);
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int k = 0; k < n; ++k) {
        const long double a = two_pi * (long double)k / (long double)n;
        t[k] = cd{(double)cosl(a), (double)-sinl(a)};
    }
    return t;
}

// ---------------------------------------------------------------------------
// F0: kernel spectra on the device (replaces utils.py:9-22, :126-133)
// d_canvas: [2*n_psf][S], image 2p = padded PSF p, image 2p+1 = its variance map
// ---------------------------------------------------------------------------
static int spectra_hipfft(psfmc_ctx* c, const double* d_canvas) {
    HIP_TRY(hipMalloc(&c->d_pspec, (size_t)c->n_psf * c->F * sizeof(double2)));
    HIP_TRY(hipMalloc(&c->d_vspec, (size_t)c->n_psf * c->F * sizeof(double2)));
    hipfftHandle plan;
    int n[2] = {c->ny, c->nx};
    FFT_TRY(hipfftPlanMany(&plan, 2, n, nullptr, 1, 0, nullptr, 1, 0, HIPFFT_D2Z, 1));
    int rc = PSFMC_OK;
    hipfftSetStream(plan, c->stream);
    for (int p = 0; p < c->n_psf && rc == PSFMC_OK; ++p) {
        double* a = const_cast<double*>(d_canvas) + (size_t)(2 * p) * c->S;
        if (hipfftExecD2Z(plan, a, (hipfftDoubleComplex*)(c->d_pspec + (size_t)p * c->F)) != HIPFFT_SUCCESS ||
            hipfftExecD2Z(plan, a + c->S, (hipfftDoubleComplex*)(c->d_vspec + (size_t)p * c->F)) !=
                HIPFFT_SUCCESS)
            rc = fail(PSFMC_EHIP, "hipfftExecD2Z (PSF spectra) failed");
    }
    (void)hipStreamSynchronize(c->stream);
    hipfftDestroy(plan);
    return rc;
}

static int spectra_fused(psfmc_ctx* c, const double* d_canvas) {
    const size_t n_el = (size_t)c->n_psf * 2 * c->nxh * c->ny;
    HIP_TRY(hipMalloc(&c->d_Kraw, (size_t)c->n_psf * 2 * c->nxh * c->nyp * sizeof(cd)));
    HIP_TRY(hipMemsetAsync(c->d_Kraw, 0, (size_t)c->n_psf * 2 * c->nxh * c->nyp * sizeof(cd), c->stream));
    HIP_TRY(hipMalloc(&c->d_Kt, n_el * sizeof(cd)));
    {
        SizeCall a;
        a.c = c; a.n = c->n_psf; a.T = c->d_Kraw; a.img = d_canvas; a.img_scale = c->d_rho; a.st = c->stream;
        a.from_image = true;
        RC_TRY(size_call(SZ_ROWS_FWD, c->nx, a));
        a.convolve = false;
        RC_TRY(size_call(SZ_COLS, c->ny, a));
    }
    hipLaunchKernelGGL(k_scale_kernel_spectrum, dim3(256), dim3(256), 0, c->stream, c->d_Kraw, c->d_Kt,
                       (int)n_el, c->ny, c->nxh, c->rg_log2, 0.25 / (double)c->S);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PSFMC_OK;
}

// ---------------------------------------------------------------------------
// API
// ---------------------------------------------------------------------------
extern "C" int psfmc_abi_version(void) { return 1; }

extern "C" const char* psfmc_last_error(void) { return g_err.c_str(); }

// psf / psf_var: every field's [n_psf_field][psf_ny[f]][psf_nx[f]] block, in field order
static int ctx_init(psfmc_ctx* c, const double* sci, const double* obs_var, const uint8_t* bad_px,
                    const int* psf_ny, const int* psf_nx, const double* psf, const double* psf_var) {
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < psfmc_ctx::kMaxStreams; ++i) HIP_TRY(hipEventCreateWithFlags(&c->ev_stagger[i], hipEventDisableTiming));
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreateWithFlags(&c->ev_excl[k][i], hipEventDisableTiming));
    for (int i = 1; i < psfmc_ctx::kMaxStreams; ++i) {
        HIP_TRY(hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming));
    }
    const size_t all_px = (size_t)c->n_fields * c->S;             // [field][ny][nx]
    HIP_TRY(hipMalloc(&c->d_sci, all_px * sizeof(double)));
    HIP_TRY(hipMalloc(&c->d_var, all_px * sizeof(double)));
    HIP_TRY(hipMalloc(&c->d_bad, all_px));
    HIP_TRY(hipMemcpy(c->d_sci, sci, all_px * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_var, obs_var, all_px * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_bad, bad_px, all_px, hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&c->d_rows, (size_t)c->max_walkers * c->rlen * sizeof(double)));
    HIP_TRY(hipMalloc(&c->d_prep, (size_t)c->max_walkers * c->plen * sizeof(double)));
    HIP_TRY(hipMalloc(&c->d_like, (size_t)c->max_walkers * sizeof(double)));
    HIP_TRY(hipMalloc(&c->d_skip, (size_t)c->max_walkers));
    HIP_TRY(hipMalloc(&c->d_partial, (size_t)c->max_walkers * c->nblk * sizeof(double)));
    // the fields' image sides (multi-field record derivation) and, embedded, the descriptor of every kernel spectrum
    std::vector<int> sides(2 * (size_t)c->n_fields);
    std::vector<WrapDesc> wrap_tab(c->n_psf);
    for (int f = 0; f < c->n_fields; ++f) {
        sides[2 * f] = c->wraps[f].ly;
        sides[2 * f + 1] = c->wraps[f].lx;
        for (int p = 0; p < c->n_psf_field; ++p) wrap_tab[(size_t)f * c->n_psf_field + p] = c->wraps[f];
    }
    HIP_TRY(hipMalloc(&c->d_field_sides, sides.size() * sizeof(int)));
    HIP_TRY(hipMemcpy(c->d_field_sides, sides.data(), sides.size() * sizeof(int), hipMemcpyHostToDevice));
    if (c->embed) {
        HIP_TRY(hipMalloc(&c->d_wrap, wrap_tab.size() * sizeof(WrapDesc)));
        HIP_TRY(hipMemcpy(c->d_wrap, wrap_tab.data(), wrap_tab.size() * sizeof(WrapDesc), hipMemcpyHostToDevice));
    }
    // where field f's PSF block starts in psf / psf_var
    std::vector<size_t> psf_off(c->n_fields + 1, 0);
    for (int f = 0; f < c->n_fields; ++f)
        psf_off[f + 1] = psf_off[f] + (size_t)c->n_psf_field * psf_ny[f] * psf_nx[f];

    if (c->backend == PSFMC_BACKEND_FUSED) {
        const std::vector<cd> tx = twiddle_table(c->nx), ty = twiddle_table(c->ny);
        HIP_TRY(hipMalloc(&c->d_twx, tx.size() * sizeof(cd)));
        HIP_TRY(hipMalloc(&c->d_twy, ty.size() * sizeof(cd)));
        HIP_TRY(hipMemcpy(c->d_twx, tx.data(), tx.size() * sizeof(cd), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_twy, ty.data(), ty.size() * sizeof(cd), hipMemcpyHostToDevice));
        // rho[p] = 2^-round(log2(sum of the variance map)): brings the variance
        // channel of the packed complex transforms up to the model channel's scale
        std::vector<double> rho(c->n_psf, 1.0);
        for (int p = 0; p < c->n_psf; ++p) {
            const int f = p / c->n_psf_field;
            const size_t small_n = (size_t)psf_ny[f] * psf_nx[f];
            const double* pv = psf_var + psf_off[f] + (size_t)(p % c->n_psf_field) * small_n;
            double tot = 0.0;
            for (size_t i = 0; i < small_n; ++i) tot += pv[i];
            if (tot > 0.0 && std::isfinite(tot)) {
                int e;
                (void)frexp(tot, &e);
                rho[p] = ldexp(1.0, -e);
            }
        }
        HIP_TRY(hipMalloc(&c->d_rho, c->n_psf * sizeof(double)));
        HIP_TRY(hipMemcpy(c->d_rho, rho.data(), c->n_psf * sizeof(double), hipMemcpyHostToDevice));
        size_t field_len = 0;
        {
            SizeCall a;
            a.len = &field_len; a.ny = c->ny; a.rows3 = c->rows3_inv;
            RC_TRY(size_call(SZ_FIELD_LEN, c->nx, a));
        }
        c->field_len = field_len;
        HIP_TRY(hipMalloc(&c->d_field, (size_t)c->n_fields * field_len * sizeof(FieldPx)));
        for (int f = 0; f < c->n_fields; ++f) {
            SizeCall a;
            a.c = c; a.field = f;
            RC_TRY(size_call(SZ_PACK_FIELD, c->nx, a));
        }
    }

    // centre-padded canvases, interleaved (psf0, var0, psf1, var1, ...), each field's at its own PSF shape
    std::vector<double> inter(2 * psf_off[c->n_fields]);
    for (int p = 0; p < c->n_psf; ++p) {
        const int f = p / c->n_psf_field;
        const size_t small = (size_t)psf_ny[f] * psf_nx[f];
        const size_t src = psf_off[f] + (size_t)(p % c->n_psf_field) * small;
        const size_t dst = 2 * psf_off[f] + (size_t)(2 * (p % c->n_psf_field)) * small;
        memcpy(&inter[dst], psf + src, small * sizeof(double));
        memcpy(&inter[dst + small], psf_var + src, small * sizeof(double));
    }
    double *d_small = nullptr, *d_canvas = nullptr;
    HIP_TRY(hipMalloc(&d_small, inter.size() * sizeof(double)));
    int rc = PSFMC_OK;
    if (hipMalloc(&d_canvas, (size_t)2 * c->n_psf * c->S * sizeof(double)) != hipSuccess)
        rc = fail(PSFMC_ENOMEM, "hipMalloc(canvas) failed");
    if (rc == PSFMC_OK &&
        hipMemcpy(d_small, inter.data(), inter.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(PSFMC_EHIP, "hipMemcpy(psf) failed");
    if (rc == PSFMC_OK) {
        for (int f = 0; f < c->n_fields; ++f)
            hipLaunchKernelGGL(k_pad, dim3(256), dim3(256), 0, c->stream, d_small + 2 * psf_off[f],
                               d_canvas + (size_t)2 * f * c->n_psf_field * c->S, 2 * c->n_psf_field, psf_ny[f], psf_nx[f],
                               c->ny, c->nx);
        rc = c->backend == PSFMC_BACKEND_FUSED ? spectra_fused(c, d_canvas) : spectra_hipfft(c, d_canvas);
    }
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(d_small);
    if (d_canvas) (void)hipFree(d_canvas);
    RC_TRY(rc);
    RC_TRY(alloc_work(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PSFMC_OK;
}

// One axis of an image whose side `l` the transforms are not built for: the smallest built side
// m >= l + pk - 1 (pk the PSF's side on that axis), the margin a in front of the image and the extent e of
// the filled transform pixels (psfmc_device.h WrapDesc).  The kernel's origin inside the centre-padded
// PSF, c = m/2 - (m - pk)/2 (utils.py:9-22 + the ifftshift of :32), is the same for every even m, so
// outputs [a, a + l) of the length-m circular convolution are those of the length-l one when a = pk - 1 - c.
static void embed_axis_at(int l, int pk, int m, int* a, int* e) {
    const int c = m / 2 - (m - pk) / 2;
    *a = pk - 1 - c;
    *e = l + pk - 1;
}

// The transform shape of a context's fields (image sides ly[f] x lx[f], PSF sides pky[f] x pkx[f]), per axis:
// an axis on which every field has one built side keeps it; otherwise a built side m serves if every field
// either has that side (it is not embedded on the axis) or fits with its wrap-around margin, m >= l + pk - 1
// (embedded).  The kernels of the built sides differ by up to 2x per pixel (radix mix, lanes per transform,
// registers), so the smallest pair is often not the cheapest: the pair (my, mx) with the least
// ny nx (rows(nx) + cols(ny)) of the measured table psfmc_side_costs.h wins, if it beats the smallest pair by
// 4 % (the table's noise).  One field (or fields of one shape) get the choice of an image of their own.
// false: no built side serves every field on an axis; *bad = a field the largest built side does not serve.
static bool choose_embedding(int n, const int* ly, const int* lx, const int* pky, const int* pkx, int* my, int* mx,
                             int* bad) {
    auto cost_of = [](int side) -> const SideCost* {
        for (const SideCost& sc : kSideCosts)
            if (sc.side == side) return &sc;
        return nullptr;
    };
    auto fixed_side = [n](const int* l) {            // the axis's side if every field has it and it is built
        for (int f = 1; f < n; ++f)
            if (l[f] != l[0]) return 0;
        return fused_side(l[0]) ? l[0] : 0;
    };
    const int fix_y = fixed_side(ly), fix_x = fixed_side(lx);
    auto misfit = [n](int m, int fix, const int* l, const int* pk) {   // the first field m does not serve, or -1
        if (fix) return m == fix ? -1 : 0;
        for (int f = 0; f < n; ++f)
            if (l[f] != m && m < l[f] + pk[f] - 1) return f;
        return -1;
    };
    int small_y = 0, small_x = 0;
    for (int v : kFusedSides) {
        if (!small_y && misfit(v, fix_y, ly, pky) < 0) small_y = v;
        if (!small_x && misfit(v, fix_x, lx, pkx) < 0) small_x = v;
    }
    if (!small_y || !small_x) {
        *bad = !small_y ? misfit(kMaxFusedSide, fix_y, ly, pky) : misfit(kMaxFusedSide, fix_x, lx, pkx);
        return false;
    }
    *my = small_y; *mx = small_x;
    const SideCost *sy0 = cost_of(small_y), *sx0 = cost_of(small_x);
    if (!sy0 || !sx0) return true;
    const double base = (double)small_y * small_x * (sx0->rows_ps + sy0->cols_ps);
    double best = base * 0.96;
    for (int vy : kFusedSides) {
        if (misfit(vy, fix_y, ly, pky) >= 0) continue;
        const SideCost* sy = cost_of(vy);
        if (!sy) continue;
        for (int vx : kFusedSides) {
            if (misfit(vx, fix_x, lx, pkx) >= 0) continue;
            const SideCost* sx = cost_of(vx);
            if (!sx) continue;
            const double cst = (double)vy * vx * (sx->rows_ps + sy->cols_ps);
            if (cst < best) { best = cst; *my = vy; *mx = vx; }
        }
    }
    return true;
}

// Every context is made here: n_fields fields, field f an image of ny[f] x nx[f] pixels with n_psf PSFs of
// psf_ny[f] x psf_nx[f]; the pixel arrays are the fields' own arrays concatenated in field order.
static int ctx_create_impl(psfmc_ctx** out, int device, int n_fields, const int* ny_f, const int* nx_f,
                           const double* sci, const double* obs_var, const uint8_t* bad_px, int n_psf,
                           const int* psf_ny, const int* psf_nx, const double* psf, const double* psf_var,
                           int n_ps, int n_sersic, int max_walkers, int backend) {
    if (!out) return fail(PSFMC_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_fields < 1 || n_fields > 4096) return fail(PSFMC_EINVAL, "n_fields out of range");
    if (n_fields > 1 && backend != PSFMC_BACKEND_FUSED)
        return fail(PSFMC_EINVAL, "several fields per context need the fused back end");
    if (!ny_f || !nx_f || !psf_ny || !psf_nx) return fail(PSFMC_EINVAL, "NULL shape array");
    if (!sci || !obs_var || !bad_px || !psf || !psf_var) return fail(PSFMC_EINVAL, "NULL input array");
    for (int f = 0; f < n_fields; ++f) {
        if (ny_f[f] < 2 || nx_f[f] < 2 || (ny_f[f] & 1) || (nx_f[f] & 1))
            return fail(PSFMC_EINVAL, "field %d: image sides must be even (got %d x %d)", f, ny_f[f], nx_f[f]);
        if (psf_ny[f] < 1 || psf_nx[f] < 1 || psf_ny[f] > ny_f[f] || psf_nx[f] > nx_f[f])
            return fail(PSFMC_EINVAL, "field %d: PSF larger than the observation is not supported (%d x %d in %d x %d)",
                        f, psf_ny[f], psf_nx[f], ny_f[f], nx_f[f]);
    }
    if (n_psf < 1) return fail(PSFMC_EINVAL, "n_psf must be >= 1");
    if (n_ps < 0 || n_sersic < 0 || n_ps > 16 || n_sersic > 16)
        return fail(PSFMC_EINVAL, "component counts out of range (n_ps=%d n_sersic=%d)", n_ps, n_sersic);
    if (max_walkers < 1) return fail(PSFMC_EINVAL, "max_walkers must be >= 1");
    if (backend != PSFMC_BACKEND_HIPFFT && backend != PSFMC_BACKEND_FUSED)
        return fail(PSFMC_EINVAL, "unknown backend %d", backend);
    int ny = ny_f[0], nx = nx_f[0];                   // the transform's sides
    int row_tiles = 0;
    bool rows3_fwd = false, rows3_inv = false;
    RowShape rs{};
    // every field's image inside the transform: the identity unless it is embedded
    std::vector<WrapDesc> wraps(n_fields);
    for (int f = 0; f < n_fields; ++f) wraps[f] = WrapDesc{nx_f[f], 0, nx_f[f], ny_f[f], 0, ny_f[f]};
    bool embed = false;
    std::vector<double> pad_sci, pad_var;
    std::vector<uint8_t> pad_bad;
    if (backend == PSFMC_BACKEND_FUSED) {
        int bad = 0;
        if (!choose_embedding(n_fields, ny_f, nx_f, psf_ny, psf_nx, &ny, &nx, &bad))
            return fail(PSFMC_EINVAL, "fused backend: field %d: image %d x %d + PSF %d x %d - 1 exceeds the largest "
                        "built side (2048)%s", bad, ny_f[bad], nx_f[bad], psf_ny[bad], psf_nx[bad],
                        n_fields > 1 ? " where the transform shared by the fields needs it" : "");
        // embed the axes on which a field's side is not the transform's (an axis that is stays as it is)
        for (int f = 0; f < n_fields; ++f) {
            if (nx != nx_f[f]) embed_axis_at(nx_f[f], psf_nx[f], nx, &wraps[f].ax, &wraps[f].ex);
            if (ny != ny_f[f]) embed_axis_at(ny_f[f], psf_ny[f], ny, &wraps[f].ay, &wraps[f].ey);
            embed = embed || nx != nx_f[f] || ny != ny_f[f];
        }
        if (embed) {
            // the field arrays in transform coordinates: each image at its (ay, ax), every other pixel excluded
            const size_t S_t = (size_t)ny * nx;
            pad_sci.assign((size_t)n_fields * S_t, 0.0);
            pad_var.assign((size_t)n_fields * S_t, 1.0);
            pad_bad.assign((size_t)n_fields * S_t, 1);
            size_t src = 0;
            for (int f = 0; f < n_fields; ++f) {
                const WrapDesc& w = wraps[f];
                for (int y = 0; y < w.ly; ++y, src += w.lx) {
                    const size_t dst = (size_t)f * S_t + (size_t)(y + w.ay) * nx + w.ax;
                    memcpy(&pad_sci[dst], sci + src, (size_t)w.lx * sizeof(double));
                    memcpy(&pad_var[dst], obs_var + src, (size_t)w.lx * sizeof(double));
                    memcpy(&pad_bad[dst], bad_px + src, (size_t)w.lx);
                }
            }
            sci = pad_sci.data(); obs_var = pad_var.data(); bad_px = pad_bad.data();
        }
        const char* env3 = getenv("PSFMC_ROWS3");
        const int force = env3 ? (atoi(env3) != 0 ? 1 : 0) : -1;          // -1: the defaults
        RowFamilies fam{};
        RC_TRY(row_shape_for(nx, &rs, false, &fam));                       // (the two-stage shape where there is one)
        const bool two = fam.two_stage;
        rows3_inv = !two || (fam.rows3_inv && (force == 1 || (force < 0 && fam.rows3_inv_default)));
        rows3_fwd = !two || (fam.rows3_fwd && force == 1);
        // a power-of-two side takes both kernels of a family (their layouts differ: row groups of 2 against 4)
        if (two && rs.plain && rows3_inv != rows3_fwd) rows3_inv = rows3_fwd = false;
        row_tiles = rows3_inv ? ny : (ny + rs.rg - 1) / rs.rg;             // chi^2 partial sums per walker
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(PSFMC_ENODEV, "no HIP device");
    if (device < 0 || device >= ndev) return fail(PSFMC_ENODEV, "device %d of %d", device, ndev);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PSFMC_ENODEV, "device %d is %s; this library is built for gfx950 only", device,
                    prop.gcnArchName);

    psfmc_ctx* c = new psfmc_ctx;
    c->device = device;
    c->ny = ny; c->nx = nx; c->nxh = nx / 2 + 1; c->S = ny * nx; c->F = ny * c->nxh;
    c->embed = embed; c->wraps = wraps;
    c->n_fields = n_fields; c->n_psf_field = n_psf;
    c->layouts.resize(n_fields);
    c->has_layout.assign(n_fields, 0);
    c->layout_blobs.assign(n_fields, nullptr);
    c->acc_count.assign(n_fields, 0);
    c->aux_records.resize(n_fields);
    c->blk.resize(kAuxBlocks);
    c->n_psf = n_fields * n_psf; c->n_ps = n_ps; c->n_sersic = n_sersic;
    c->max_walkers = max_walkers; c->backend = backend;
    c->rlen = row_len(n_ps, n_sersic);
    c->plen = prep_len(n_ps, n_sersic);
    // the rasteriser's form of (rho^2)^p for this context's kernels (psfmc_device.h pow_tabs_side)
    c->use_pow_tabs = pow_tabs_side(nx);
    c->nyp = ny;
    if (backend == PSFMC_BACKEND_FUSED) {
        c->nblk = row_tiles;
        c->rows3_fwd = rows3_fwd; c->rows3_inv = rows3_inv;
        // the power-of-two row kernels run without row guards: whole workgroups of rows only;
        // any other ny takes the guarded code path of the same shape (layout groups of 4 rows)
        c->row_fast = !rows3_fwd && !rows3_inv && rs.plain && ny % (rs.rg * rs.fast_waves) == 0;
        c->rg_log2 = c->row_fast ? rs.fast_rg_log2 : (rows3_fwd || rows3_inv) ? rows3_rg_log2(nx) : 2;   // (rows3: 2; 0 above 1024)
        c->nyp = t_col_len(ny, c->rg_log2);
        RowShape cs{};
        RC_TRY(row_shape_for(ny, &cs));
        c->plain_shape = !rows3_fwd && !rows3_inv && rs.plain && cs.plain;
        c->cols_grid = prop.multiProcessorCount * 2;
        c->chunk = fused_pass_walkers(c);
        // measured (gpurun_out/stag*_quick.txt, same-box A/B): 64^2 +2.7 %, 128^2 +1.7 %, 256^2 +4.6 %
        // (+3.8 % with two Sersics); 384^2 -0.4 %, 512^2 -1.3...-2.5 %, 1024^2 0, 200^2 -1.6 %, 300^2 -7.7 %,
        // 400^2 -10.6 %: on for the small power-of-two shapes only
        c->stagger = (c->plain_shape && c->row_fast && nx <= 256 && ny <= 256) ? 1 : 0;
    } else {
        c->nblk = (c->S + 1023) / 1024;
        if (c->nblk > 64) c->nblk = 64;
        // keep the work space of the hipFFT path <= ~6 GiB
        const double per_walker = 2.0 * (c->S * 8.0 + c->F * 16.0);
        int chunk = (int)(6.0 * 1073741824.0 / per_walker);
        c->chunk = chunk < 1 ? 1 : chunk;
    }
    if (c->chunk > max_walkers) c->chunk = max_walkers;

    int rc = ctx_init(c, sci, obs_var, bad_px, psf_ny, psf_nx, psf, psf_var);
    if (rc != PSFMC_OK) {
        const std::string keep = g_err;
        psfmc_ctx_destroy(c);
        g_err = keep;
        return rc;
    }
    *out = c;
    return PSFMC_OK;
}

extern "C" int psfmc_ctx_create(psfmc_ctx** out, int device, int ny, int nx, const double* sci,
                                const double* obs_var, const uint8_t* bad_px, int n_psf,
                                int psf_ny, int psf_nx, const double* psf, const double* psf_var,
                                int n_ps, int n_sersic, int max_walkers, int backend) {
    return ctx_create_impl(out, device, 1, &ny, &nx, sci, obs_var, bad_px, n_psf, &psf_ny, &psf_nx, psf, psf_var, n_ps,
                           n_sersic, max_walkers, backend);
}

// Several observed fields in ONE context (fused back end): their walkers share the batches of
// psfmc_eval_theta_device_fields, so many small ensembles run at the rate of one large one (BASELINE config 5:
// independent fields x 256 walkers each).  Field f is an image of ny[f] x nx[f] pixels with n_psf[f] PSFs of
// psf_ny[f] x psf_nx[f] (n_psf[f] the same for every field); sci / obs_var / bad_px and psf / psf_var are the
// fields' own arrays concatenated in field order; the same component counts for every field.  The fields share
// one transform shape (choose_embedding), which every one of them pays for.
extern "C" int psfmc_ctx_create_fields_shaped(psfmc_ctx** out, int device, int n_fields, const int* ny, const int* nx,
                                              const double* sci, const double* obs_var, const uint8_t* bad_px,
                                              const int* n_psf, const int* psf_ny, const int* psf_nx, const double* psf,
                                              const double* psf_var, int n_ps, int n_sersic, int max_walkers) {
    if (!out) return fail(PSFMC_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_fields < 1 || n_fields > 4096) return fail(PSFMC_EINVAL, "n_fields out of range");
    if (!n_psf) return fail(PSFMC_EINVAL, "NULL shape array");
    for (int f = 1; f < n_fields; ++f)
        if (n_psf[f] != n_psf[0])
            return fail(PSFMC_EINVAL, "field %d: %d PSFs where field 0 has %d (every field needs the same number)", f,
                        n_psf[f], n_psf[0]);
    return ctx_create_impl(out, device, n_fields, ny, nx, sci, obs_var, bad_px, n_psf[0], psf_ny, psf_nx, psf, psf_var,
                           n_ps, n_sersic, max_walkers, PSFMC_BACKEND_FUSED);
}

// the same with every field of one shape: sci / obs_var / bad_px [n_fields][ny][nx], psf / psf_var
// [n_fields][n_psf][psf_ny][psf_nx]
extern "C" int psfmc_ctx_create_fields(psfmc_ctx** out, int device, int ny, int nx, int n_fields,
                                       const double* sci, const double* obs_var, const uint8_t* bad_px,
                                       int n_psf, int psf_ny, int psf_nx, const double* psf,
                                       const double* psf_var, int n_ps, int n_sersic, int max_walkers) {
    if (!out) return fail(PSFMC_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_fields < 1 || n_fields > 4096) return fail(PSFMC_EINVAL, "n_fields out of range");
    const std::vector<int> ys(n_fields, ny), xs(n_fields, nx), ks(n_fields, n_psf), pys(n_fields, psf_ny),
        pxs(n_fields, psf_nx);
    return psfmc_ctx_create_fields_shaped(out, device, n_fields, ys.data(), xs.data(), sci, obs_var, bad_px, ks.data(),
                                          pys.data(), pxs.data(), psf, psf_var, n_ps, n_sersic, max_walkers);
}

// a field's own image sides (the shape of its pixel arrays at the C ABI; get_option "transform_ny" / "_nx" gives
// the transform's, shared by every field)
extern "C" int psfmc_field_shape(psfmc_ctx* c, int field, int* ny, int* nx) {
    if (!c || !ny || !nx) return fail(PSFMC_EINVAL, "NULL argument");
    if (field < 0 || field >= c->n_fields) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    *ny = c->wraps[field].ly;
    *nx = c->wraps[field].lx;
    return PSFMC_OK;
}

static void free_joint(psfmc_ctx* c) {
    for (void* b : c->joint.blobs)
        if (b) (void)hipFree(b);
    c->joint.blobs.clear();
    c->joint.fields.clear();
    if (c->joint.d_fields) (void)hipFree(c->joint.d_fields);
    c->joint.d_fields = nullptr;
    c->joint.ready = false;
}

extern "C" int psfmc_ctx_destroy(psfmc_ctx* c) {
    if (!c) return PSFMC_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    prof_collect(c);
    for (auto& kv : c->plans) {
        hipfftDestroy(kv.second.first);
        hipfftDestroy(kv.second.second);
    }
    void* bufs[] = {c->d_sci,  c->d_var,  c->d_bad,     c->d_pspec, c->d_vspec, c->d_rows, c->d_prep,
                    c->d_like, c->d_skip, c->d_partial, c->d_real,  c->d_spec,  c->d_Ts[0], c->d_Kraw,
                    c->d_Kt,   c->d_twx,  c->d_twy,     c->d_img0,  c->d_img1, c->d_rho,   c->d_field, c->d_Ts[1], c->d_acc, c->d_lin, c->d_linpart,
                    c->d_theta, c->d_extra, c->d_lnprior, c->d_rawstage, c->d_field_layouts,
                    c->d_wrap, c->d_field_sides, c->d_Ts[2], c->d_Ts[3], c->stretch.pos, c->stretch.lnp, c->stretch.q, c->stretch.newlnp,
                    c->stretch.rand, c->stretch.chain, c->stretch.lnchain, c->stretch.partner, c->stretch.iter,
                    c->stretch.nacc, c->stretch.accflag, c->stretch.kind, c->stretch.partner_b, c->pt_blob, c->d_integ_flags, c->d_integ_par,
                    c->d_extra_img, c->d_gen_flags, c->d_gen_par, c->d_aux, c->d_mean_flags, c->fisher.stash, c->fisher.partial,
                    c->fisher.io, c->fisher.recs, c->fisher.field_col, c->fisher.link};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    for (const psfmc_ctx::AuxBlockState& k : c->blk) {
        if (k.d_masks) (void)hipFree(k.d_masks);
        if (k.d_par) (void)hipFree(k.d_par);
    }
    for (void* p : c->aux_blobs)
        if (p) (void)hipFree(p);
    for (const std::vector<psfmc_ctx::TieRecord>* v : {&c->ties_live, &c->ties_next})
        for (const psfmc_ctx::TieRecord& r : *v)
            if (r.blob) (void)hipFree(r.blob);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    for (int i = 1; i < psfmc_ctx::kMaxStreams; ++i) {
        if (c->side[i]) {
            (void)hipStreamSynchronize(c->side[i]);
            (void)hipStreamDestroy(c->side[i]);
        }
        if (c->ev_join[i]) (void)hipEventDestroy(c->ev_join[i]);
    }
    for (void* b : c->layout_blobs)
        if (b) (void)hipFree(b);
    free_joint(c);
    if (c->joint.d_lp) (void)hipFree(c->joint.d_lp);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    for (int i = 0; i < psfmc_ctx::kMaxStreams; ++i)
        if (c->ev_stagger[i]) (void)hipEventDestroy(c->ev_stagger[i]);
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 2; ++i)
            if (c->ev_excl[k][i]) (void)hipEventDestroy(c->ev_excl[k][i]);
    delete c;
    return PSFMC_OK;
}

extern "C" int psfmc_row_len(const psfmc_ctx* c) { return c ? c->rlen : PSFMC_EINVAL; }

extern "C" int psfmc_set_option(psfmc_ctx* c, const char* key, double value) {
    if (!c || !key) return fail(PSFMC_EINVAL, "NULL argument");
    if (!strcmp(key, "chunk_walkers")) {
        int v = (int)value;
        if (v < 1 || v > c->max_walkers) return fail(PSFMC_EINVAL, "chunk_walkers out of range");
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipDeviceSynchronize());
        c->chunk = v;
        if (c->d_img0) { (void)hipFree(c->d_img0); c->d_img0 = nullptr; }
        if (c->d_img1) { (void)hipFree(c->d_img1); c->d_img1 = nullptr; }
        if (c->d_rawstage) { (void)hipFree(c->d_rawstage); c->d_rawstage = nullptr; }
        c->img_cap = 0;
        return alloc_work(c);
    }
    if (!strcmp(key, "storage_f32")) {
        // keep the intermediate half-spectra as complex64 (arithmetic stays fp64): half the
        // traffic of every kernel, ~1e-7 relative error in the log-posterior -- the class of the
        // reference's own float32 raw model (psfMC/models.py:249), not an fp64 result
        const bool on = value != 0;
        if (on && (c->backend != PSFMC_BACKEND_FUSED || !c->plain_shape || !c->row_fast || c->embed))
            return fail(PSFMC_EINVAL, "storage_f32 needs the fused back end and power-of-two sides");
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipDeviceSynchronize());
        c->t_f32 = on;
        c->chunk = fused_pass_walkers(c);
        if (c->chunk > c->max_walkers) c->chunk = c->max_walkers;
        if (c->d_img0) { (void)hipFree(c->d_img0); c->d_img0 = nullptr; }
        if (c->d_img1) { (void)hipFree(c->d_img1); c->d_img1 = nullptr; }
        if (c->d_rawstage) { (void)hipFree(c->d_rawstage); c->d_rawstage = nullptr; }
        c->img_cap = 0;
        return alloc_work(c);
    }
    if (!strcmp(key, "cols_grid")) {
        if (value < 1) return fail(PSFMC_EINVAL, "cols_grid must be >= 1");
        c->cols_grid = (int)value;
        return PSFMC_OK;
    }
    if (!strcmp(key, "stagger")) {
        c->stagger = (int)value;
        return PSFMC_OK;
    }
    if (!strcmp(key, "exclusive")) {
        c->exclusive = (int)value & 7;
        return PSFMC_OK;
    }
    if (!strcmp(key, "linear_accumulation")) {
        HIP_TRY(hipSetDevice(c->device));
        RC_TRY(flush_linear_sums(c));
        c->linear_acc = value != 0;
        return PSFMC_OK;
    }
    if (!strcmp(key, "cols3")) {
        // refused here, not at the next evaluation: only the engines col_engine knows, and k_cols only where the
        // transform's column side has a two-stage kernel
        if (!(value >= 0 && value <= 4) || value != (double)(int)value)
            return fail(PSFMC_EINVAL, "cols3 must be one of 0, 1, 2, 3, 4 (got %g)", value);
        if (value == 0 && c->backend == PSFMC_BACKEND_FUSED && !two_stage_side(c->ny))
            return fail(PSFMC_EINVAL, "cols3 = 0: transform side %d has only the three-stage column kernels", c->ny);
        c->cols3 = (int)value;
        return PSFMC_OK;
    }
    if (!strcmp(key, "speculate")) {
        c->speculate = (int)value;          // 0 never, n > 0 up to n walkers per half, -1 the default rule
        return PSFMC_OK;
    }
    if (!strcmp(key, "graph")) {
        c->use_graph = value != 0;
        return PSFMC_OK;
    }
    if (!strcmp(key, "min_split")) {
        c->min_split = value < 1 ? 1 : (int)value;
        return PSFMC_OK;
    }
    if (!strcmp(key, "profile")) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipDeviceSynchronize());
        prof_collect(c);
        c->profile = value != 0;
        for (int i = 0; i < 3; ++i) { c->prof_ms[i] = 0; c->prof_n[i] = 0; }
        return PSFMC_OK;
    }
    if (!strcmp(key, "streams")) {
        if (value < 1 || value > psfmc_ctx::kMaxStreams) return fail(PSFMC_EINVAL, "streams must be 1..4");
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipDeviceSynchronize());
        c->n_streams = (int)value;
        return alloc_work(c);
    }
    return fail(PSFMC_EINVAL, "unknown option '%s'", key);
}

extern "C" double psfmc_get_option(const psfmc_ctx* cc, const char* key) {
    if (!cc || !key) return NAN;
    psfmc_ctx* c = const_cast<psfmc_ctx*>(cc);
    static const char* kinds[3] = {"rows_fwd", "cols", "rows_inv"};
    for (int i = 0; i < 3; ++i) {
        char name[64];
        snprintf(name, sizeof name, "prof_ms_%s", kinds[i]);
        if (!strcmp(key, name)) { prof_collect(c); return c->prof_ms[i]; }
        snprintf(name, sizeof name, "prof_n_%s", kinds[i]);
        if (!strcmp(key, name)) { prof_collect(c); return (double)c->prof_n[i]; }
    }
    if (!strcmp(key, "row_group")) return 1 << c->rg_log2;
    if (!strcmp(key, "rows3")) return (c->rows3_fwd ? 1.0 : 0.0) + (c->rows3_inv ? 2.0 : 0.0);   // bit 0 forward, bit 1 inverse
    // what the choice functions answer for this context NOW.  column_engine: 0 k_cols, 1 k_cols3, 2 k_cols3g, 3 k_cols3f;
    // raster_group: pixels per group of the forward row kernel's power-table rasteriser (0: log2 + exp2 form)
    const bool col_engine_key = !strcmp(key, "column_engine");
    if (col_engine_key || !strcmp(key, "raster_group")) {
        if (c->backend != PSFMC_BACKEND_FUSED) return NAN;
        int code = 0;
        SizeCall a;
        a.c = c; a.code = &code;
        const int rc = col_engine_key ? size_call(SZ_COL_ENGINE, c->ny, a) : size_call(SZ_RASTER_GROUP, c->nx, a);
        return rc == PSFMC_OK ? (double)code : NAN;
    }
    if (!strcmp(key, "speculate")) return c->speculate;
    if (!strcmp(key, "pow_tabs")) return c->use_pow_tabs ? 1.0 : 0.0;
    if (!strcmp(key, "pow_tabs_built")) return c->prep_tabs_built ? 1.0 : 0.0;   // the last batch read k_pow_tables' output
    if (!strcmp(key, "speculated_runs")) return (double)c->speculated_runs;
    if (!strcmp(key, "transform_ny")) return c->ny;        // the transform shape (the image's own, or the one it is embedded in)
    if (!strcmp(key, "transform_nx")) return c->nx;
    if (!strcmp(key, "partials_per_walker")) return c->nblk;
    if (!strcmp(key, "storage_f32")) return c->t_f32 ? 1.0 : 0.0;
    if (!strcmp(key, "graph_launches")) return (double)c->graph_launches;
    if (!strcmp(key, "chunk_walkers")) return c->chunk;
    if (!strcmp(key, "backend")) return c->backend;
    if (!strcmp(key, "max_walkers")) return c->max_walkers;
    if (!strcmp(key, "cols_grid")) return c->cols_grid;
    if (!strcmp(key, "streams")) return c->n_streams;
    if (!strcmp(key, "stagger")) return c->stagger;
    if (!strcmp(key, "exclusive")) return c->exclusive;
    if (!strcmp(key, "cols3")) return c->cols3;
    if (!strcmp(key, "linear_accumulation")) return c->linear_acc ? 1.0 : 0.0;
    if (!strcmp(key, "aux_stride")) return c->aux_stride;  // doubles per walker of the auxiliary vectors (0: none yet)
    return NAN;
}

// ---------------------------------------------------------------------------
// hipFFT path: rasterise + convolve one chunk; results in d_real (conv, var)
// ---------------------------------------------------------------------------
static int hipfft_convolve(psfmc_ctx* c, int n, const double* d_prep, const uint8_t* d_skip,
                           hipStream_t st, int ps_only) {
    const size_t lds = (size_t)prep_rec_len(c->n_ps, c->n_sersic) * sizeof(double);
    RC_TRY(use_plans(c, 2 * n));
    hipLaunchKernelGGL(k_raster, dim3((c->S + 1023) / 1024, n), dim3(256), lds, st, d_prep, d_skip,
                       c->d_real, c->n_ps, c->n_sersic, c->ny, c->nx, ps_only, extra_image_of(c, d_prep));
    FFT_TRY(hipfftSetStream(c->plan_fwd, st));
    FFT_TRY(hipfftSetStream(c->plan_inv, st));
    FFT_TRY(hipfftExecD2Z(c->plan_fwd, c->d_real, (hipfftDoubleComplex*)c->d_spec));
    int gx = (c->F + 255) / 256;
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(k_spec_mul, dim3(gx, n), dim3(256), 0, st, c->d_spec, c->d_pspec, c->d_vspec,
                       d_prep, d_skip, c->plen, c->ny, c->nxh, 1.0 / (double)c->S);
    FFT_TRY(hipfftExecZ2D(c->plan_inv, (hipfftDoubleComplex*)c->d_spec, c->d_real));
    return PSFMC_OK;
}

// Walkers per internal pass for a batch of W (fused path).  Pass i runs on stream
// i % n_streams with its own T buffer, so the VALU-bound row kernels of one pass overlap the
// HBM-bound column kernel of its neighbours; passes of equal size (no short tail), an even
// number of them when two run at a time.
// A batch of up to two chunks runs as ONE pass: with only two passes the fork/join
// between the streams costs more than their overlap gains (256^2, MI355X: W = 128
// 148 vs 157 us, W = 224 228 vs 237 us, W = 256 264 vs 269 us, W = 320 353 vs 338 us).
static int pass_size(const psfmc_ctx* c, int W) {
    const bool fused = c->backend == PSFMC_BACKEND_FUSED;
    int chunk = c->chunk;
    if (fused && c->n_streams > 1 && W <= chunk && W / 2 >= c->min_split) chunk = ((W + 1) / 2 + 7) & ~7;
    if (fused && W > chunk && W <= c->single_cap && c->min_split > W / 2) {
        chunk = W;
    } else if (fused && W > chunk) {
        int np = (W + chunk - 1) / chunk;
        if (c->n_streams == 2 && (np & 1)) ++np;
        chunk = (((W + np - 1) / np) + 3) & ~3;
        // the T buffers hold c->chunk walkers: rounding up must never pass that
        if (chunk > c->chunk) chunk = c->chunk;
    } else if (chunk > c->chunk) {
        chunk = c->chunk;
    }
    return chunk;
}

extern "C" int psfmc_pass_size(const psfmc_ctx* c, int W) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (W < 1 || W > c->max_walkers) return fail(PSFMC_EINVAL, "W=%d outside [1, max_walkers=%d]", W, c->max_walkers);
    return pass_size(c, W);
}

// the likelihood pipeline over walkers whose prep records are in c->d_prep;
// leaves the chi^2 partial sums in c->d_partial.  Fork/join on events keeps the caller's
// stream semantics.
static int run_pipeline(psfmc_ctx* c, int W, const uint8_t* d_skip, hipStream_t st, int w_off = 0) {
    const bool fused = c->backend == PSFMC_BACKEND_FUSED;
    const int chunk = pass_size(c, W);
    const int npass = (W + chunk - 1) / chunk;
    const int lanes = !fused ? 1 : (npass < c->n_streams ? npass : c->n_streams);
    if (lanes > 1) {
        HIP_TRY(hipEventRecord(c->ev_fork, st));
        for (int i = 1; i < lanes; ++i) HIP_TRY(hipStreamWaitEvent(c->side[i], c->ev_fork, 0));
    }
    int pass = 0;
    for (int w0 = 0; w0 < W; w0 += chunk, ++pass) {
        const int n = W - w0 < chunk ? W - w0 : chunk;
        // walkers [w_off, w_off + W) of the prep / skip / partial arrays
        const double* prep = c->d_prep + (size_t)(w_off + w0) * c->plen;
        const uint8_t* skip = d_skip ? d_skip + w_off + w0 : nullptr;
        double* partial = c->d_partial + (size_t)(w_off + w0) * c->nblk;
        if (fused) {
            const int lane = pass % lanes;
            hipStream_t s = lane ? c->side[lane] : st;
            cd* Tbuf = c->d_Ts[lane];
            if (c->stagger && lanes >= 2 && npass >= 8 && pass < lanes - 1) {
                // start the next lane one forward-row kernel late, so that its VALU-bound kernel
                // meets this lane's memory-bound ones instead of this lane's own copy of it (the idle
                // start costs about half a kernel per batch: worth it from ~8 passes on; 4 passes of
                // 64 walkers ran 249 instead of 235 us with it)
                RC_TRY(fused_rows_fwd(c, n, Tbuf, prep, skip, 0, nullptr, s));
                HIP_TRY(hipEventRecord(c->ev_stagger[pass], s));
                HIP_TRY(hipStreamWaitEvent(c->side[pass + 1], c->ev_stagger[pass], 0));
                RC_TRY(fused_cols(c, n, Tbuf, prep, skip, s));
            } else if (c->exclusive && lanes == 2) {
                // kind k of this pass starts only when kind k of the previous pass (the other lane) has finished
                auto gate = [&](int k) -> int {
                    if ((c->exclusive >> k) & 1) {
                        if (pass > 0) HIP_TRY(hipStreamWaitEvent(s, c->ev_excl[k][(pass - 1) & 1], 0));
                    }
                    return PSFMC_OK;
                };
                auto done = [&](int k) -> int {
                    if ((c->exclusive >> k) & 1) HIP_TRY(hipEventRecord(c->ev_excl[k][pass & 1], s));
                    return PSFMC_OK;
                };
                RC_TRY(gate(0));
                RC_TRY(fused_rows_fwd(c, n, Tbuf, prep, skip, 0, nullptr, s));
                RC_TRY(done(0));
                RC_TRY(gate(1));
                RC_TRY(fused_cols(c, n, Tbuf, prep, skip, s));
                RC_TRY(done(1));
                RC_TRY(gate(2));
                RC_TRY(fused_inverse(c, n, Tbuf, prep, skip, partial, nullptr, nullptr, s));
                RC_TRY(done(2));
                continue;
            } else {
                RC_TRY(fused_forward(c, n, Tbuf, prep, skip, 0, nullptr, s));
            }
            RC_TRY(fused_inverse(c, n, Tbuf, prep, skip, partial, nullptr, nullptr, s));
        } else {
            RC_TRY(hipfft_convolve(c, n, prep, skip, st, 0));
            hipLaunchKernelGGL(k_chi2, dim3(c->nblk, n), dim3(256), 0, st, c->d_real, c->d_sci, c->d_var,
                               c->d_bad, skip, partial, c->S);
        }
    }
    for (int i = 1; i < lanes; ++i) {
        HIP_TRY(hipEventRecord(c->ev_join[i], c->side[i]));
        HIP_TRY(hipStreamWaitEvent(st, c->ev_join[i], 0));
    }
    return PSFMC_OK;
}

// The power tables of every (walker, Sersic component) of a batch, behind the walkers' prep records
// (psfmc_device.h: what the fused rasteriser reads instead of a log2 and an exp2 per pixel).  One wave per
// pair; p = 1 / (2n) is the record's own value, so a table and the record it belongs to always agree.
__global__ void __launch_bounds__(256) k_pow_tables(double* __restrict__ prep, const uint8_t* __restrict__ skip,
                                                    int n_pairs, int n_ps, int n_sersic) {
    const int pair = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pair >= n_pairs) return;                                   // wave-uniform
    const int w = pair / n_sersic, k = pair - w * n_sersic;
    if (skip && skip[w]) return;
    double* rec = prep + (size_t)w * prep_len(n_ps, n_sersic);
    const double p = rec[kPrepHead + kPrepPs * n_ps + kPrepSersic * k + 7];
    build_pow_table(p, rec + prep_rec_len(n_ps, n_sersic) + (size_t)k * kPowTab, lane);
}
// The walkers' extra images: pixel-integrated Sersic components (psfmc_integrated.h), then general Sersic components
// and tilted skies (psfmc_general.h).  After every kernel that writes prep records, same stream, the images are
// formed and the components' blocks made neutral for the rasterisers.  The integrated profile's kernels WRITE the
// images, the general kernel then ADDS to them; alone it writes.
// What a launch of the general kernels carries is decided ONCE, here, from the blocks' any-bits and the facts table:
// block j is carried when some block b with `any` set has kAuxBlock[b].first <= j <= b.  So laws, truncations and bending
// bring the masks and constants of every block before them, a context with only spirals does not carry the Fourier
// buffers, and a context without modes and without spirals runs the kernels it always ran.
enum GenLevel { GEN_PLAIN = 0, GEN_FOU = 1, GEN_SPI = 2, GEN_FOU_SPI = 3, GEN_RAD, GEN_TRU, GEN_BND };
struct GenLaunch {
    double* par[kAuxBlocks];             // the block's per-walker constants from walker w_off on; nullptr: not carried
    const uint8_t* masks[kAuxBlocks];    // its mask bytes, or nullptr
    int off[kAuxBlocks];                 // its first entry in a walker's auxiliary vector
    GenLevel level;                      // which instantiation of the general kernels the context needs
};
static GenLaunch general_launch(const psfmc_ctx* c, int w_off) {
    GenLaunch g{};
    int off = c->aux_base, last = -1;
    for (int b = 0; b < kAuxBlocks; ++b) {
        g.off[b] = off;
        off += aux_block_len(b, c->n_sersic);
        if (!c->blk[b].any) continue;
        last = b;
        for (int j = kAuxBlock[b].first; j <= b; ++j) {
            g.par[j] = c->blk[j].d_par + (size_t)w_off * c->n_sersic * kAuxBlock[j].par;
            g.masks[j] = c->blk[j].d_masks;
        }
    }
    g.level = last == kBlkBnd ? GEN_BND : last == kBlkTru ? GEN_TRU : last == kBlkRad ? GEN_RAD
            : GenLevel((c->blk[kBlkFou].any ? GEN_FOU : 0) | (c->blk[kBlkSpi].any ? GEN_SPI : 0));
    return g;
}
static decltype(&k_general_rows<false, false>) general_rows_kernel(GenLevel level) {
    switch (level) {
        case GEN_BND: return k_general_rows<true, true, true, true, true>;
        case GEN_TRU: return k_general_rows<true, true, true, true>;
        case GEN_RAD: return k_general_rows<true, true, true>;
        case GEN_FOU_SPI: return k_general_rows<true, true>;
        case GEN_SPI: return k_general_rows<false, true>;
        case GEN_FOU: return k_general_rows<true, false>;
        default: return k_general_rows<false, false>;
    }
}
static decltype(&k_general_split<false, false>) general_split_kernel(GenLevel level) {
    switch (level) {
        case GEN_BND: return k_general_split<true, true, true, true>;
        case GEN_TRU: return k_general_split<true, true, true>;
        case GEN_RAD: return k_general_split<true, true>;
        case GEN_FOU_SPI: case GEN_SPI: return k_general_split<true, false>;
        default: return k_general_split<false, false>;
    }
}

// k_general_rows over walkers w_off ... w_off + n: every general component, less the mean ones where the context has
// some (the same flags pointer as ever where it has none), and the tilted skies; add: onto the integrated images
static void launch_general_rows(psfmc_ctx* c, const GenLaunch& g, int n, int w_off, const uint8_t* skip,
                                hipStream_t st, int add) {
    const uint8_t* rows_flags = c->mean_any ? c->d_mean_flags + (size_t)c->n_fields * c->n_sersic : c->d_gen_flags;
    hipLaunchKernelGGL(general_rows_kernel(g.level), dim3((c->ny + 3) / 4, n), dim3(256), 0, st,
                       c->d_prep + (size_t)w_off * c->plen, c->plen, skip,
                       c->d_gen_par + (size_t)w_off * c->n_sersic * kGenPar,
                       c->d_aux + (size_t)w_off * c->aux_stride, c->aux_stride, c->aux_n_sky,
                       c->d_gen_flags + (size_t)c->n_fields * c->n_sersic, rows_flags, c->n_sersic, c->n_psf,
                       c->n_psf_field, c->d_wrap, c->ny, c->nx, c->d_extra_img + (size_t)w_off * c->S, add,
                       g.par[kBlkFou], g.masks[kBlkFou], g.par[kBlkSpi], g.masks[kBlkSpi], g.par[kBlkRad],
                       g.masks[kBlkRad], g.par[kBlkTru], g.masks[kBlkTru], g.par[kBlkBnd], g.masks[kBlkBnd]);
}

// the mean components of a context that has some (psfmc_general_mean.h): behind k_general_rows, which left them out
static void launch_general_mean(psfmc_ctx* c, const GenLaunch& g, int n, int w_off, const uint8_t* skip,
                                hipStream_t st) {
    const double* prep = c->d_prep + (size_t)w_off * c->plen;
    double* img = c->d_extra_img + (size_t)w_off * c->S;
    const double* gpar = c->d_gen_par + (size_t)w_off * c->n_sersic * kGenPar;
    const bool tru = g.level == GEN_TRU, bnd = g.level == GEN_BND;
    const auto rows_kernel = bnd ? k_general_mean_rows<true, true>
                           : tru ? k_general_mean_rows<true, false> : k_general_mean_rows<false, false>;
    const auto core_kernel = bnd ? k_general_mean_core<true, true>
                           : tru ? k_general_mean_core<true, false> : k_general_mean_core<false, false>;
    hipLaunchKernelGGL(rows_kernel, dim3((c->ny + 3) / 4, n),
                       dim3(256), 0, st, prep, c->plen, skip, gpar, c->d_mean_flags, c->n_sersic, c->n_psf,
                       c->n_psf_field, c->d_wrap, c->ny, c->nx, img, g.par[kBlkFou], g.masks[kBlkFou],
                       g.par[kBlkSpi], g.masks[kBlkSpi], g.par[kBlkRad], g.masks[kBlkRad], g.par[kBlkTru],
                       g.masks[kBlkTru], g.par[kBlkBnd], g.masks[kBlkBnd]);
    hipLaunchKernelGGL(core_kernel, dim3(n), dim3(64), 0, st, prep,
                       c->plen, skip, gpar, c->d_mean_flags, c->n_sersic, c->n_psf, c->n_psf_field, c->d_wrap, c->ny,
                       c->nx, img, g.par[kBlkFou], g.masks[kBlkFou], g.par[kBlkSpi], g.masks[kBlkSpi],
                       g.par[kBlkRad], g.masks[kBlkRad], g.par[kBlkTru], g.masks[kBlkTru], g.par[kBlkBnd],
                       g.masks[kBlkBnd]);
}

static void launch_extra_images(psfmc_ctx* c, int n, int w_off, const uint8_t* skip, hipStream_t st) {
    if ((!c->integ_any && !c->gen_any) || n <= 0) return;
    double* prep = c->d_prep + (size_t)w_off * c->plen;
    const int items = n * c->n_sersic;
    const GenLaunch g = c->gen_any ? general_launch(c, w_off) : GenLaunch{};
    if (c->gen_any) {
        // (the flags the context owns are writable: a boxiness outside its support skips the walker)
        uint8_t* own_skip = (skip && skip >= c->d_skip && skip < c->d_skip + c->max_walkers) ? const_cast<uint8_t*>(skip)
                                                                                           : nullptr;
        double* gpar = c->d_gen_par + (size_t)w_off * c->n_sersic * kGenPar;
        const double* aux = c->d_aux + (size_t)w_off * c->aux_stride;
        // (the same launch also forms the per-walker constants of the spirals, laws, truncations and bending modes the
        // context carries)
        if (items > 0)
            hipLaunchKernelGGL(general_split_kernel(g.level), dim3((items + 255) / 256), dim3(256), 0, st, prep,
                               c->plen, skip ? own_skip : nullptr, gpar, aux, c->aux_stride, c->aux_n_sky,
                               c->d_gen_flags, c->n_ps, c->n_sersic, c->n_psf, c->n_psf_field, n, g.par[kBlkSpi],
                               g.masks[kBlkSpi], g.off[kBlkSpi], g.par[kBlkRad], g.masks[kBlkRad], g.off[kBlkRad],
                               g.par[kBlkTru], g.masks[kBlkTru], g.off[kBlkTru], g.par[kBlkBnd], g.masks[kBlkBnd],
                               g.off[kBlkBnd]);
        if (c->blk[kBlkFou].any && items > 0)
            hipLaunchKernelGGL(k_fourier_prep, dim3((items + 3) / 4), dim3(256), 0, st, prep, c->plen,
                               skip ? own_skip : nullptr, gpar, g.par[kBlkFou], aux, c->aux_stride, g.off[kBlkFou],
                               g.masks[kBlkFou], c->n_sersic, c->n_psf, c->n_psf_field, n);
        if (!c->integ_any) {
            launch_general_rows(c, g, n, w_off, skip, st, 0);
            if (c->mean_any) launch_general_mean(c, g, n, w_off, skip, st);
            return;
        }
    }
    double* img = c->d_extra_img + (size_t)w_off * c->S;
    double* ipar = c->d_integ_par + (size_t)w_off * c->n_sersic * kPrepSersic;
    hipLaunchKernelGGL(k_integ_split, dim3((items + 255) / 256), dim3(256), 0, st, prep, c->plen, skip, ipar,
                       c->d_integ_flags, c->n_ps, c->n_sersic, c->n_psf, c->n_psf_field, n);
    hipLaunchKernelGGL(k_integ_rows, dim3((c->ny + 3) / 4, n), dim3(256), 0, st, prep, c->plen, skip, ipar,
                       c->d_integ_flags, c->n_sersic, c->n_psf, c->n_psf_field, c->d_wrap, c->ny, c->nx, img);
    hipLaunchKernelGGL(k_integ_core, dim3(n), dim3(64), 0, st, prep, c->plen, skip, ipar, c->d_integ_flags,
                       c->n_sersic, c->n_psf, c->n_psf_field, c->d_wrap, c->ny, c->nx, img);
    if (c->gen_any) launch_general_rows(c, g, n, w_off, skip, st, 1);
    if (c->gen_any && c->mean_any) launch_general_mean(c, g, n, w_off, skip, st);
}

// Small batches run WITHOUT the launch: their forward row waves form the table entries they read themselves (same
// function, same bits; ~400 instructions per wave and component) -- a kernel boundary plus a one-wave-per-pair
// kernel are 4 ... 5 us of a small ensemble's half-step.  "Small" = up to this many (row wave, component) pairs in
// the forward launch, about where the chip's wave slots are full and the extra instructions stop being free
// (64 (walker, component) pairs at 512^2, 16 at 1024^2, ~110 at 288^2).
constexpr int kInWavePowTabWaves = 8192;
// walkers [w_off, w_off + n) of c->d_prep; after the kernel that wrote their records, same stream.
// (Only the forward row kernels read the tables: k_raster_sums keeps the log2 + exp2 form at every size.)
static void launch_extra_images(psfmc_ctx* c, int n, int w_off, const uint8_t* skip, hipStream_t st);
static void launch_pow_tables(psfmc_ctx* c, int n, int w_off, const uint8_t* skip, hipStream_t st) {
    launch_extra_images(c, n, w_off, skip, st);       // (before the tables: it rewrites the flagged components' blocks)
    c->prep_tabs_valid = true;
    if (c->backend != PSFMC_BACKEND_FUSED || c->n_sersic == 0 || n <= 0 || !c->use_pow_tabs) return;
    const int pairs = n * c->n_sersic;
    const bool build = (long long)pairs * c->nblk > kInWavePowTabWaves;
    // a batch written in several pieces (w_off > 0) reads its tables from memory only if every piece has them
    c->prep_tabs_built = w_off == 0 ? build : (c->prep_tabs_built && build);
    if (!build) return;
    hipLaunchKernelGGL(k_pow_tables, dim3((pairs + 3) / 4), dim3(256), 0, st, c->d_prep + (size_t)w_off * c->plen,
                       skip, pairs, c->n_ps, c->n_sersic);
}

// field < 0: the rows' PSF index counts over every kernel spectrum of the context; field >= 0: within that field
static int take_aux_rows(psfmc_ctx* c, int W);
static int eval_device(psfmc_ctx* c, int W, const double* d_rows, const uint8_t* d_skip,
                       double* d_like, hipStream_t st, int field = -1) {
    RC_TRY(take_aux_rows(c, W));
    c->prep_tabs_valid = false;                       // d_prep is being rewritten
    hipLaunchKernelGGL(k_prep, dim3((W + 127) / 128), dim3(128), 0, st, d_rows, c->d_prep, W, c->n_ps,
                       c->n_sersic, c->wraps[field < 0 ? 0 : field].ly, c->wraps[field < 0 ? 0 : field].lx, c->d_rho,
                       field < 0 ? c->n_psf : c->n_psf_field,
                       field < 0 ? 0 : field * c->n_psf_field);
    launch_pow_tables(c, W, 0, d_skip, st);
    RC_TRY(run_pipeline(c, W, d_skip, st));
    hipLaunchKernelGGL(k_finish, dim3(finish_blocks(W)), dim3(kFinishThreads), 0, st, c->d_partial, d_skip, d_like,
                       W, c->nblk);
    HIP_TRY(hipGetLastError());
    return PSFMC_OK;
}

// raw vectors (or, with sp.pos set, stretch-move proposals formed on the fly) -> prep
// records, log-priors and skip flags of W walkers
// `field` / `w_off`: walkers [w_off, w_off + W) of the batch belong to observed field `field` (0, 0
// for the usual one-field context): its layout, its block of kernel spectra
// `n_seg` > 1: ONE launch for the fields `field` .. `field + n_seg - 1`, W walkers each (blockIdx.y = field):
// the same per-walker arrays with field f's block at offset f W, every field's own layout
// where k_theta_prep writes the auxiliary vectors of the walkers from w_off on (nullptr: the context has none);
// aux rows a caller left for a row-based call are gone
static AuxOut aux_out(psfmc_ctx* c, int w_off) {
    c->aux_rows_w = -1;
    return AuxOut{c->d_aux ? c->d_aux + (size_t)w_off * c->aux_stride : nullptr, c->aux_stride};
}
// Row-based calls on a context with general components or tilted skies read the walkers' auxiliary vectors that
// psfmc_set_aux_rows left in d_aux; they serve one call.
static int take_aux_rows(psfmc_ctx* c, int W) {
    if (!c->gen_any) return PSFMC_OK;
    const int have = c->aux_rows_w;
    c->aux_rows_w = -1;
    if (have != W)
        return fail(PSFMC_EINVAL, "this context has general Sersic components or tilted skies (boxiness / slope): call "
                    "psfmc_set_aux_rows for the %d walkers of a row-based call first (aux rows of %d walkers are set)",
                    W, have);
    return PSFMC_OK;
}
static void launch_theta_prep(psfmc_ctx* c, int W, const double* d_theta, const double* d_extra,
                              double* d_rows, hipStream_t st, const StretchIn& sp, int field = 0, int w_off = 0,
                              int n_seg = 1) {
    const ThetaLayout& L = c->layouts[field];
    FieldSegs segs{nullptr, nullptr, 0};
    if (n_seg > 1) segs = FieldSegs{c->d_field_layouts + field, c->d_field_sides + 2 * field, c->n_psf_field};
    if (w_off == 0) c->prep_tabs_valid = false;       // d_prep is being rewritten (w_off > 0: a further piece of one batch)
    hipLaunchKernelGGL(k_theta_prep, dim3((W + kThetaThreads - 1) / kThetaThreads, n_seg),
                       dim3(kThetaThreads, theta_task_waves(c->n_ps, c->n_sersic)), c->theta_lds, st,
                       L, d_theta, d_extra, d_rows, c->d_prep + (size_t)w_off * c->plen, c->d_lnprior + w_off,
                       c->d_skip + w_off, W, c->wraps[field].ly, c->wraps[field].lx, c->d_rho, sp, field * c->n_psf_field,
                       segs, aux_out(c, w_off));
    launch_pow_tables(c, W * n_seg, w_off, c->d_skip + w_off, st);
}

// raw vectors -> log-posterior, everything on the device
static int eval_theta_device(psfmc_ctx* c, int W, const double* d_theta, const double* d_extra,
                             double* d_lnprob, hipStream_t st) {
    launch_theta_prep(c, W, d_theta, d_extra, nullptr, st, StretchIn{});
    RC_TRY(run_pipeline(c, W, c->d_skip, st));
    hipLaunchKernelGGL(k_finish_posterior, dim3(finish_blocks(W)), dim3(kFinishThreads), 0, st, c->d_partial, c->d_skip,
                       c->d_lnprior, d_lnprob, W, c->nblk, 1, 0);
    HIP_TRY(hipGetLastError());
    return PSFMC_OK;
}

static int check_call(psfmc_ctx* c, int W, const void* rows, const void* out) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (W < 0 || W > c->max_walkers)
        return fail(PSFMC_EINVAL, "W=%d outside [0, max_walkers=%d]", W, c->max_walkers);
    if (W > 0 && (!rows || !out)) return fail(PSFMC_EINVAL, "NULL buffer");
    return PSFMC_OK;
}

extern "C" int psfmc_eval_batch_device(psfmc_ctx* c, int W, const double* d_rows,
                                       const uint8_t* d_skip, double* d_like, void* stream) {
    int rc = check_call(c, W, d_rows, d_like);
    if (rc != PSFMC_OK || W == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return eval_device(c, W, d_rows, d_skip, d_like, stream ? (hipStream_t)stream : c->stream);
}

static int eval_batch_impl(psfmc_ctx* c, int field, int W, const double* rows, const uint8_t* skip, double* loglike);

extern "C" int psfmc_eval_batch(psfmc_ctx* c, int W, const double* rows, const uint8_t* skip,
                                double* loglike) {
    return eval_batch_impl(c, -1, W, rows, skip, loglike);
}

// the log-likelihoods of derived rows of ONE field of a psfmc_ctx_create_fields context (the rows' PSF index
// counts within the field, as for psfmc_eval_images_field)
extern "C" int psfmc_eval_batch_field(psfmc_ctx* c, int field, int W, const double* rows, const uint8_t* skip,
                                      double* loglike) {
    if (c && (field < 0 || field >= c->n_fields)) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    return eval_batch_impl(c, field, W, rows, skip, loglike);
}

static int eval_batch_impl(psfmc_ctx* c, int field, int W, const double* rows, const uint8_t* skip, double* loglike) {
    int rc = check_call(c, W, rows, loglike);
    if (rc != PSFMC_OK || W == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(c->d_rows, rows, (size_t)W * c->rlen * sizeof(double), hipMemcpyHostToDevice, st));
    if (skip) HIP_TRY(hipMemcpyAsync(c->d_skip, skip, (size_t)W, hipMemcpyHostToDevice, st));
    rc = eval_device(c, W, c->d_rows, skip ? c->d_skip : nullptr, c->d_like, st, field);
    if (rc != PSFMC_OK) return rc;
    HIP_TRY(hipMemcpyAsync(loglike, c->d_like, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PSFMC_OK;
}

// ---------------------------------------------------------------------------
// images (models.py:222-226)
// ---------------------------------------------------------------------------
static int ensure_image_staging(psfmc_ctx* c) {
    if (c->img_cap >= c->chunk) return PSFMC_OK;
    if (c->d_img0) { (void)hipFree(c->d_img0); c->d_img0 = nullptr; }
    if (c->d_img1) { (void)hipFree(c->d_img1); c->d_img1 = nullptr; }
    if (c->d_rawstage) { (void)hipFree(c->d_rawstage); c->d_rawstage = nullptr; }
    c->img_cap = 0;
    HIP_TRY(hipMalloc(&c->d_img0, (size_t)c->chunk * c->S * sizeof(double)));
    HIP_TRY(hipMalloc(&c->d_img1, (size_t)c->chunk * c->S * sizeof(double)));
    c->img_cap = c->chunk;
    return PSFMC_OK;
}

// The image flow, shared by psfmc_eval_images[_field] and psfmc_fisher_rows: host rows (and the aux rows the caller
// left) of W walkers of `field` -> prep records in c->d_prep, then passes of up to c->chunk walkers each.
static int images_begin(psfmc_ctx* c, int field, int W, const double* rows, hipStream_t st) {
    RC_TRY(take_aux_rows(c, W));
    HIP_TRY(hipMemcpyAsync(c->d_rows, rows, (size_t)W * c->rlen * sizeof(double), hipMemcpyHostToDevice, st));
    c->prep_tabs_valid = false;                       // d_prep is being rewritten
    hipLaunchKernelGGL(k_prep, dim3((W + 127) / 128), dim3(128), 0, st, c->d_rows, c->d_prep, W, c->n_ps,
                       c->n_sersic, c->wraps[field].ly, c->wraps[field].lx, c->d_rho, c->n_psf_field, field * c->n_psf_field);
    launch_pow_tables(c, W, 0, nullptr, st);
    return ensure_image_staging(c);
}
// One pass: the convolved model and model variance of the n walkers whose records start at `prep`, in c->d_img0 /
// c->d_img1 (fused) or interleaved in c->d_real (hipFFT: image_source).  `partial`: where the fused pass leaves the
// walkers' chi^2 partial sums.
static int image_pass(psfmc_ctx* c, int n, const double* prep, int ps_only, double* raw_dev, double* partial,
                      hipStream_t st) {
    if (c->backend == PSFMC_BACKEND_FUSED) {
        RC_TRY(fused_forward(c, n, c->d_T, prep, nullptr, ps_only, raw_dev, st));
        return fused_inverse(c, n, c->d_T, prep, nullptr, partial, c->d_img0, c->d_img1, st);
    }
    return hipfft_convolve(c, n, prep, nullptr, st, ps_only);
}

static int eval_images_impl(psfmc_ctx* c, int field, int W, const double* rows, double* raw, double* conv,
                            double* resid, double* ivm, double* ps_sub) {
    int rc = check_call(c, W, rows, rows);
    if (rc != PSFMC_OK || W == 0) return rc;
    if (field < 0 || field >= c->n_fields) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    const double* f_sci = c->d_sci + (size_t)field * c->S;      // this field's pixels
    const double* f_var = c->d_var + (size_t)field * c->S;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const bool fused = c->backend == PSFMC_BACKEND_FUSED;
    const size_t S_img = img_pixels(c, field);                  // pixels of a host image (the field's own shape)
    const size_t img = S_img * sizeof(double);
    RC_TRY(images_begin(c, field, W, rows, st));
    double *d_out = nullptr, *d_rawdev = nullptr;     // [chunk] staging for derived images / the raw models (transform shape)
    HIP_TRY(hipMalloc(&d_out, (size_t)c->chunk * img));
    if (raw && fused && hipMalloc(&d_rawdev, (size_t)c->chunk * c->S * sizeof(double)) != hipSuccess) {
        (void)hipFree(d_out);
        return fail(PSFMC_ENOMEM, "hipMalloc (raw-model staging)");
    }
    // where the convolved model / model variance of walker w live after a pass
    const double* conv_src = fused ? c->d_img0 : c->d_real;
    const double* var_src = fused ? c->d_img1 : c->d_real;
    const int stride = fused ? 1 : 2, var_c = fused ? 0 : 1;
    for (int w0 = 0; w0 < W && rc == PSFMC_OK; w0 += c->chunk) {
        const int n = W - w0 < c->chunk ? W - w0 : c->chunk;
        const double* prep = c->d_prep + (size_t)w0 * c->plen;
        auto emit = [&](double* host, const double* src, int strd, int comp, int op) -> int {
            if (!host) return PSFMC_OK;
            hipLaunchKernelGGL(k_image_out, dim3(64, n), dim3(256), 0, st, src, f_sci, f_var, d_out,
                               c->S, strd, comp, op, img_window(c, field));
            HIP_TRY(hipMemcpyAsync(host + (size_t)w0 * S_img, d_out, (size_t)n * img,
                                   hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return PSFMC_OK;
        };
        auto pass = [&](int ps_only, double* raw_dev) -> int {
            return image_pass(c, n, prep, ps_only, raw_dev, c->d_partial, st);
        };
        if (raw && !fused) {   // raw model before the inverse transform overwrites it
            hipLaunchKernelGGL(k_raster, dim3((c->S + 1023) / 1024, n), dim3(256),
                               (size_t)prep_rec_len(c->n_ps, c->n_sersic) * sizeof(double), st, prep,
                               (const uint8_t*)nullptr, c->d_real, c->n_ps, c->n_sersic, c->ny, c->nx, 0,
                               extra_image_of(c, prep));
            rc = emit(raw, c->d_real, 2, 0, IMG_COPY);
            if (rc != PSFMC_OK) break;
        }
        if (conv || resid || ivm || (raw && fused)) {
            rc = pass(0, (raw && fused) ? d_rawdev : nullptr);
            if (rc == PSFMC_OK && raw && fused) rc = emit(raw, d_rawdev, 1, 0, IMG_COPY);
            if (rc == PSFMC_OK) rc = emit(conv, conv_src, stride, 0, IMG_COPY);
            if (rc == PSFMC_OK) rc = emit(resid, conv_src, stride, 0, IMG_RESID);
            if (rc == PSFMC_OK) rc = emit(ivm, var_src, stride, var_c, IMG_IVM);
        }
        if (rc == PSFMC_OK && ps_sub) {
            rc = pass(1, nullptr);
            if (rc == PSFMC_OK) rc = emit(ps_sub, conv_src, stride, 0, IMG_RESID);
        }
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(d_out);
    if (d_rawdev) (void)hipFree(d_rawdev);
    if (rc == PSFMC_OK) HIP_TRY(hipGetLastError());
    return rc;
}

extern "C" int psfmc_eval_images(psfmc_ctx* c, int W, const double* rows, double* raw, double* conv,
                                 double* resid, double* ivm, double* ps_sub) {
    if (c && c->n_fields > 1) return fail(PSFMC_EINVAL, "this entry point serves contexts of one field");
    return eval_images_impl(c, 0, W, rows, raw, conv, resid, ivm, ps_sub);
}

// the five images of walkers of ONE field of a psfmc_ctx_create_fields context (rows as for
// psfmc_eval_images; their PSF index counts within the field)
extern "C" int psfmc_eval_images_field(psfmc_ctx* c, int field, int W, const double* rows, double* raw,
                                       double* conv, double* resid, double* ivm, double* ps_sub) {
    return eval_images_impl(c, field, W, rows, raw, conv, resid, ivm, ps_sub);
}

// ---------------------------------------------------------------------------
// raw-vector path
// ---------------------------------------------------------------------------
// no launch may read the tables, flags and masks a layout call replaces
static int layout_sync(psfmc_ctx* c) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    c->joint.ready = false;                  // (the joint layouts are copies of the fields' layouts)
    return PSFMC_OK;
}

// the device copy of the mean flags (psfmc_set_general_mean) and of the general flags less the mean components, and
// the any-bit; a context that never had a flag has neither
static int sync_mean_flags(psfmc_ctx* c) {
    bool any = false;
    for (uint8_t f : c->mean_flags) any = any || f;
    if (!any && !c->d_mean_flags) {
        c->mean_any = false;
        return PSFMC_OK;
    }
    RC_TRY(layout_sync(c));                            // (no batch in flight reads the flags)
    const size_t n = (size_t)c->n_fields * c->n_sersic;
    if (!c->d_mean_flags) HIP_TRY(hipMalloc(&c->d_mean_flags, 2 * n));
    std::vector<uint8_t> both(2 * n, 0);
    for (size_t i = 0; i < n && i < c->mean_flags.size(); ++i) {
        both[i] = c->mean_flags[i];
        both[n + i] = (i < c->gen_flags.size() && c->gen_flags[i] && !c->mean_flags[i]) ? 1 : 0;
    }
    HIP_TRY(hipMemcpy(c->d_mean_flags, both.data(), 2 * n, hipMemcpyHostToDevice));
    c->mean_any = any;
    c->prep_tabs_valid = false;                        // records written under the old flags are not to be rasterised
    return PSFMC_OK;
}
// a new layout or aux layout of a field drops its mean flags
static int drop_mean_flags(psfmc_ctx* c, int field) {
    if (c->mean_flags.empty()) return PSFMC_OK;
    for (int k = 0; k < c->n_sersic; ++k) c->mean_flags[(size_t)field * c->n_sersic + k] = 0;
    return sync_mean_flags(c);
}

// field `field`'s rows of the blocks' mask arrays from its record, the any-bits and the device copies where they
// exist.  `touched`: the block this call registers; the context has its mask array from then on.
static int write_block_masks(psfmc_ctx* c, int field, int touched = -1) {
    const FieldAuxRecord& r = c->aux_records[field];
    const size_t n_ser = c->n_sersic;
    for (int b = 0; b < kAuxBlocks; ++b) {
        const AuxBlockFacts& k = kAuxBlock[b];
        psfmc_ctx::AuxBlockState& s = c->blk[b];
        if (b == touched && s.masks.empty()) s.masks.assign((size_t)c->n_fields * n_ser, 0);
        if (s.masks.empty()) continue;
        const std::vector<int>& tags = r.block[b].tags;
        for (size_t i = 0; i < n_ser; ++i) {
            const int t = tags.empty() ? 0 : tags[i];
            s.masks[(size_t)field * n_ser + i] =
                (uint8_t)(t ? ((k.flag ? k.flag : t) | (r.sersic_degrees[i] ? k.deg_bit : 0)) : 0);
        }
        bool any = false;
        for (uint8_t m : s.masks) any = any || (m & k.any_bits);
        if (s.d_masks) HIP_TRY(hipMemcpy(s.d_masks, s.masks.data(), s.masks.size(), hipMemcpyHostToDevice));
        s.any = any;
    }
    return PSFMC_OK;
}

// A column table's entries against the field's columns and ties: -1 a constant, >= 0 a column, <= -2 tie -2 - entry
static int live_ties(const psfmc_ctx* c, int field) {
    return (size_t)field < c->ties_live.size() ? c->ties_live[field].n : 0;
}
static int check_table_entries(const char* what, const int* col, int n, int n_params, int n_ties) {
    for (int i = 0; i < n; ++i) {
        if (col[i] >= n_params) return fail(PSFMC_EINVAL, "%s %d refers to column %d of %d", what, i, col[i], n_params);
        if (col[i] <= -2 && -2 - (long long)col[i] >= n_ties)
            return fail(PSFMC_EINVAL, "%s %d refers to tie %lld of %d (psfmc_set_ties)", what, i, -2 - (long long)col[i],
                        n_ties);
    }
    return PSFMC_OK;
}

extern "C" int psfmc_set_ties(psfmc_ctx* c, int field, int n_ties, const int* src_col, const int* ratio_col,
                              const double* ratio_const, const int* offset_col, const double* offset_const) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (field < 0 || field >= c->n_fields) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    if (n_ties < 0 || n_ties > PSFMC_MAX_TIES)
        return fail(PSFMC_EINVAL, "n_ties=%d outside [0, PSFMC_MAX_TIES=%d]", n_ties, PSFMC_MAX_TIES);
    if (n_ties && (!src_col || !ratio_col || !ratio_const || !offset_col || !offset_const))
        return fail(PSFMC_EINVAL, "NULL tie array");
    for (int t = 0; t < n_ties; ++t) {
        if (src_col[t] < 0) return fail(PSFMC_EINVAL, "tie %d: source column %d", t, src_col[t]);
        if (ratio_col[t] < -1 || offset_col[t] < -1)
            return fail(PSFMC_EINVAL, "tie %d: ratio column %d, offset column %d (-1: the constant)", t, ratio_col[t],
                        offset_col[t]);
        if (!std::isfinite(ratio_const[t]) || !std::isfinite(offset_const[t]))
            return fail(PSFMC_EINVAL, "tie %d: ratio %g, offset %g: the constants must be finite", t, ratio_const[t],
                        offset_const[t]);
    }
    if (c->ties_live.empty()) {
        if (!n_ties) return PSFMC_OK;                  // (a context that never had a tie stays what it was)
        c->ties_live.assign(c->n_fields, psfmc_ctx::TieRecord{});
        c->ties_next.assign(c->n_fields, psfmc_ctx::TieRecord{});
        c->ties_dirty.assign(c->n_fields, 0);
    }
    HIP_TRY(hipSetDevice(c->device));
    psfmc_ctx::TieRecord& r = c->ties_next[field];     // (no layout points to it: no launch reads its blob)
    if (r.blob) (void)hipFree(r.blob);
    r = psfmc_ctx::TieRecord{};
    c->ties_dirty[field] = 1;
    if (!n_ties) return PSFMC_OK;
    r.n = n_ties;
    r.col.insert(r.col.end(), src_col, src_col + n_ties);
    r.col.insert(r.col.end(), ratio_col, ratio_col + n_ties);
    r.col.insert(r.col.end(), offset_col, offset_col + n_ties);
    r.konst.insert(r.konst.end(), ratio_const, ratio_const + n_ties);
    r.konst.insert(r.konst.end(), offset_const, offset_const + n_ties);
    const size_t cb = r.konst.size() * sizeof(double), ib = r.col.size() * sizeof(int);
    std::vector<unsigned char> blob(cb + ib);
    memcpy(blob.data(), r.konst.data(), cb);
    memcpy(blob.data() + cb, r.col.data(), ib);
    HIP_TRY(hipMalloc(&r.blob, blob.size()));
    HIP_TRY(hipMemcpy(r.blob, blob.data(), blob.size(), hipMemcpyHostToDevice));
    return PSFMC_OK;
}

// Make field `field`'s record live: its table composed afresh (psfmc_aux_table.h) in a new blob, the layout's counts
// and pointers, the mask rows, and -- the first time the context needs them -- longer auxiliary vectors (the entries
// they hold keep their places; aux_stride only grows) and the blocks' masks and parameter buffers, all clear.
static int apply_aux_record(psfmc_ctx* c, int field, int touched = -1) {
    RC_TRY(layout_sync(c));
    ThetaLayout& L = c->layouts[field];
    const FieldAuxRecord& r = c->aux_records[field];
    const AuxTable t = compose_aux_table(r, L.n_sky, c->n_sersic);
    void* fresh = nullptr;
    if (t.n_aux) {
        // konst first (8-byte units), then col and, behind the columns, the kinds and the truncation sides
        const size_t cb = t.konst.size() * sizeof(double), ib = t.col.size() * sizeof(int);
        const size_t kb = t.kinds.size() * sizeof(int);
        std::vector<unsigned char> blob(cb + ib + kb + t.sides.size() * sizeof(int));
        memcpy(blob.data(), t.konst.data(), cb);
        memcpy(blob.data() + cb, t.col.data(), ib);
        if (!t.kinds.empty()) memcpy(blob.data() + cb + ib, t.kinds.data(), kb);
        if (!t.sides.empty()) memcpy(blob.data() + cb + ib + kb, t.sides.data(), t.sides.size() * sizeof(int));
        HIP_TRY(hipMalloc(&fresh, blob.size()));
        HIP_TRY(hipMemcpy(fresh, blob.data(), blob.size(), hipMemcpyHostToDevice));
    }
    if (c->aux_blobs.size() != (size_t)c->n_fields) c->aux_blobs.assign(c->n_fields, nullptr);
    if (c->aux_blobs[field]) (void)hipFree(c->aux_blobs[field]);
    c->aux_blobs[field] = fresh;
    L.n_aux = t.n_aux; L.n_fou = t.n_fou; L.n_spi = t.n_spi; L.n_rad = t.n_rad; L.n_tru = t.n_tru;
    L.n_bnd = t.n_bnd;
    L.aux_const = static_cast<const double*>(fresh);
    L.aux_col = fresh ? reinterpret_cast<const int*>(L.aux_const + t.n_aux) : nullptr;
    L.rad_kind = t.kinds.empty() ? nullptr : L.aux_col + t.n_aux;
    L.tru_side = t.sides.empty() ? nullptr : L.aux_col + t.n_aux + t.kinds.size();
    if (c->n_fields > 1 && c->d_field_layouts)
        HIP_TRY(hipMemcpy(c->d_field_layouts + field, &L, sizeof(ThetaLayout), hipMemcpyHostToDevice));
    if (t.n_aux > c->aux_stride) {           // (a table index is the entry's place in the walker's vector)
        double* longer = nullptr;
        HIP_TRY(hipMalloc(&longer, (size_t)c->max_walkers * t.n_aux * sizeof(double)));
        HIP_TRY(hipMemset(longer, 0, (size_t)c->max_walkers * t.n_aux * sizeof(double)));
        if (c->d_aux) (void)hipFree(c->d_aux);
        c->d_aux = longer;
        c->aux_stride = t.n_aux;
    }
    const size_t n_masks = (size_t)c->n_fields * c->n_sersic;
    for (int b = 0; b < kAuxBlocks; ++b)
        for (int j = kAuxBlock[b].first; !r.block[b].empty() && j <= b; ++j) {
            psfmc_ctx::AuxBlockState& s = c->blk[j];
            if (s.d_masks) continue;
            const size_t par_bytes = ((size_t)c->max_walkers * c->n_sersic * kAuxBlock[j].par + 1) * sizeof(double);
            if (s.masks.empty()) s.masks.assign(n_masks, 0);
            HIP_TRY(hipMalloc(&s.d_masks, n_masks));
            HIP_TRY(hipMalloc(&s.d_par, par_bytes));
            HIP_TRY(hipMemset(s.d_par, 0, par_bytes));
        }
    RC_TRY(write_block_masks(c, field, touched));
    c->aux_rows_w = -1;
    c->prep_tabs_valid = false;              // records written under the old flags and masks are not to be rasterised
    return PSFMC_OK;
}

static int set_layout_impl(psfmc_ctx* c, int field, int n_sky, int n_params, const int* slot_col,
                           const double* slot_const, const int* ps_method, const int* sersic_degrees,
                           double mag_zeropoint, const int* family, const double* p0,
                           const double* p1, const double* p2) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (field < 0 || field >= c->n_fields) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    if (field > 0 && (!c->has_layout[0] || n_sky != c->layouts[0].n_sky || n_params != c->layouts[0].n_params))
        return fail(PSFMC_EINVAL, "set field 0's layout first; every field has the same slots and columns");
    if (n_sky < 0 || n_sky > 16 || n_params < 0 || n_params > 4096) return fail(PSFMC_EINVAL, "bad counts");
    if (c->d_aux && n_sky != c->aux_n_sky)
        return fail(PSFMC_EINVAL, "n_sky=%d: the context's auxiliary vectors were allocated for %d skies "
                    "(psfmc_set_aux_layout); a layout with another number of skies needs a new context", n_sky,
                    c->aux_n_sky);
    const int ns = n_slots(n_sky, c->n_ps, c->n_sersic);
    if (!slot_col || !slot_const || (c->n_ps && !ps_method) || (c->n_sersic && !sersic_degrees) ||
        (n_params && (!family || !p0 || !p1 || !p2)))
        return fail(PSFMC_EINVAL, "NULL layout array");
    // the ties this layout will stand on: those registered since the field's last layout, else the live ones
    const bool new_ties = !c->ties_dirty.empty() && c->ties_dirty[field];
    const psfmc_ctx::TieRecord none{};
    const psfmc_ctx::TieRecord& tr = new_ties ? c->ties_next[field] : (c->ties_live.empty() ? none : c->ties_live[field]);
    RC_TRY(check_table_entries("slot", slot_col, ns, n_params, tr.n));
    if (slot_col[ns - 1] <= -2) return fail(PSFMC_EINVAL, "slot %d, the PSF index, cannot be tied", ns - 1);
    for (int t = 0; t < tr.n; ++t)
        if (tr.col[t] >= n_params || tr.col[tr.n + t] >= n_params || tr.col[2 * tr.n + t] >= n_params)
            return fail(PSFMC_EINVAL, "tie %d: source column %d, ratio column %d, offset column %d of %d", t,
                        tr.col[t], tr.col[tr.n + t], tr.col[2 * tr.n + t], n_params);
    for (int i = 0; i < n_params; ++i)
        if (family[i] < 0 || family[i] > PRIOR_RANDINT)
            return fail(PSFMC_EINVAL, "unknown prior family %d for column %d", family[i], i);
    RC_TRY(layout_sync(c));
    // pack everything into one device allocation (8-byte units)
    const size_t n_int = (size_t)ns + c->n_ps + c->n_sersic + n_params;
    const size_t n_dbl = (size_t)ns + 5 * (size_t)n_params;         // slot constants, pa, pb, pc, pd (0 here), pk
    const size_t int_bytes = (n_int * sizeof(int) + 7) / 8 * 8;
    std::vector<unsigned char> blob(int_bytes + n_dbl * sizeof(double));
    int* ip = reinterpret_cast<int*>(blob.data());
    double* dp = reinterpret_cast<double*>(blob.data() + int_bytes);
    memcpy(ip, slot_col, ns * sizeof(int));
    if (c->n_ps) memcpy(ip + ns, ps_method, c->n_ps * sizeof(int));
    if (c->n_sersic) memcpy(ip + ns + c->n_ps, sersic_degrees, c->n_sersic * sizeof(int));
    if (n_params) memcpy(ip + ns + c->n_ps + c->n_sersic, family, n_params * sizeof(int));
    memcpy(dp, slot_const, ns * sizeof(double));
    if (n_params) {
        memcpy(dp + ns, p0, n_params * sizeof(double));
        memcpy(dp + ns + n_params, p1, n_params * sizeof(double));
        memcpy(dp + ns + 2 * n_params, p2, n_params * sizeof(double));
        for (int i = 0; i < n_params; ++i) dp[ns + 4 * n_params + i] = prior_log_norm(family[i], p0[i], p1[i], p2[i]);
    }
    void** blob_slot = &c->layout_blobs[field];
    if (*blob_slot) { (void)hipFree(*blob_slot); *blob_slot = nullptr; }
    HIP_TRY(hipMalloc(blob_slot, blob.size()));
    HIP_TRY(hipMemcpy(*blob_slot, blob.data(), blob.size(), hipMemcpyHostToDevice));
    const int* dip = reinterpret_cast<const int*>(*blob_slot);
    const double* ddp = reinterpret_cast<const double*>(static_cast<unsigned char*>(*blob_slot) + int_bytes);
    ThetaLayout& L = c->layouts[field];
    // (a new layout has no auxiliary parameters until psfmc_set_aux_layout names them again, and no modes, spirals
    // or laws: the record keeps only the degrees)
    L = ThetaLayout{};
    c->aux_records[field] = FieldAuxRecord{};
    c->aux_records[field].sersic_degrees.assign(sersic_degrees, sersic_degrees + c->n_sersic);
    L.n_sky = n_sky; L.n_ps = c->n_ps; L.n_sersic = c->n_sersic; L.n_params = n_params; L.n_psf = c->n_psf_field;
    L.mag_zp = mag_zeropoint;
    L.slot_col = dip; L.ps_method = dip + ns; L.sersic_deg = dip + ns + c->n_ps;
    L.family = dip + ns + c->n_ps + c->n_sersic;
    L.slot_const = ddp; L.pa = ddp + ns; L.pb = ddp + ns + n_params; L.pc = ddp + ns + 2 * n_params;
    L.pd = ddp + ns + 3 * n_params; L.pk = ddp + ns + 4 * n_params;
    if (new_ties) {                          // (after layout_sync: no launch reads the blob being freed)
        if (c->ties_live[field].blob) (void)hipFree(c->ties_live[field].blob);
        c->ties_live[field] = std::move(c->ties_next[field]);
        c->ties_next[field] = psfmc_ctx::TieRecord{};
        c->ties_dirty[field] = 0;
    }
    if (live_ties(c, field)) {
        L.n_ties = c->ties_live[field].n;
        L.tie_const = static_cast<const double*>(c->ties_live[field].blob);
        L.tie_col = reinterpret_cast<const int*>(L.tie_const + 2 * L.n_ties);
    }
    RC_TRY(write_block_masks(c, field));
    if (!c->d_aux) c->gen_flags.clear();     // (no flag was ever set; psfmc_set_aux_layout sizes them for its n_sky)
    if (!c->gen_flags.empty()) {
        const size_t n_ser = c->n_sersic, n_sk = c->aux_n_sky;
        for (size_t k = 0; k < n_ser; ++k) c->gen_flags[(size_t)field * n_ser + k] = 0;
        for (size_t k = 0; k < n_sk; ++k) c->gen_flags[(size_t)c->n_fields * n_ser + (size_t)field * n_sk + k] = 0;
        bool any = false;
        for (uint8_t f : c->gen_flags) any = any || f;
        if (c->d_gen_flags)
            HIP_TRY(hipMemcpy(c->d_gen_flags, c->gen_flags.data(), c->gen_flags.size(), hipMemcpyHostToDevice));
        c->gen_any = any;
    }
    RC_TRY(drop_mean_flags(c, field));
    if (c->n_fields > 1) {
        if (!c->d_field_layouts) HIP_TRY(hipMalloc(&c->d_field_layouts, (size_t)c->n_fields * sizeof(ThetaLayout)));
        HIP_TRY(hipMemcpy(c->d_field_layouts + field, &L, sizeof(ThetaLayout), hipMemcpyHostToDevice));
    }
    if (field == 0) {                        // (the walkers' staging, sized by the columns every field shares)
        for (double** p : {&c->d_theta, &c->d_extra, &c->d_lnprior})
            if (*p) { (void)hipFree(*p); *p = nullptr; }
        HIP_TRY(hipMalloc(&c->d_theta, (size_t)c->max_walkers * (n_params > 0 ? n_params : 1) * sizeof(double)));
        HIP_TRY(hipMalloc(&c->d_extra, (size_t)c->max_walkers * sizeof(double)));
        HIP_TRY(hipMalloc(&c->d_lnprior, (size_t)c->max_walkers * sizeof(double)));
        c->theta_lds = theta_prep_lds_bytes(n_sky, c->n_ps, c->n_sersic, n_params);
        if (c->theta_lds > 64 * 1024) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_theta_prep),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->theta_lds));
        }
    }
    c->has_layout[field] = 1;
    return PSFMC_OK;
}

extern "C" int psfmc_set_layout(psfmc_ctx* c, int n_sky, int n_params, const int* slot_col,
                                const double* slot_const, const int* ps_method, const int* sersic_degrees,
                                double mag_zeropoint, const int* family, const double* p0,
                                const double* p1, const double* p2) {
    return set_layout_impl(c, 0, n_sky, n_params, slot_col, slot_const, ps_method, sersic_degrees, mag_zeropoint,
                           family, p0, p1, p2);
}

// Replace field `field`'s prior table: family [n_params], params [n_params][PSFMC_PRIOR_NPAR] (scipy's
// arguments in order).  Everything is checked before anything is written, so a refused table leaves the
// previous one in force.  The tables sit in the layout blob (L.family, and L.pa ... L.pk back to back),
// which keeps its place: the device copies of the layouts stay valid.
static_assert(kPriorNpar == PSFMC_PRIOR_NPAR && PRIOR_TRUNCNORM == PSFMC_PRIOR_TRUNCNORM &&
              PRIOR_INVGAMMA == PSFMC_PRIOR_INVGAMMA && PRIOR_N_FAMILIES == PSFMC_PRIOR_INVGAMMA + 1,
              "prior codes of include/psfmc_hip.h");
// the checked device form of a prior table: tab = pa | pb | pc | pd | pk, n_params each
static int prior_table(int n_params, const int* family, const double* params, std::vector<double>& tab) {
    if (!family || !params) return fail(PSFMC_EINVAL, "NULL prior table");
    tab.assign(5 * (size_t)n_params, 0.0);
    for (int i = 0; i < n_params; ++i) {
        const double* p = params + (size_t)kPriorNpar * i;
        if (family[i] < 0 || family[i] >= PRIOR_N_FAMILIES)
            return fail(PSFMC_EINVAL, "unknown prior family %d for column %d", family[i], i);
        if (!prior_params_ok(family[i], p))
            return fail(PSFMC_EINVAL, "column %d: parameters (%g, %g, %g, %g) invalid for prior family %d", i, p[0],
                        p[1], p[2], p[3], family[i]);
        double e[5];
        prior_prepare(family[i], p, e);
        for (int j = 0; j < 5; ++j) tab[(size_t)j * n_params + i] = e[j];
    }
    return PSFMC_OK;
}

static int ensure_extra_images(psfmc_ctx* c, const char* what);
extern "C" int psfmc_set_sersic_integrate(psfmc_ctx* c, int field, int n_sersic, const int* integrate) {
    if (!c || !integrate) return fail(PSFMC_EINVAL, "NULL argument");
    if (field < 0 || field >= c->n_fields) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    if (n_sersic != c->n_sersic) return fail(PSFMC_EINVAL, "n_sersic=%d, the context has %d", n_sersic, c->n_sersic);
    HIP_TRY(hipSetDevice(c->device));
    for (int k = 0; k < n_sersic; ++k)
        if (integrate[k] && !c->gen_flags.empty() && c->gen_flags[(size_t)field * n_sersic + k])
            return fail(PSFMC_EINVAL, "Sersic %d of field %d has a boxiness: boxiness and integrate exclude each other", k,
                        field);
    if (c->integ_flags.empty()) c->integ_flags.assign((size_t)c->n_fields * c->n_sersic, 0);
    for (int k = 0; k < n_sersic; ++k) c->integ_flags[(size_t)field * n_sersic + k] = integrate[k] ? 1 : 0;
    bool any = false;
    for (uint8_t f : c->integ_flags) any = any || f;
    if (any && !c->d_integ_flags) {
        HIP_TRY(hipMalloc(&c->d_integ_flags, c->integ_flags.size()));
        HIP_TRY(hipMalloc(&c->d_integ_par, (size_t)c->max_walkers * c->n_sersic * kPrepSersic * sizeof(double)));
        RC_TRY(ensure_extra_images(c, "integrated-profile"));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));          // (no batch in flight reads the flags)
    if (c->d_integ_flags)
        HIP_TRY(hipMemcpy(c->d_integ_flags, c->integ_flags.data(), c->integ_flags.size(), hipMemcpyHostToDevice));
    c->integ_any = any;
    c->prep_tabs_valid = false;                        // records written under the old flags are not to be rasterised
    return PSFMC_OK;
}

// the extra images (and nothing else) of a context that just got its first integrated / general flag
static int ensure_extra_images(psfmc_ctx* c, const char* what) {
    if (c->d_extra_img) return PSFMC_OK;
    if (hipMalloc(&c->d_extra_img, (size_t)c->max_walkers * c->S * sizeof(double)) != hipSuccess)
        return fail(PSFMC_ENOMEM, "hipMalloc (%s images: %d walkers x %d pixels)", what, c->max_walkers, c->S);
    return PSFMC_OK;
}

extern "C" int psfmc_set_aux_layout(psfmc_ctx* c, int field, int n_aux, const int* aux_col, const double* aux_const,
                                    const int* sky_slope_flags, const int* sersic_general_flags) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (field < 0 || field >= c->n_fields) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    if (!c->has_layout[field]) return fail(PSFMC_EINVAL, "field %d has no layout yet (psfmc_set_layout[_field])", field);
    ThetaLayout& L = c->layouts[field];
    const int want = aux_len(L.n_sky, c->n_sersic);
    if (n_aux != 0 && n_aux != want)
        return fail(PSFMC_EINVAL, "n_aux=%d: a layout of %d skies and %d Sersics has 2 x %d + %d", n_aux, L.n_sky,
                    c->n_sersic, L.n_sky, c->n_sersic);
    if (n_aux && (!aux_col || !aux_const || (L.n_sky && !sky_slope_flags) || (c->n_sersic && !sersic_general_flags)))
        return fail(PSFMC_EINVAL, "NULL aux array");
    RC_TRY(check_table_entries("aux value", aux_col, n_aux, L.n_params, live_ties(c, field)));
    for (int k = 0; n_aux && k < c->n_sersic; ++k)
        if (sersic_general_flags[k] && !c->integ_flags.empty() && c->integ_flags[(size_t)field * c->n_sersic + k])
            return fail(PSFMC_EINVAL, "Sersic %d of field %d is pixel-integrated: boxiness and integrate exclude each other",
                        k, field);
    if (c->d_aux && n_aux && (want != c->aux_base || L.n_sky != c->aux_n_sky))
        return fail(PSFMC_EINVAL, "n_aux=%d: the context's auxiliary vectors were allocated with %d values per walker",
                    n_aux, c->aux_base);
    // (the field's modes, spirals and laws are registered after its aux layout: a new one drops them)
    FieldAuxRecord& r = c->aux_records[field];
    r.base_col.assign(aux_col, aux_col + n_aux);
    r.base_const.assign(aux_const, aux_const + n_aux);
    for (AuxBlockRecord& blk : r.block) blk.clear();
    const bool first = n_aux && !c->d_aux;             // (every layout with n_aux > 0 writes aux vectors)
    RC_TRY(apply_aux_record(c, field));
    const int n_sky = L.n_sky, n_ser = c->n_sersic;
    const size_t n_flags = (size_t)c->n_fields * (n_ser + n_sky);
    if (c->gen_flags.size() != n_flags) c->gen_flags.assign(n_flags, 0);
    uint8_t* ser_fl = c->gen_flags.data() + (size_t)field * n_ser;
    uint8_t* sky_fl = c->gen_flags.data() + (size_t)c->n_fields * n_ser + (size_t)field * n_sky;
    for (int k = 0; k < n_ser; ++k) ser_fl[k] = n_aux && sersic_general_flags[k] ? 1 : 0;
    for (int k = 0; k < n_sky; ++k) sky_fl[k] = n_aux && sky_slope_flags[k] ? 1 : 0;
    bool any = false;
    for (uint8_t f : c->gen_flags) any = any || f;
    if (first) {
        c->aux_base = want;
        c->aux_n_sky = n_sky;
        HIP_TRY(hipMalloc(&c->d_gen_flags, n_flags));
        HIP_TRY(hipMalloc(&c->d_gen_par, ((size_t)c->max_walkers * n_ser * kGenPar + 1) * sizeof(double)));
    }
    if (any) RC_TRY(ensure_extra_images(c, "general-component"));
    if (c->d_gen_flags)
        HIP_TRY(hipMemcpy(c->d_gen_flags, c->gen_flags.data(), n_flags, hipMemcpyHostToDevice));
    c->gen_any = any;
    return drop_mean_flags(c, field);
}

extern "C" int psfmc_set_general_mean(psfmc_ctx* c, int field, int n_sersic, const int* flags) {
    if (!c || !flags) return fail(PSFMC_EINVAL, "NULL argument");
    if (field < 0 || field >= c->n_fields) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    if (n_sersic != c->n_sersic) return fail(PSFMC_EINVAL, "n_sersic=%d, the context has %d", n_sersic, c->n_sersic);
    bool any_here = false;
    for (int k = 0; k < n_sersic; ++k) any_here = any_here || flags[k];
    if (any_here && c->aux_records[field].base_col.empty())
        return fail(PSFMC_EINVAL, "field %d has no aux layout: call psfmc_set_aux_layout (with the mean components "
                    "flagged general) before psfmc_set_general_mean", field);
    for (int k = 0; k < n_sersic; ++k) {
        if (!flags[k]) continue;
        if (!c->integ_flags.empty() && c->integ_flags[(size_t)field * n_sersic + k])
            return fail(PSFMC_EINVAL, "Sersic %d of field %d is pixel-integrated: pixel_mean and integrate exclude each "
                        "other", k, field);
        if (c->gen_flags.empty() || !c->gen_flags[(size_t)field * n_sersic + k])
            return fail(PSFMC_EINVAL, "Sersic %d of field %d is not flagged general in the field's aux layout: the pixel "
                        "mean is a general component's", k, field);
    }
    if (!any_here && c->mean_flags.empty()) return PSFMC_OK;           // (nothing registered, nothing to remove)
    if (c->mean_flags.empty()) c->mean_flags.assign((size_t)c->n_fields * n_sersic, 0);
    for (int k = 0; k < n_sersic; ++k) c->mean_flags[(size_t)field * n_sersic + k] = flags[k] ? 1 : 0;
    return sync_mean_flags(c);
}

extern "C" int psfmc_set_aux_rows(psfmc_ctx* c, int W, const double* aux) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (!c->gen_any) return fail(PSFMC_EINVAL, "the context has no auxiliary parameters (psfmc_set_aux_layout)");
    if (W < 0 || W > c->max_walkers) return fail(PSFMC_EINVAL, "W=%d outside [0, max_walkers=%d]", W, c->max_walkers);
    if (W > 0 && !aux) return fail(PSFMC_EINVAL, "NULL aux rows");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));          // (no batch in flight reads d_aux)
    if (W) HIP_TRY(hipMemcpy(c->d_aux, aux, (size_t)W * c->aux_stride * sizeof(double), hipMemcpyHostToDevice));
    c->aux_rows_w = W;
    return PSFMC_OK;
}

// psfmc_set_fourier_layout, _spiral_layout, _radial_layout, _truncation_layout and _bending_layout: block b of field
// `field` with its per-Sersic tags.
// Everything is checked before the record changes, so a refused call leaves the field as it was.
static int set_block_layout(psfmc_ctx* c, int b, int field, int n_sersic, const int* tags, const int* col,
                            const double* konst) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (field < 0 || field >= c->n_fields) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    if (n_sersic != c->n_sersic) return fail(PSFMC_EINVAL, "n_sersic=%d, the context has %d", n_sersic, c->n_sersic);
    const AuxBlockFacts& k = kAuxBlock[b];
    if (n_sersic && (!tags || !col || !konst)) return fail(PSFMC_EINVAL, "NULL %s array", k.name);
    if (!c->has_layout[field]) return fail(PSFMC_EINVAL, "field %d has no layout yet (psfmc_set_layout[_field])", field);
    const ThetaLayout& L = c->layouts[field];
    FieldAuxRecord& r = c->aux_records[field];
    bool any_here = false;
    for (int i = 0; i < n_sersic; ++i) {
        if (b == kBlkFou && (tags[i] & ~kFouModeBits))
            return fail(PSFMC_EINVAL, "Sersic %d: mode mask 0x%x names a mode outside 1 ... %d", i, tags[i], kFouModes);
        if (b == kBlkRad && (tags[i] < 0 || tags[i] > kRadFerrer))
            return fail(PSFMC_EINVAL, "Sersic %d: radial kind %d outside 0 ... %d", i, tags[i], kRadFerrer);
        if (b == kBlkTru && (tags[i] & ~(kTruInner | kTruOuter)))
            return fail(PSFMC_EINVAL, "Sersic %d: truncation flags %d outside 0 ... %d (bit 0 inner, bit 1 outer)", i,
                        tags[i], kTruInner | kTruOuter);
        if (b == kBlkBnd && (tags[i] & ~kBndModeBits))
            return fail(PSFMC_EINVAL, "Sersic %d: bending mask 0x%x names a mode outside 1 ... %d", i, tags[i], kBndModes);
        any_here = any_here || tags[i];
    }
    if (any_here && r.base_col.empty())
        return fail(PSFMC_EINVAL, "field %d has no aux layout: call psfmc_set_aux_layout (with the components that have "
                    "%s flagged general) before psfmc_set_%s_layout", field, k.what, k.name);
    for (int i = 0; i < n_sersic; ++i) {
        if (!tags[i]) continue;
        if (!c->integ_flags.empty() && c->integ_flags[(size_t)field * n_sersic + i])
            return fail(PSFMC_EINVAL, "Sersic %d of field %d is pixel-integrated: %s and integrate exclude each other", i,
                        field, k.excl);
        if (c->gen_flags.empty() || !c->gen_flags[(size_t)field * n_sersic + i])
            return fail(PSFMC_EINVAL, "Sersic %d of field %d has %s but is not flagged general in the field's aux layout",
                        i, field, k.what);
    }
    const int len = aux_block_len(b, n_sersic);
    if (any_here) {
        char what[32];
        snprintf(what, sizeof(what), "%s value", k.name);
        RC_TRY(check_table_entries(what, col, len, L.n_params, live_ties(c, field)));
    }
    // (a field's blocks are registered in table order: a call drops the blocks behind its own with their entries)
    bool behind = false;
    for (int j = b + 1; j < kAuxBlocks; ++j) behind = behind || !r.block[j].empty();
    if (!any_here && c->blk[b].masks.empty() && !behind) return layout_sync(c);    // (nothing registered, nothing to remove)
    r.block[b].store(n_sersic, len, tags, col, konst);
    for (int j = b + 1; j < kAuxBlocks; ++j) r.block[j].clear();
    return apply_aux_record(c, field, b);
}

extern "C" int psfmc_set_fourier_layout(psfmc_ctx* c, int field, int n_sersic, const int* mode_mask, const int* col,
                                        const double* konst) {
    return set_block_layout(c, kBlkFou, field, n_sersic, mode_mask, col, konst);
}

extern "C" int psfmc_set_spiral_layout(psfmc_ctx* c, int field, int n_sersic, const int* flags, const int* col,
                                       const double* konst) {
    return set_block_layout(c, kBlkSpi, field, n_sersic, flags, col, konst);
}

extern "C" int psfmc_set_radial_layout(psfmc_ctx* c, int field, int n_sersic, const int* kinds, const int* col,
                                       const double* konst) {
    return set_block_layout(c, kBlkRad, field, n_sersic, kinds, col, konst);
}

extern "C" int psfmc_set_truncation_layout(psfmc_ctx* c, int field, int n_sersic, const int* flags, const int* col,
                                           const double* konst) {
    return set_block_layout(c, kBlkTru, field, n_sersic, flags, col, konst);
}

extern "C" int psfmc_set_bending_layout(psfmc_ctx* c, int field, int n_sersic, const int* mode_mask, const int* col,
                                        const double* konst) {
    return set_block_layout(c, kBlkBnd, field, n_sersic, mode_mask, col, konst);
}

extern "C" int psfmc_debug_aux_table(int n_sky, int n_sersic, const int* base_col, const double* base_const,
                                     const int* mode_mask, const int* fou_col, const double* fou_const,
                                     const int* spi_flags, const int* spi_col, const double* spi_const,
                                     const int* rad_kinds, const int* rad_col, const double* rad_const,
                                     double* out_const, int* out_col, int* out_kinds, int* counts) {
    return psfmc_debug_aux_table_blocks(n_sky, n_sersic, base_col, base_const, mode_mask, fou_col, fou_const,
                                        spi_flags, spi_col, spi_const, rad_kinds, rad_col, rad_const, nullptr, nullptr,
                                        nullptr, out_const, out_col, out_kinds, nullptr, counts);
}

// ... with the truncation block: out_sides and counts[4] are written where tru_flags is given
extern "C" int psfmc_debug_aux_table_blocks(int n_sky, int n_sersic, const int* base_col, const double* base_const,
                                            const int* mode_mask, const int* fou_col, const double* fou_const,
                                            const int* spi_flags, const int* spi_col, const double* spi_const,
                                            const int* rad_kinds, const int* rad_col, const double* rad_const,
                                            const int* tru_flags, const int* tru_col, const double* tru_const,
                                            double* out_const, int* out_col, int* out_kinds, int* out_sides,
                                            int* counts) {
    return psfmc_debug_aux_table_bending(n_sky, n_sersic, base_col, base_const, mode_mask, fou_col, fou_const, spi_flags,
                                         spi_col, spi_const, rad_kinds, rad_col, rad_const, tru_flags, tru_col,
                                         tru_const, nullptr, nullptr, nullptr, out_const, out_col, out_kinds, out_sides,
                                         nullptr, counts);
}

// ... and with the bending block: out_bends and counts[5] are written where bnd_mask is given, out_sides and counts[4]
// where tru_flags or bnd_mask is
extern "C" int psfmc_debug_aux_table_bending(int n_sky, int n_sersic, const int* base_col, const double* base_const,
                                             const int* mode_mask, const int* fou_col, const double* fou_const,
                                             const int* spi_flags, const int* spi_col, const double* spi_const,
                                             const int* rad_kinds, const int* rad_col, const double* rad_const,
                                             const int* tru_flags, const int* tru_col, const double* tru_const,
                                             const int* bnd_mask, const int* bnd_col, const double* bnd_const,
                                             double* out_const, int* out_col, int* out_kinds, int* out_sides,
                                             int* out_bends, int* counts) {
    if (n_sky < 0 || n_sersic < 0 || !out_const || !out_col || !out_kinds || !counts ||
        ((tru_flags || bnd_mask) && !out_sides) || (bnd_mask && !out_bends))
        return fail(PSFMC_EINVAL, "bad counts or NULL output");
    FieldAuxRecord r;
    if (base_col && base_const) {
        r.base_col.assign(base_col, base_col + aux_len(n_sky, n_sersic));
        r.base_const.assign(base_const, base_const + aux_len(n_sky, n_sersic));
    }
    const int* tags[kAuxBlocks] = {mode_mask, spi_flags, rad_kinds, tru_flags, bnd_mask};
    const int* col[kAuxBlocks] = {fou_col, spi_col, rad_col, tru_col, bnd_col};
    const double* konst[kAuxBlocks] = {fou_const, spi_const, rad_const, tru_const, bnd_const};
    for (int b = 0; b < kAuxBlocks; ++b)
        if (tags[b] && col[b] && konst[b]) r.block[b].store(n_sersic, aux_block_len(b, n_sersic), tags[b], col[b], konst[b]);
    const AuxTable t = compose_aux_table(r, n_sky, n_sersic);
    std::copy(t.konst.begin(), t.konst.end(), out_const);
    std::copy(t.col.begin(), t.col.end(), out_col);
    std::copy(t.kinds.begin(), t.kinds.end(), out_kinds);
    counts[0] = t.n_aux; counts[1] = t.n_fou; counts[2] = t.n_spi; counts[3] = t.n_rad;
    if (tru_flags || bnd_mask) {
        std::copy(t.sides.begin(), t.sides.end(), out_sides);
        counts[4] = t.n_tru;
    }
    if (bnd_mask) {
        std::copy(t.bends.begin(), t.bends.end(), out_bends);
        counts[5] = t.n_bnd;
    }
    return PSFMC_OK;
}

extern "C" int psfmc_set_priors(psfmc_ctx* c, int field, int n_params, const int* family, const double* params) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (field < 0 || field >= c->n_fields) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    if (!c->has_layout[field]) return fail(PSFMC_EINVAL, "field %d has no layout yet (psfmc_set_layout[_field])", field);
    ThetaLayout& L = c->layouts[field];
    if (n_params != L.n_params)
        return fail(PSFMC_EINVAL, "%d prior columns for a layout of %d", n_params, L.n_params);
    if (n_params == 0) return PSFMC_OK;
    std::vector<double> tab;
    RC_TRY(prior_table(n_params, family, params, tab));
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());                          // no launch may read the tables being replaced
    HIP_TRY(hipMemcpy(const_cast<int*>(L.family), family, n_params * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(const_cast<double*>(L.pa), tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    return PSFMC_OK;
}

// the layout of one field of a psfmc_ctx_create_fields context (field 0 first; the same slot / column
// structure for every field, their own constants and priors)
extern "C" int psfmc_set_layout_field(psfmc_ctx* c, int field, int n_sky, int n_params, const int* slot_col,
                                      const double* slot_const, const int* ps_method, const int* sersic_degrees,
                                      double mag_zeropoint, const int* family, const double* p0,
                                      const double* p1, const double* p2) {
    return set_layout_impl(c, field, n_sky, n_params, slot_col, slot_const, ps_method, sersic_degrees,
                           mag_zeropoint, family, p0, p1, p2);
}

static int check_theta_call(psfmc_ctx* c, int W, const void* theta, const void* out) {
    RC_TRY(check_call(c, W, theta ? theta : out, out));
    if (!c->has_layout[0]) return fail(PSFMC_EINVAL, "psfmc_set_layout has not been called");
    if (W > 0 && c->layouts[0].n_params > 0 && !theta) return fail(PSFMC_EINVAL, "NULL theta");
    return PSFMC_OK;
}

extern "C" int psfmc_eval_theta_device(psfmc_ctx* c, int W, const double* d_theta, const double* d_extra,
                                       double* d_lnprob, void* stream) {
    int rc = check_theta_call(c, W, d_theta, d_lnprob);
    if (rc != PSFMC_OK || W == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return eval_theta_device(c, W, d_theta, d_extra, d_lnprob, stream ? (hipStream_t)stream : c->stream);
}

// psfmc_eval_theta_device_fields (below) up to the pipeline pass: the segments checked, their records derived,
// their partial sums in c->d_partial.  d_out: the caller's result buffer (checked only).  *n_w: the walkers in
// all (0: nothing was enqueued)
static int fields_records_pass(psfmc_ctx* c, int n_seg, const int* seg_field, const int* seg_count,
                               const double* d_theta, const double* d_extra, const void* d_out, hipStream_t st,
                               int* n_w) {
    *n_w = 0;
    if (!c || n_seg < 0 || (n_seg && (!seg_field || !seg_count))) return fail(PSFMC_EINVAL, "bad segment list");
    if (!c->has_layout[0]) return fail(PSFMC_EINVAL, "psfmc_set_layout has not been called");
    long long W = 0;
    for (int i = 0; i < n_seg; ++i) {
        if (seg_count[i] < 0 || seg_field[i] < 0 || seg_field[i] >= c->n_fields)
            return fail(PSFMC_EINVAL, "segment %d: field %d, count %d", i, seg_field[i], seg_count[i]);
        if (!c->has_layout[seg_field[i]])
            return fail(PSFMC_EINVAL, "field %d has no layout (psfmc_set_layout_field)", seg_field[i]);
        W += seg_count[i];
    }
    if (W > c->max_walkers) return fail(PSFMC_EINVAL, "W=%lld outside [0, max_walkers=%d]", W, c->max_walkers);
    if (W == 0) return PSFMC_OK;
    if (!d_out || (c->layouts[0].n_params > 0 && !d_theta)) return fail(PSFMC_EINVAL, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    const int P = c->layouts[0].n_params;
    int off = 0;
    for (int i = 0; i < n_seg; ++i) {
        if (!seg_count[i]) continue;
        launch_theta_prep(c, seg_count[i], d_theta + (size_t)off * P, d_extra ? d_extra + off : nullptr, nullptr, st,
                          StretchIn{}, seg_field[i], off);
        off += seg_count[i];
    }
    RC_TRY(run_pipeline(c, (int)W, c->d_skip, st));
    *n_w = (int)W;
    return PSFMC_OK;
}

// Walkers of several fields in one batch: segment i = seg_count[i] consecutive walkers of field
// seg_field[i] (host arrays); d_theta [W][P] / d_lnprob [W] in that order, W = sum of the counts.
// One record derivation per segment (its field's layout), then ONE pass of the likelihood pipeline
// over all W walkers.
extern "C" int psfmc_eval_theta_device_fields(psfmc_ctx* c, int n_seg, const int* seg_field, const int* seg_count,
                                              const double* d_theta, const double* d_extra, double* d_lnprob,
                                              void* stream) {
    hipStream_t st = stream ? (hipStream_t)stream : (c ? c->stream : nullptr);
    int W = 0;
    RC_TRY(fields_records_pass(c, n_seg, seg_field, seg_count, d_theta, d_extra, d_lnprob, st, &W));
    if (W == 0) return PSFMC_OK;
    hipLaunchKernelGGL(k_finish_posterior, dim3(finish_blocks(W)), dim3(kFinishThreads), 0, st, c->d_partial,
                       c->d_skip, c->d_lnprior, d_lnprob, W, c->nblk, 1, 0);
    HIP_TRY(hipGetLastError());
    return PSFMC_OK;
}

// host-buffer form of psfmc_eval_theta_device_fields
extern "C" int psfmc_eval_theta_fields(psfmc_ctx* c, int n_seg, const int* seg_field, const int* seg_count,
                                       const double* theta, const double* extra, double* lnprob) {
    if (!c || n_seg < 0 || (n_seg && !seg_count)) return fail(PSFMC_EINVAL, "bad segment list");
    if (!c->has_layout[0]) return fail(PSFMC_EINVAL, "psfmc_set_layout has not been called");
    long long W = 0;
    for (int i = 0; i < n_seg; ++i) W += seg_count[i] > 0 ? seg_count[i] : 0;
    if (W > c->max_walkers) return fail(PSFMC_EINVAL, "W=%lld outside [0, max_walkers=%d]", W, c->max_walkers);
    if (W == 0) return PSFMC_OK;
    if (!lnprob || (c->layouts[0].n_params > 0 && !theta)) return fail(PSFMC_EINVAL, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (c->layouts[0].n_params)
        HIP_TRY(hipMemcpyAsync(c->d_theta, theta, (size_t)W * c->layouts[0].n_params * sizeof(double),
                               hipMemcpyHostToDevice, st));
    if (extra) HIP_TRY(hipMemcpyAsync(c->d_extra, extra, (size_t)W * sizeof(double), hipMemcpyHostToDevice, st));
    RC_TRY(psfmc_eval_theta_device_fields(c, n_seg, seg_field, seg_count, c->d_theta, extra ? c->d_extra : nullptr,
                                          c->d_like, st));
    HIP_TRY(hipMemcpyAsync(lnprob, c->d_like, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PSFMC_OK;
}

// psfmc_eval_theta_fields with the two terms apart (psfmc_eval_theta_split's rules): the same records and the same
// pass, the log-likelihoods by k_split_finish, the log-priors as the record derivation left them
extern "C" int psfmc_eval_theta_split_fields(psfmc_ctx* c, int n_seg, const int* seg_field, const int* seg_count,
                                             const double* theta, const double* extra, double* lnlike,
                                             double* lnprior) {
    if (!c || n_seg < 0 || (n_seg && !seg_count)) return fail(PSFMC_EINVAL, "bad segment list");
    if (!c->has_layout[0]) return fail(PSFMC_EINVAL, "psfmc_set_layout has not been called");
    long long W = 0;
    for (int i = 0; i < n_seg; ++i) W += seg_count[i] > 0 ? seg_count[i] : 0;
    if (W > c->max_walkers) return fail(PSFMC_EINVAL, "W=%lld outside [0, max_walkers=%d]", W, c->max_walkers);
    if (W == 0) return PSFMC_OK;
    if (!lnlike || !lnprior || (c->layouts[0].n_params > 0 && !theta)) return fail(PSFMC_EINVAL, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (c->layouts[0].n_params)
        HIP_TRY(hipMemcpyAsync(c->d_theta, theta, (size_t)W * c->layouts[0].n_params * sizeof(double),
                               hipMemcpyHostToDevice, st));
    if (extra) HIP_TRY(hipMemcpyAsync(c->d_extra, extra, (size_t)W * sizeof(double), hipMemcpyHostToDevice, st));
    int n = 0;
    RC_TRY(fields_records_pass(c, n_seg, seg_field, seg_count, c->d_theta, extra ? c->d_extra : nullptr, c->d_like, st,
                               &n));
    hipLaunchKernelGGL(k_split_finish, dim3(finish_blocks(n)), dim3(kFinishThreads), 0, st, c->d_partial, c->d_skip,
                       c->nblk, c->d_like, n, 1, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(lnlike, c->d_like, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(lnprior, c->d_lnprior, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PSFMC_OK;
}

extern "C" int psfmc_eval_theta(psfmc_ctx* c, int W, const double* theta, const double* extra,
                                double* lnprob) {
    int rc = check_theta_call(c, W, theta, lnprob);
    if (rc != PSFMC_OK || W == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (c->layouts[0].n_params)
        HIP_TRY(hipMemcpyAsync(c->d_theta, theta, (size_t)W * c->layouts[0].n_params * sizeof(double),
                               hipMemcpyHostToDevice, st));
    if (extra) HIP_TRY(hipMemcpyAsync(c->d_extra, extra, (size_t)W * sizeof(double), hipMemcpyHostToDevice, st));
    RC_TRY(eval_theta_device(c, W, c->d_theta, extra ? c->d_extra : nullptr, c->d_like, st));
    HIP_TRY(hipMemcpyAsync(lnprob, c->d_like, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PSFMC_OK;
}

extern "C" int psfmc_debug_theta_rows(psfmc_ctx* c, int W, const double* theta, double* rows,
                                      double* lnprior, uint8_t* skip) {
    int rc = check_theta_call(c, W, theta, rows);
    if (rc != PSFMC_OK || W == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (c->layouts[0].n_params)
        HIP_TRY(hipMemcpyAsync(c->d_theta, theta, (size_t)W * c->layouts[0].n_params * sizeof(double),
                               hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(c->d_rows, 0, (size_t)W * c->rlen * sizeof(double), st));
    launch_theta_prep(c, W, c->d_theta, nullptr, c->d_rows, st, StretchIn{});
    HIP_TRY(hipMemcpyAsync(rows, c->d_rows, (size_t)W * c->rlen * sizeof(double), hipMemcpyDeviceToHost, st));
    if (lnprior) HIP_TRY(hipMemcpyAsync(lnprior, c->d_lnprior, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, st));
    if (skip) HIP_TRY(hipMemcpyAsync(skip, c->d_skip, (size_t)W, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PSFMC_OK;
}

// ---------------------------------------------------------------------------
// posterior-image accumulation (models.py:74-97)
// ---------------------------------------------------------------------------
extern "C" int psfmc_reset_accumulated(psfmc_ctx* c) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    const size_t acc_bytes = (size_t)c->n_fields * 4 * c->S * sizeof(double);
    if (!c->d_acc) HIP_TRY(hipMalloc(&c->d_acc, acc_bytes));
    HIP_TRY(hipMemsetAsync(c->d_acc, 0, acc_bytes, c->stream));
    if (c->d_lin) HIP_TRY(hipMemsetAsync(c->d_lin, 0, (size_t)c->n_psf * 3 * c->S * sizeof(double), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int f = 0; f < c->n_fields; ++f) c->acc_count[f] = 0;
    c->lin_pending = 0;
    return PSFMC_OK;
}

// one field of a psfmc_ctx_create_fields context: its image sums, the linear sums of its kernel spectra
// (pending samples of OTHER fields stay pending) and its count
extern "C" int psfmc_reset_accumulated_field(psfmc_ctx* c, int field) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (field < 0 || field >= c->n_fields) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    if (!c->d_acc) return psfmc_reset_accumulated(c);
    HIP_TRY(hipSetDevice(c->device));
    const size_t S = (size_t)c->S;
    HIP_TRY(hipMemsetAsync(c->d_acc + (size_t)field * 4 * S, 0, 4 * S * sizeof(double), c->stream));
    if (c->d_lin)
        HIP_TRY(hipMemsetAsync(c->d_lin + (size_t)field * c->n_psf_field * 3 * S, 0,
                               (size_t)c->n_psf_field * 3 * S * sizeof(double), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->acc_count[field] = 0;
    return PSFMC_OK;
}

// buffers of the linear sums (fused back end): allocated outside any stream capture
static int ensure_linear_sums(psfmc_ctx* c) {
    if (c->backend != PSFMC_BACKEND_FUSED || c->d_lin) return PSFMC_OK;
    if (c->n_fields > 1) {
        // several fields: a group's partial holds ONE field's sums; `lin_groups` = groups per field
        const size_t field_el = (size_t)c->n_psf_field * 3 * c->S;
        int gpf = (2048 + c->nblk * c->n_fields - 1) / (c->nblk * c->n_fields);
        const size_t budget = (size_t)96 << 20;
        while (gpf > 1 && (size_t)gpf * c->n_fields * field_el * sizeof(double) > budget) --gpf;
        if (gpf < 1) gpf = 1;
        HIP_TRY(hipMalloc(&c->d_lin, (size_t)c->n_fields * field_el * sizeof(double)));
        HIP_TRY(hipMemset(c->d_lin, 0, (size_t)c->n_fields * field_el * sizeof(double)));
        HIP_TRY(hipMalloc(&c->d_linpart, (size_t)gpf * c->n_fields * field_el * sizeof(double)));
        c->lin_groups = gpf;
        return PSFMC_OK;
    }
    const size_t per_group = (size_t)c->n_psf * 3 * c->S * sizeof(double);
    // walker groups of one call: enough waves to fill the chip (row groups x groups >= ~2048), the
    // partials within ~96 MB
    int groups = (2048 + c->nblk - 1) / c->nblk;
    const size_t budget = (size_t)96 << 20;
    if ((size_t)groups * per_group > budget) groups = (int)(budget / per_group);
    if (groups < 1) groups = 1;
    if (groups > 64) groups = 64;
    HIP_TRY(hipMalloc(&c->d_lin, per_group));
    HIP_TRY(hipMemset(c->d_lin, 0, per_group));
    HIP_TRY(hipMalloc(&c->d_linpart, (size_t)groups * per_group));
    c->lin_groups = groups;
    return PSFMC_OK;
}

// fused back end: add the W walkers whose prep records are in c->d_prep to the linear sums.  The sums are
// kept per kernel spectrum, i.e. per (field, PSF): walkers of several fields (`nf` consecutive fields from
// `f0`, `per` walkers each, W = nf * per) land in their own fields' sums by themselves.
static int accumulate_linear(psfmc_ctx* c, int W, hipStream_t st, int f0 = 0, int nf = 1, int per = -1) {
    if (per < 0) per = W;
    if (c->n_fields > 1) {
        // field-contiguous walkers: whole groups per field, each looking only at its field's kernel spectra
        // (with every group scanning all n_fields x PSFs for its walkers, eight fields accumulated at half the
        // rate of eight contexts)
        if ((long long)nf * per != W) return fail(PSFMC_EINVAL, "accumulation: %d fields x %d walkers != %d", nf, per, W);
        int gpf = c->lin_groups < per ? c->lin_groups : per;           // groups per field
        const int group_size = (per + gpf - 1) / gpf;
        gpf = (per + group_size - 1) / group_size;
        if (per % group_size) {
            // a field's last group is short: the next field's groups must still start at its first walker, which
            // g * group_size does not give -- one launch per field then
            for (int j = 0; j < nf; ++j) {
                SizeCall a;
                a.c = c; a.n = per; a.prep = c->d_prep + (size_t)j * per * c->plen; a.groups = gpf;
                a.group_size = group_size; a.st = st; a.per_field = per; a.field = f0 + j;
                RC_TRY(size_call(SZ_RASTER_SUMS, c->nx, a));
                const size_t n_el = (size_t)c->n_psf_field * 3 * c->S;
                hipLaunchKernelGGL(k_sum_partials_fields, dim3(512), dim3(256), 0, st, c->d_linpart, gpf, 1,
                                   c->d_lin + (size_t)(f0 + j) * n_el, n_el);
            }
        } else {
            SizeCall a;
            a.c = c; a.n = W; a.prep = c->d_prep; a.groups = gpf * nf; a.group_size = group_size; a.st = st;
            a.per_field = per; a.field = f0;
            RC_TRY(size_call(SZ_RASTER_SUMS, c->nx, a));
            const size_t n_el = (size_t)c->n_psf_field * 3 * c->S;
            hipLaunchKernelGGL(k_sum_partials_fields, dim3(512), dim3(256), 0, st, c->d_linpart, gpf, nf,
                               c->d_lin + (size_t)f0 * n_el, n_el);
        }
        c->lin_pending += W;
        for (int i = 0; i < nf; ++i) c->acc_count[f0 + i] += per;
        return PSFMC_OK;
    }
    const size_t n_el = (size_t)c->n_psf * 3 * c->S;
    int groups = c->lin_groups < W ? c->lin_groups : W;
    const int group_size = (W + groups - 1) / groups;
    groups = (W + group_size - 1) / group_size;
    {
        SizeCall a;
        a.c = c; a.n = W; a.prep = c->d_prep; a.groups = groups; a.group_size = group_size; a.st = st;
        RC_TRY(size_call(SZ_RASTER_SUMS, c->nx, a));
    }
    hipLaunchKernelGGL(k_sum_partials, dim3(512), dim3(256), 0, st, c->d_linpart, groups, c->d_lin, n_el);
    c->lin_pending += W;
    c->acc_count[f0] += W;
    return PSFMC_OK;
}

// convolve the pending linear sums into the four image sums of d_acc.  Per PSF three passes of
// the row / column kernels over ONE pseudo-walker read from memory: (sum raw, 0), (0, sum raw^2)
// and (sum PS-only raw, 0).  Each sum travels alone in its packed transform: added up, the samples'
// raw^2 is dominated by the brightest sample far more than their raw is, and packed together the
// two channels' rounding errors would leak into each other (measured on the `edge` fixture:
// 3e-6 relative in the weight map; alone, 1e-15).
static int flush_linear_sums(psfmc_ctx* c) {
    if (c->backend != PSFMC_BACKEND_FUSED || c->lin_pending == 0 || !c->d_lin) return PSFMC_OK;
    hipStream_t st = c->stream;
    HIP_TRY(hipStreamSynchronize(st));
    const size_t S = (size_t)c->S;
    std::vector<double> host(S), rho(c->n_psf);
    HIP_TRY(hipMemcpy(rho.data(), c->d_rho, c->n_psf * sizeof(double), hipMemcpyDeviceToHost));
    double *d_img = nullptr, *d_scale = nullptr, *d_fprep = nullptr, *d_out = nullptr;
    HIP_TRY(hipMalloc(&d_img, 2 * S * sizeof(double)));
    int rc = PSFMC_OK;
    if (hipMalloc(&d_scale, sizeof(double)) != hipSuccess ||
        hipMalloc(&d_fprep, (size_t)c->plen * sizeof(double)) != hipSuccess ||
        hipMalloc(&d_out, 2 * S * sizeof(double)) != hipSuccess)
        rc = fail(PSFMC_ENOMEM, "hipMalloc (posterior-image flush)");
    int field_of_p = 0;       // the field whose sums the current kernel spectrum's images go to
    auto acc = [&](const double* src, int slot) {
        hipLaunchKernelGGL(k_accumulate, dim3(256), dim3(256), 0, st, src,
                           c->d_acc + ((size_t)field_of_p * 4 + slot) * S, (int)S, 1, 1, 0);
    };
    // one pseudo-walker: z = img0 + i scale img1 through rows_fwd (from memory), cols, rows_inv;
    // d_out[0] = convolution of img0 with the PSF, d_out[1] = of img1 with the PSF variance map
    auto pass = [&](int psf, const double* img0, const double* img1, double scale) -> int {
        std::vector<double> fprep((size_t)c->plen, 0.0);
        fprep[kPrepPsfIdx] = (double)psf;
        fprep[kPrepMu] = scale;
        fprep[kPrepInvLambda] = 1.0 / (scale * rho[psf]);
        for (int h = 0; h < 2; ++h) {
            const double* src = h ? img1 : img0;
            if (src) HIP_TRY(hipMemcpyAsync(d_img + h * S, src, S * sizeof(double), hipMemcpyDeviceToDevice, st));
            else HIP_TRY(hipMemsetAsync(d_img + h * S, 0, S * sizeof(double), st));
        }
        HIP_TRY(hipMemcpyAsync(d_scale, &scale, sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_fprep, fprep.data(), fprep.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));                 // (fprep / scale are stack data)
        SizeCall a;
        a.c = c; a.n = 1; a.T = c->d_T; a.img = d_img; a.img_scale = d_scale; a.st = st; a.from_image = true;
        RC_TRY(size_call(SZ_ROWS_FWD, c->nx, a));
        a.from_image = false; a.prep = d_fprep;
        RC_TRY(size_call(SZ_COLS, c->ny, a));
        a.partial = c->d_partial; a.conv_out = d_out; a.var_out = d_out + S;
        RC_TRY(size_call(SZ_ROWS_INV, c->nx, a));
        return PSFMC_OK;
    };
    for (int p = 0; p < c->n_psf && rc == PSFMC_OK; ++p) {
        field_of_p = p / c->n_psf_field;
        const double* lin = c->d_lin + (size_t)p * 3 * S;
        // the variance channel's power-of-two scale, and whether any sample used this PSF
        if (hipMemcpy(host.data(), lin + S, S * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(PSFMC_EHIP, "posterior-image flush: copy failed");
            break;
        }
        double peak_b = 0.0;
        bool any = false;
        for (size_t i = 0; i < S; ++i) {
            const double b = fabs(host[i]);
            any |= host[i] != 0.0;                                // (NaN counts)
            if (b > peak_b && b < 1e300) peak_b = b;
        }
        if (!any) continue;                                       // (raw^2 = 0 everywhere: no sample, or an empty model)
        double sc = 1.0;
        if (peak_b > 0.0) {
            int eb;
            (void)frexp(peak_b, &eb);
            sc = ldexp(1.0, -eb);
        }
        rc = pass(p, lin, nullptr, 1.0);
        if (rc != PSFMC_OK) break;
        acc(lin, 0);                          // raw
        acc(d_out, 1);                        // convolved model
        rc = pass(p, nullptr, lin + S, sc);
        if (rc != PSFMC_OK) break;
        acc(d_out + S, 2);                    // model variance
        rc = pass(p, lin + 2 * S, nullptr, 1.0);
        if (rc != PSFMC_OK) break;
        acc(d_out, 3);                        // PS-only convolved
        if (hipStreamSynchronize(st) != hipSuccess) rc = fail(PSFMC_EHIP, "posterior-image flush failed: %s",
                                                              hipGetErrorString(hipGetLastError()));
    }
    if (rc == PSFMC_OK) {
        (void)hipMemsetAsync(c->d_lin, 0, (size_t)c->n_psf * 3 * S * sizeof(double), st);
        (void)hipStreamSynchronize(st);
        c->lin_pending = 0;
    }
    (void)hipFree(d_img);
    if (d_scale) (void)hipFree(d_scale);
    if (d_fprep) (void)hipFree(d_fprep);
    if (d_out) (void)hipFree(d_out);
    return rc;
}

// add the images of the W walkers whose prep records are in c->d_prep to the sums
static int accumulate_from_prep(psfmc_ctx* c, int W, hipStream_t st, int f0 = 0, int nf = 1, int per = -1) {
    const bool fused = c->backend == PSFMC_BACKEND_FUSED;
    if (fused && c->linear_acc) {
        if (!c->d_lin) return fail(PSFMC_EINVAL, "linear sums not allocated");
        return accumulate_linear(c, W, st, f0, nf, per);
    }
    if (c->n_fields > 1) return fail(PSFMC_EINVAL, "contexts of several fields accumulate images as linear sums only");
    RC_TRY(ensure_image_staging(c));
    if (fused && !c->d_rawstage) HIP_TRY(hipMalloc(&c->d_rawstage, (size_t)c->img_cap * c->S * sizeof(double)));
    const double* conv_src = fused ? c->d_img0 : c->d_real;
    const double* var_src = fused ? c->d_img1 : c->d_real;
    const int stride = fused ? 1 : 2, var_c = fused ? 0 : 1;
    auto acc = [&](const double* src, int strd, int comp, int slot, int n) {
        hipLaunchKernelGGL(k_accumulate, dim3(256), dim3(256), 0, st, src, c->d_acc + (size_t)slot * c->S,
                           c->S, n, strd, comp);
    };
    for (int w0 = 0; w0 < W; w0 += c->chunk) {
        const int n = W - w0 < c->chunk ? W - w0 : c->chunk;
        const double* prep = c->d_prep + (size_t)w0 * c->plen;
        if (fused) {
            RC_TRY(fused_forward(c, n, c->d_T, prep, nullptr, 0, c->d_rawstage, st));
            RC_TRY(fused_inverse(c, n, c->d_T, prep, nullptr, c->d_partial, c->d_img0, c->d_img1, st));
            acc(c->d_rawstage, 1, 0, 0, n);
        } else {
            hipLaunchKernelGGL(k_raster, dim3((c->S + 1023) / 1024, n), dim3(256),
                               (size_t)prep_rec_len(c->n_ps, c->n_sersic) * sizeof(double), st, prep,
                               (const uint8_t*)nullptr, c->d_real, c->n_ps, c->n_sersic, c->ny, c->nx, 0,
                               extra_image_of(c, prep));
            acc(c->d_real, 2, 0, 0, n);
            RC_TRY(hipfft_convolve(c, n, prep, nullptr, st, 0));
        }
        acc(conv_src, stride, 0, 1, n);
        acc(var_src, stride, var_c, 2, n);
        if (fused) {
            RC_TRY(fused_forward(c, n, c->d_T, prep, nullptr, 1, nullptr, st));
            RC_TRY(fused_inverse(c, n, c->d_T, prep, nullptr, c->d_partial, c->d_img0, c->d_img1, st));
        } else {
            RC_TRY(hipfft_convolve(c, n, prep, nullptr, st, 1));
        }
        acc(conv_src, stride, 0, 3, n);
    }
    c->acc_count[0] += W;
    return PSFMC_OK;
}

extern "C" int psfmc_accumulate_images(psfmc_ctx* c, int W, const double* rows) {
    if (c && c->n_fields > 1) return fail(PSFMC_EINVAL, "this entry point serves contexts of one field");
    int rc = check_call(c, W, rows, rows);
    if (rc != PSFMC_OK || W == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->d_acc) RC_TRY(psfmc_reset_accumulated(c));
    RC_TRY(ensure_linear_sums(c));
    hipStream_t st = c->stream;
    RC_TRY(take_aux_rows(c, W));
    HIP_TRY(hipMemcpyAsync(c->d_rows, rows, (size_t)W * c->rlen * sizeof(double), hipMemcpyHostToDevice, st));
    c->prep_tabs_valid = false;                       // d_prep is being rewritten
    hipLaunchKernelGGL(k_prep, dim3((W + 127) / 128), dim3(128), 0, st, c->d_rows, c->d_prep, W, c->n_ps,
                       c->n_sersic, c->wraps[0].ly, c->wraps[0].lx, c->d_rho, c->n_psf, 0);
    launch_pow_tables(c, W, 0, nullptr, st);
    rc = accumulate_from_prep(c, W, st);
    (void)hipStreamSynchronize(st);
    if (rc == PSFMC_OK) HIP_TRY(hipGetLastError());
    return rc;
}

// raw parameter vectors (host) -> posterior-image sums: the records are derived on the device like
// psfmc_eval_theta does (no host-side gammaincinv per sample when the images of a whole database
// are recomputed, analysis/images.py:62-74)
static int accumulate_theta_impl(psfmc_ctx* c, int field, int W, const double* theta) {
    int rc = check_theta_call(c, W, theta, theta ? (const void*)theta : (const void*)c);
    if (rc != PSFMC_OK || W == 0) return rc;
    if (field < 0 || field >= c->n_fields) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    if (!c->has_layout[field])
        return fail(PSFMC_EINVAL, "field %d has no layout (psfmc_set_layout_field)", field);
    HIP_TRY(hipSetDevice(c->device));
    if (!c->d_acc) RC_TRY(psfmc_reset_accumulated(c));
    RC_TRY(ensure_linear_sums(c));
    hipStream_t st = c->stream;
    if (c->layouts[0].n_params)
        HIP_TRY(hipMemcpyAsync(c->d_theta, theta, (size_t)W * c->layouts[0].n_params * sizeof(double),
                               hipMemcpyHostToDevice, st));
    launch_theta_prep(c, W, c->d_theta, nullptr, nullptr, st, StretchIn{}, field, 0);
    rc = accumulate_from_prep(c, W, st, field, 1, W);
    (void)hipStreamSynchronize(st);
    if (rc == PSFMC_OK) HIP_TRY(hipGetLastError());
    return rc;
}

extern "C" int psfmc_accumulate_theta(psfmc_ctx* c, int W, const double* theta) {
    if (c && c->n_fields > 1) return fail(PSFMC_EINVAL, "this entry point serves contexts of one field");
    return accumulate_theta_impl(c, 0, W, theta);
}

// the same for one field of a psfmc_ctx_create_fields context
extern "C" int psfmc_accumulate_theta_field(psfmc_ctx* c, int field, int W, const double* theta) {
    return accumulate_theta_impl(c, field, W, theta);
}

// ---------------------------------------------------------------------------
// device-resident stretch-move sampling
// ---------------------------------------------------------------------------
// Sampler buffers live in the context and only ever grow: a block of iterations used to pay
// a dozen hipMalloc / hipFree.
template <typename Tp>
static int grow(Tp** p, size_t* cap, size_t need) {
    if (need <= *cap && *p) return PSFMC_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
    HIP_TRY(hipMalloc(p, (need ? need : 1) * sizeof(Tp)));
    *cap = need ? need : 1;
    return PSFMC_OK;
}

// F: ensembles of the run -- 1 (an ordinary context), or every field of a psfmc_ctx_create_fields context
static int stretch_check(psfmc_ctx* c, int W, int F = 1) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (F != c->n_fields)
        return fail(PSFMC_EINVAL, F == 1 ? "this entry point serves contexts of one field"
                                         : "psfmc_stretch_run_fields samples every field of the context");
    if (!c->has_layout[0]) return fail(PSFMC_EINVAL, "psfmc_set_layout has not been called");
    if (W < 2 || (W & 1) || (long long)W * F > c->max_walkers)
        return fail(PSFMC_EINVAL, "W must be even and fields x W within max_walkers");
    const int P = c->layouts[0].n_params;
    if (P < 1) return fail(PSFMC_EINVAL, "model has no free parameter");
    // every prior must be evaluated on the device
    std::vector<int> fam(P);
    HIP_TRY(hipSetDevice(c->device));
    for (int f = 0; f < F; ++f) {
        if (!c->has_layout[f])
            return fail(PSFMC_EINVAL, "field %d has no layout (psfmc_set_layout_field)", f);
        const ThetaLayout& L = c->layouts[f];
        HIP_TRY(hipMemcpy(fam.data(), L.family, P * sizeof(int), hipMemcpyDeviceToHost));
        for (int v : fam)
            if (v == PRIOR_HOST) return fail(PSFMC_EINVAL, "a prior is evaluated on the host; use the host sampler");
    }
    return PSFMC_OK;
}

// upload the walkers, counters and the block's random numbers; size the chain buffers.  F ensembles of W
// walkers each: host arrays carry the ensemble as their leading dimension (pos [F][W][P], z [F][n_iter][2][half],
// ...); on the device the three random arrays are [3][F][n_iter W].
static int stretch_upload(psfmc_ctx* c, int W, int n_iter, const double* pos, const double* lnprob,
                          int lnprob_valid, const double* z, const double* lz, const int* partner,
                          const double* log_u, const long long* naccepted, bool store, hipStream_t st, int F = 1) {
    psfmc_ctx::Stretch& S = c->stretch;
    const int P = c->layouts[0].n_params, half = W / 2;
    const size_t n_rand = (size_t)n_iter * W * F;             // per random array, all ensembles
    const size_t WF = (size_t)W * F;
    RC_TRY(grow(&S.pos, &S.cap_pos, WF * P));
    RC_TRY(grow(&S.lnp, &S.cap_lnp, WF));
    RC_TRY(grow(&S.q, &S.cap_q, (size_t)half * F * P * (F == 1 ? 3 : 1)));       // (three proposal sets: whole-iteration launches)
    RC_TRY(grow(&S.accflag, &S.cap_acc, (size_t)half));
    RC_TRY(grow(&S.newlnp, &S.cap_new, (size_t)half * F));
    RC_TRY(grow(&S.nacc, &S.cap_nacc, WF));
    RC_TRY(grow(&S.rand, &S.cap_rand, 3 * n_rand));
    RC_TRY(grow(&S.partner, &S.cap_partner, n_rand));
    RC_TRY(grow(&S.iter, &S.cap_iter, (size_t)1));
    if (store && n_iter) {
        RC_TRY(grow(&S.chain, &S.cap_chain, WF * n_iter * P));
        RC_TRY(grow(&S.lnchain, &S.cap_lnchain, WF * n_iter));
    }
    S.W = W; S.n_iter = n_iter; S.F = F; S.store = store && n_iter; S.open = true;
    S.moves = false;                                          // (moves_upload sets it for the runs that propose by kind)
    if (n_rand) {
        HIP_TRY(hipMemcpyAsync(S.rand, z, n_rand * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(S.rand + n_rand, lz, n_rand * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(S.rand + 2 * n_rand, log_u, n_rand * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(S.partner, partner, n_rand * sizeof(int), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(S.pos, pos, WF * P * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(S.nacc, naccepted, WF * sizeof(long long), hipMemcpyHostToDevice, st));
    if (lnprob_valid)
        HIP_TRY(hipMemcpyAsync(S.lnp, lnprob, WF * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(S.iter, 0, sizeof(int), st));
    return PSFMC_OK;
}

static int stretch_download(psfmc_ctx* c, double* pos, double* lnprob, double* chain, double* lnprob_chain,
                            long long* naccepted, hipStream_t st) {
    psfmc_ctx::Stretch& S = c->stretch;
    const int P = c->layouts[0].n_params;
    const size_t W = (size_t)S.W * S.F;
    HIP_TRY(hipMemcpyAsync(pos, S.pos, W * P * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(lnprob, S.lnp, W * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(naccepted, S.nacc, W * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (S.store && chain) {
        HIP_TRY(hipMemcpyAsync(chain, S.chain, W * S.n_iter * P * sizeof(double), hipMemcpyDeviceToHost, st));
        if (lnprob_chain)
            HIP_TRY(hipMemcpyAsync(lnprob_chain, S.lnchain, W * S.n_iter * sizeof(double),
                                   hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return PSFMC_OK;
}

// first stage of a half-step: the stretch proposals of half `h` at iteration `it`, their
// priors and prep records (every walker of the half: the accept step needs every proposal)
static void stretch_propose(psfmc_ctx* c, int it, int h, bool graph_iter, hipStream_t st) {
    psfmc_ctx::Stretch& S = c->stretch;
    const int half = S.W / 2, P = c->layouts[0].n_params;
    const size_t per_field = (size_t)S.n_iter * S.W;          // random numbers of one ensemble
    launch_theta_prep(c, half, nullptr, nullptr, nullptr, st,
                      StretchIn{S.pos, S.q, S.rand, S.partner, graph_iter ? S.iter : nullptr, it, half, h,
                                (size_t)S.W * P, (size_t)half * P, per_field},
                      0, 0, S.F);
}

// last stage: sum (or take the gathered values), accept, move, chain entry.  nf > 1: joint walkers, each
// proposal nf field records, half apart
static void stretch_accept(psfmc_ctx* c, int it, int h, const double* d_newlnp, bool graph_iter, hipStream_t st,
                           int nf = 1) {
    psfmc_ctx::Stretch& S = c->stretch;
    const int half = S.W / 2;
    const size_t per_field = (size_t)S.n_iter * S.W;
    const size_t n_rand = per_field * S.F;
    // whole-iteration launches: the first half records its outcomes, the second half selects its rows by them
    uint8_t* acc_out = S.spec && h == 0 ? S.accflag : nullptr;
    const uint8_t* acc_in = S.spec && h == 1 ? S.accflag : nullptr;
    hipLaunchKernelGGL(k_stretch_finish, dim3(finish_blocks(half), S.F), dim3(kFinishThreads), 0, st, c->d_partial,
                       c->d_skip, c->d_lnprior, c->nblk, d_newlnp, S.pos, S.lnp, S.q, S.rand + n_rand,
                       S.rand + 2 * n_rand, S.nacc, S.store ? S.chain : nullptr, S.store ? S.lnchain : nullptr,
                       graph_iter ? S.iter : nullptr, it, S.n_iter, half, h, c->layouts[0].n_params, per_field,
                       acc_out, acc_in, S.partner, nf, half);
}

// the end of every run that called stretch_upload, on every path: the results come down if all went well, the
// stream is drained, and the run is closed
static int stretch_end_run(psfmc_ctx* c, int rc, double* pos, double* lnprob, double* chain, double* lnprob_chain,
                           long long* naccepted, hipStream_t st) {
    psfmc_ctx::Stretch& S = c->stretch;
    if (rc == PSFMC_OK) rc = stretch_download(c, pos, lnprob, chain, lnprob_chain, naccepted, st);
    (void)hipStreamSynchronize(st);
    if (rc == PSFMC_OK && hipGetLastError() != hipSuccess) rc = fail(PSFMC_EHIP, "kernel launch failed");
    S.open = false;
    S.spec = false;
    S.moves = false;
    return rc;
}

// a whole iteration's proposals in one launch (StretchIn::spec): 3 half walkers
static void stretch_propose_iteration(psfmc_ctx* c, int it, bool graph_iter, hipStream_t st) {
    psfmc_ctx::Stretch& S = c->stretch;
    const int half = S.W / 2, P = c->layouts[0].n_params;
    StretchIn sp{S.pos, S.q, S.rand, S.partner, graph_iter ? S.iter : nullptr, it, half, 0,
                 (size_t)S.W * P, (size_t)half * P, (size_t)S.n_iter * S.W, 1};
    launch_theta_prep(c, 3 * half, nullptr, nullptr, nullptr, st, sp);
}

static int stretch_prepare_accumulation(psfmc_ctx* c) {
    if (!c->d_acc) RC_TRY(psfmc_reset_accumulated(c));
    RC_TRY(ensure_linear_sums(c));
    RC_TRY(ensure_image_staging(c));
    if (c->backend == PSFMC_BACKEND_FUSED && !c->linear_acc && !c->d_rawstage)
        HIP_TRY(hipMalloc(&c->d_rawstage, (size_t)c->img_cap * c->S * sizeof(double)));
    return PSFMC_OK;
}

// log-posteriors of the F ensembles' current positions (S.pos -> S.lnp): one record derivation per field,
// one pass of the likelihood pipeline over all F W walkers
static int stretch_eval_positions(psfmc_ctx* c, hipStream_t st) {
    psfmc_ctx::Stretch& S = c->stretch;
    if (S.F == 1) return eval_theta_device(c, S.W, S.pos, nullptr, S.lnp, st);
    launch_theta_prep(c, S.W, S.pos, nullptr, nullptr, st, StretchIn{}, 0, 0, S.F);
    RC_TRY(run_pipeline(c, S.W * S.F, c->d_skip, st));
    hipLaunchKernelGGL(k_finish_posterior, dim3(finish_blocks(S.W * S.F)), dim3(kFinishThreads), 0, st, c->d_partial,
                       c->d_skip, c->d_lnprior, S.lnp, S.W * S.F, c->nblk, 1, 0);
    HIP_TRY(hipGetLastError());
    return PSFMC_OK;
}

static int stretch_run_impl(psfmc_ctx* c, int F, int W, int n_iter, double* pos, double* lnprob,
                            int lnprob_valid, const double* z, const double* lz, const int* partner,
                            const double* log_u, double* chain, double* lnprob_chain,
                            long long* naccepted, int accumulate) {
    RC_TRY(stretch_check(c, W, F));
    if (n_iter < 0 || !pos || !lnprob || !naccepted || (n_iter && (!z || !lz || !partner || !log_u)))
        return fail(PSFMC_EINVAL, "NULL buffer");
    const int half = W / 2;
    hipStream_t st = c->stream;
    psfmc_ctx::Stretch& S = c->stretch;
    int rc = stretch_upload(c, W, n_iter, pos, lnprob, lnprob_valid, z, lz, partner, log_u, naccepted,
                            chain != nullptr, st, F);
    if (rc == PSFMC_OK && !lnprob_valid) rc = stretch_eval_positions(c, st);
    if (rc == PSFMC_OK && accumulate) rc = stretch_prepare_accumulation(c);
    if (rc != PSFMC_OK) return stretch_end_run(c, rc, pos, lnprob, chain, lnprob_chain, naccepted, st);
    // one iteration: two half-ensemble proposals (chain entries included), optional image
    // sums.  A half-step is three stages: proposals + priors + prep records (one kernel), the
    // likelihood pipeline, and sum + accept + move + chain entry (one kernel).  The kernels take
    // the iteration number by value, or from *S.iter when one captured iteration is replayed as
    // a hipGraph.
    const bool use_d_iter = n_iter > 2 && c->use_graph && !c->profile && c->backend == PSFMC_BACKEND_FUSED && F == 1;
    int it_host = 0;
    // Small ensembles (the reference's default 2 P + 2 walkers, fitting.py:52-53) are latency-bound: a half-step of
    // 11 walkers takes as long as one of 33.  They run ONE pipeline pass per iteration over the first half's
    // proposals and BOTH candidate proposals of every second-half walker (partner moved / partner stayed), and the
    // second accept step picks by the first one's outcomes: the same chain bit for bit (per-walker results do not
    // depend on the batch), 6 launches per iteration instead of 10.
    // default rule, measured (tools/time_small_sampler.py; profiles/r3_small_sampler.txt): the single pass wins while
    // half an ensemble is at most ~3 M transform pixels -- 183 walkers at 128^2 (x1.55 at 22 walkers ... x1.10 at
    // 256), 45 at 256^2 (x1.31 at 22, x1.09 at 64), 11 at 512^2 (x1.07); beyond it the extra half-ensemble of
    // evaluations costs more than the launches it saves
    const int spec_bound = c->speculate >= 0 ? c->speculate : (int)(3.0e6 / ((double)c->ny * c->nx));
    S.spec = F == 1 && half <= spec_bound && 3 * half <= c->max_walkers && c->backend == PSFMC_BACKEND_FUSED;
    if (S.spec) ++c->speculated_runs;
    auto iteration = [&]() -> int {
        if (S.spec) {
            stretch_propose_iteration(c, it_host, use_d_iter, st);
            RC_TRY(run_pipeline(c, 3 * half, c->d_skip, st));
            stretch_accept(c, it_host, 0, nullptr, use_d_iter, st);
            stretch_accept(c, it_host, 1, nullptr, use_d_iter, st);
        } else for (int h = 0; h < 2; ++h) {
            stretch_propose(c, it_host, h, use_d_iter, st);
            RC_TRY(run_pipeline(c, half * F, c->d_skip, st));
            stretch_accept(c, it_host, h, nullptr, use_d_iter, st);
        }
        if (accumulate) {
            launch_theta_prep(c, W, S.pos, nullptr, nullptr, st, StretchIn{}, 0, 0, F);
            RC_TRY(accumulate_from_prep(c, W * F, st, 0, F, W));
        }
        if (use_d_iter) hipLaunchKernelGGL(k_stretch_next, dim3(1), dim3(1), 0, st, S.iter);
        ++it_host;
        return PSFMC_OK;
    };
    // Optionally capture one iteration into a hipGraph and replay it (set_option "graph";
    // measured: no gain, the iteration is kernel-time- not launch-bound).
    hipGraphExec_t exec = nullptr;
    if (use_d_iter) {
        hipGraph_t graph = nullptr;
        // un-captured warm-up of the pipeline: one-time attribute calls must not fall
        // inside the capture
        rc = eval_theta_device(c, half, S.pos, nullptr, S.newlnp, st);      // (F == 1 here)
        const long long count_before = c->acc_count[0], pending_before = c->lin_pending;
        if (rc == PSFMC_OK && hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const int crc = iteration();
            const hipError_t e = hipStreamEndCapture(st, &graph);
            if (crc != PSFMC_OK || e != hipSuccess || !graph ||
                hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess)
                exec = nullptr;
            if (graph) (void)hipGraphDestroy(graph);
            it_host = 0;
        }
        (void)hipGetLastError();
        c->acc_count[0] = count_before;            // the captured pass did not run
        c->lin_pending = pending_before;
    }
    for (int it = 0; it < n_iter && rc == PSFMC_OK; ++it) {
        if (exec) {
            if (hipGraphLaunch(exec, st) != hipSuccess) rc = fail(PSFMC_EHIP, "hipGraphLaunch failed");
            else {
                ++c->graph_launches;
                if (accumulate) {
                    c->acc_count[0] += W;
                    if (c->backend == PSFMC_BACKEND_FUSED && c->linear_acc) c->lin_pending += W;
                }
            }
        } else {
            rc = iteration();
        }
    }
    if (exec) {
        (void)hipStreamSynchronize(st);
        (void)hipGraphExecDestroy(exec);
    }
    return stretch_end_run(c, rc, pos, lnprob, chain, lnprob_chain, naccepted, st);
}

extern "C" int psfmc_stretch_run(psfmc_ctx* c, int W, int n_iter, double* pos, double* lnprob,
                                 int lnprob_valid, const double* z, const double* lz, const int* partner,
                                 const double* log_u, double* chain, double* lnprob_chain,
                                 long long* naccepted, int accumulate) {
    return stretch_run_impl(c, 1, W, n_iter, pos, lnprob, lnprob_valid, z, lz, partner, log_u, chain, lnprob_chain,
                            naccepted, accumulate);
}

// Every field of a psfmc_ctx_create_fields context sampled together: n_fields independent ensembles of W
// walkers, each with its own random numbers, their half-step proposals evaluated in ONE batch of
// n_fields W / 2 walkers.  All arrays carry the field as their leading dimension: pos [F][W][P],
// lnprob [F][W], z / lz / log_u / partner [F][n_iter][2][W/2], chain [F][W][n_iter][P],
// lnprob_chain [F][W][n_iter], naccepted [F][W].  A field's chain equals the chain of its own
// one-field context given the same start and random numbers, bit for bit (per-walker results do not
// depend on the batch).
extern "C" int psfmc_stretch_run_fields(psfmc_ctx* c, int W, int n_iter, double* pos, double* lnprob,
                                        int lnprob_valid, const double* z, const double* lz, const int* partner,
                                        const double* log_u, double* chain, double* lnprob_chain,
                                        long long* naccepted, int accumulate) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    return stretch_run_impl(c, c->n_fields, W, n_iter, pos, lnprob, lnprob_valid, z, lz, partner, log_u, chain,
                            lnprob_chain, naccepted, accumulate);
}

// ---------------------------------------------------------------------------
// proposal moves (include/psfmc_hip.h psfmc_move_run): every iteration proposes with the move kind[it] names,
// the stretch move or differential evolution.  A half-step is four stages: k_move_propose writes the
// proposals to S.q, k_theta_prep derives their records from S.q (its "theta is given" mode), the likelihood
// pipeline, and k_stretch_finish as it is (the caller's lz is 0 for a DE half-step: no Hastings term).  No
// whole-iteration launches and no hipGraph here: a DE proposal of the second half depends on the outcomes of
// two walkers of the first.
// ---------------------------------------------------------------------------
// the indices are checked on the host before anything is uploaded: they address the positions on the device
static int moves_check(int W, int n_iter, const int* kind, const int* partner, const int* partner_b) {
    if (n_iter && (!kind || !partner || !partner_b)) return fail(PSFMC_EINVAL, "NULL buffer");
    const int half = W / 2;
    for (int it = 0; it < n_iter; ++it) {
        const int k = kind[it];
        if (k != MOVE_STRETCH && k != MOVE_DE)
            return fail(PSFMC_EINVAL, "kind[%d] = %d is not a move (0 stretch, 1 differential evolution)", it, k);
        if (k == MOVE_DE && W < 4)
            return fail(PSFMC_EINVAL, "a differential-evolution move needs W >= 4 (two distinct partners in each "
                        "half-ensemble); W = %d", W);
        for (int j = 0; j < 2 * half; ++j) {
            const size_t i = (size_t)it * 2 * half + j;
            const int a = partner[i];
            if (a < 0 || a >= half)
                return fail(PSFMC_EINVAL, "partner index %d out of range [0, %d) at iteration %d", a, half, it);
            if (k != MOVE_DE) continue;                       // (partner_b is not read for a stretch move)
            const int b = partner_b[i];
            if (b < 0 || b >= half)
                return fail(PSFMC_EINVAL, "partner index %d out of range [0, %d) at iteration %d", b, half, it);
            if (a == b)
                return fail(PSFMC_EINVAL, "the two partners of a differential-evolution proposal must differ "
                            "(a == b == %d at iteration %d)", a, it);
        }
    }
    return PSFMC_OK;
}

// after stretch_upload: the kinds and second partners of the run's iterations
static int moves_upload(psfmc_ctx* c, const int* kind, const int* partner_b, hipStream_t st) {
    psfmc_ctx::Stretch& S = c->stretch;
    const size_t n_rand = (size_t)S.n_iter * S.W;
    RC_TRY(grow(&S.kind, &S.cap_kind, (size_t)S.n_iter));
    RC_TRY(grow(&S.partner_b, &S.cap_pb, n_rand));
    if (S.n_iter) {
        HIP_TRY(hipMemcpyAsync(S.kind, kind, (size_t)S.n_iter * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(S.partner_b, partner_b, n_rand * sizeof(int), hipMemcpyHostToDevice, st));
    }
    S.moves = true;
    S.spec = false;
    return PSFMC_OK;
}

// the proposals of half `h` at iteration `it` -> S.q
static void move_propose(psfmc_ctx* c, int it, int h, hipStream_t st) {
    psfmc_ctx::Stretch& S = c->stretch;
    const int half = S.W / 2, P = c->layouts[0].n_params;
    hipLaunchKernelGGL(k_move_propose, dim3((half * P + kMoveThreads - 1) / kMoveThreads), dim3(kMoveThreads), 0, st,
                       S.pos, S.q, S.kind, S.partner, S.partner_b, S.rand, it, half, h, P);
}

// ... and their priors and prep records (stretch_propose's results, by k_theta_prep's "theta is given" mode)
static void move_propose_records(psfmc_ctx* c, int it, int h, hipStream_t st) {
    move_propose(c, it, h, st);
    launch_theta_prep(c, c->stretch.W / 2, c->stretch.q, nullptr, nullptr, st, StretchIn{});
}

// ---------------------------------------------------------------------------
// joint walkers (the joint fits' section, psfmc_set_joint_priors, is further down): record derivation and
// proposals, used by the tempered and the plain run loops alike
// ---------------------------------------------------------------------------
// W walkers' vectors d_theta [W][P] -> the prep records, skip flags and log-priors of their F field
// records (field-major).  d_extra: the joint log-priors (joint.d_lp), or nullptr where only the records
// are needed (posterior-image sums)
static void launch_theta_prep_joint(psfmc_ctx* c, int W, const double* d_theta, const double* d_extra,
                                    hipStream_t st) {
    const int F = c->n_fields;
    const FieldSegs segs = F > 1 ? FieldSegs{c->joint.d_fields, c->d_field_sides, c->n_psf_field, 1}
                                 : FieldSegs{nullptr, nullptr, 0, 0};
    c->prep_tabs_valid = false;
    hipLaunchKernelGGL(k_theta_prep, dim3((W + kThetaThreads - 1) / kThetaThreads, F),
                       dim3(kThetaThreads, theta_task_waves(c->n_ps, c->n_sersic)), c->theta_lds, st,
                       c->joint.fields[0], d_theta, d_extra, nullptr, c->d_prep, c->d_lnprior, c->d_skip, W,
                       c->wraps[0].ly, c->wraps[0].lx, c->d_rho, StretchIn{}, 0, segs, aux_out(c, 0));
    launch_pow_tables(c, W * F, 0, c->d_skip, st);
}

// n given vectors d_theta [n][P] -> their joint log-priors (joint.d_lp) and the records of their fields
static void launch_joint_records(psfmc_ctx* c, int n, const double* d_theta, hipStream_t st) {
    hipLaunchKernelGGL(k_joint_prior, dim3((n + 63) / 64), dim3(64), 0, st, c->joint.prior, c->joint.d_fields,
                       c->n_fields, d_theta, c->joint.d_lp, n);
    launch_theta_prep_joint(c, n, d_theta, c->joint.d_lp, st);
}

// the stretch proposals of half `h` at iteration `it` of T ensembles of 2 half joint walkers (k_joint_propose)
// -> d_q [T half][P], joint.d_lp and the records of their fields
static void launch_joint_propose(psfmc_ctx* c, const double* d_pos, double* d_q, const double* d_z,
                                 const int* d_partner, int it, int T, int half, int h, hipStream_t st) {
    const int n = T * half;
    hipLaunchKernelGGL(k_joint_propose, dim3((n + 63) / 64), dim3(64), 0, st, c->joint.prior, c->joint.d_fields,
                       c->n_fields, d_pos, d_q, d_z, d_partner, it, T, half, h, c->joint.d_lp);
    launch_theta_prep_joint(c, n, d_q, c->joint.d_lp, st);
}

static int joint_check(psfmc_ctx* c, int W) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (!c->joint.ready)
        return fail(PSFMC_EINVAL, "psfmc_set_joint_priors has not been called since the last field layout");
    if (W < 0 || (long long)W * c->n_fields > c->max_walkers)
        return fail(PSFMC_EINVAL, "n_fields x W = %d x %d exceeds max_walkers=%d", c->n_fields, W, c->max_walkers);
    return PSFMC_OK;
}

// ---------------------------------------------------------------------------
// parallel tempering (include/psfmc_hip.h psfmc_eval_theta_split, psfmc_pt_run)
// ---------------------------------------------------------------------------
// n vectors d_theta [n][P] on the device -> their log-likelihoods d_lnL [n]; *d_lnpi: where their log-priors
// are left.  One-field walkers (d_extra: optional extra log-priors), or joint walkers of F field records,
// whose likelihood is the sum over their fields and whose prior is the joint one
static int eval_theta_split_device(psfmc_ctx* c, bool joint, int n, const double* d_theta, const double* d_extra,
                                   double* d_lnL, const double** d_lnpi, hipStream_t st) {
    const int F = joint ? c->n_fields : 1;
    if (joint) launch_joint_records(c, n, d_theta, st);
    else launch_theta_prep(c, n, d_theta, d_extra, nullptr, st, StretchIn{});
    RC_TRY(run_pipeline(c, n * F, c->d_skip, st));
    hipLaunchKernelGGL(k_split_finish, dim3(finish_blocks(n)), dim3(kFinishThreads), 0, st, c->d_partial, c->d_skip,
                       c->nblk, d_lnL, n, F, n);
    HIP_TRY(hipGetLastError());
    *d_lnpi = joint ? c->joint.d_lp : c->d_lnprior;
    return PSFMC_OK;
}

extern "C" int psfmc_eval_theta_split(psfmc_ctx* c, int W, const double* theta, const double* extra,
                                      double* lnlike, double* lnprior) {
    if (c && c->n_fields > 1) return fail(PSFMC_EINVAL, "this entry point serves contexts of one field");
    int rc = check_theta_call(c, W, theta, lnlike);
    if (rc != PSFMC_OK || W == 0) return rc;
    if (!lnprior) return fail(PSFMC_EINVAL, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (c->layouts[0].n_params)
        HIP_TRY(hipMemcpyAsync(c->d_theta, theta, (size_t)W * c->layouts[0].n_params * sizeof(double),
                               hipMemcpyHostToDevice, st));
    if (extra) HIP_TRY(hipMemcpyAsync(c->d_extra, extra, (size_t)W * sizeof(double), hipMemcpyHostToDevice, st));
    const double* d_lnpi = nullptr;
    RC_TRY(eval_theta_split_device(c, false, W, c->d_theta, extra ? c->d_extra : nullptr, c->d_like, &d_lnpi, st));
    HIP_TRY(hipMemcpyAsync(lnlike, c->d_like, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(lnprior, d_lnpi, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PSFMC_OK;
}

// n vectors d_theta [n_seg][per][P], segment f field f's -> their log-likelihoods d_lnL [n_seg per], their
// log-priors in c->d_lnprior: one record launch over the fields, one pipeline pass
static int eval_fields_split_device(psfmc_ctx* c, int n_seg, int per, const double* d_theta, double* d_lnL,
                                    hipStream_t st) {
    launch_theta_prep(c, per, d_theta, nullptr, nullptr, st, StretchIn{}, 0, 0, n_seg);
    RC_TRY(run_pipeline(c, n_seg * per, c->d_skip, st));
    hipLaunchKernelGGL(k_split_finish, dim3(finish_blocks(n_seg * per)), dim3(kFinishThreads), 0, st, c->d_partial,
                       c->d_skip, c->nblk, d_lnL, n_seg * per, 1, 0);
    HIP_TRY(hipGetLastError());
    return PSFMC_OK;
}

// psfmc_pt_run, (joint) psfmc_pt_run_joint and (fields) psfmc_pt_run_fields: the same ladder rules, index checks,
// device state, swap kernel and downloads.  A joint walker is F field records: its capacity check counts them,
// its proposals come from k_joint_propose (k_theta_prep forms the one-field ones itself), and its image sums take
// every field's records.  Fields: every field of the context has its own ladder -- L = n_fields ladders, L T
// ensembles; the host arrays carry the field as their leading dimension, the random numbers behind the
// iteration (and half-step); proposals by k_pt_fields_propose, records by ONE k_theta_prep launch over the fields.
// kind, partner_b (psfmc_pt_move_run*; both null: none of this): every mode proposes by kind with k_pt_move_propose.
enum PtMode { PT_ONE, PT_JOINT, PT_FIELDS };
static int pt_run_impl(psfmc_ctx* c, PtMode mode, int T, int W, int n_iter, const double* betas, double* pos,
                       double* lnlike, double* lnprior, int state_valid, const double* z, const double* lz,
                       const int* partner, const double* log_u, const int* swap_i, const int* swap_j,
                       const double* swap_log_u, double* chain, double* lnprob_chain, double* lnlike_chain,
                       double* lnprior_chain, long long* naccepted, long long* nswap, int accumulate,
                       const int* kind = nullptr, const int* partner_b = nullptr) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    const bool joint = mode == PT_JOINT, fields = mode == PT_FIELDS;
    const bool moves = kind || partner_b;         // (psfmc_pt_move_run*: proposals by kind)
    const int F = joint ? c->n_fields : 1;        // field records per walker
    const int L = fields ? c->n_fields : 1;       // ladders
    if (fields) {
        if (T < 1 || W < 0 || (long long)L * T * W > c->max_walkers)
            return fail(PSFMC_EINVAL, "%d fields x T=%d temperatures x W=%d walkers outside [1, max_walkers=%d]", L, T,
                        W, c->max_walkers);
        if (c->joint.ready)
            return fail(PSFMC_EINVAL, "the context has joint priors (psfmc_set_joint_priors): its fields are one joint "
                        "fit (psfmc_pt_run_joint), not independent ladders");
        if (W < 2 || (W & 1)) return fail(PSFMC_EINVAL, "W must be even and >= 2");
        RC_TRY(stretch_check(c, W, L));           // every field a layout, every prior on the device
    } else if (joint) {
        if (T < 1 || W < 0 || (long long)T * W * F > c->max_walkers)
            return fail(PSFMC_EINVAL, "T=%d temperatures x W=%d walkers x %d fields outside [1, max_walkers=%d]", T, W,
                        F, c->max_walkers);
        RC_TRY(joint_check(c, T * W));            // joint priors set (every prior on the device)
        if (W < 2 || (W & 1)) return fail(PSFMC_EINVAL, "W must be even and >= 2");
    } else {
        if (T < 1 || W < 0 || (long long)T * W > c->max_walkers)
            return fail(PSFMC_EINVAL, "T=%d temperatures x W=%d walkers outside [1, max_walkers=%d]", T, W,
                        c->max_walkers);
        RC_TRY(stretch_check(c, W, 1));           // one field, a layout, W even, every prior on the device
    }
    const bool swaps = T > 1 && n_iter > 0;
    if (n_iter < 0 || !betas || !pos || !lnlike || !lnprior || !naccepted || (T > 1 && !nswap) ||
        (n_iter && (!z || !lz || !partner || !log_u)) || (swaps && (!swap_i || !swap_j || !swap_log_u)) ||
        (moves && n_iter && (!kind || !partner_b)))
        return fail(PSFMC_EINVAL, "NULL buffer");
    // the ladder: finite, beta_0 = 1, strictly decreasing, the last rung 0 (the evidence needs the prior rung)
    for (int t = 0; t < T; ++t)
        if (!std::isfinite(betas[t]) || (t == 0 && betas[t] != 1.0) || (t > 0 && !(betas[t] < betas[t - 1])))
            return fail(PSFMC_EINVAL, "bad temperature ladder at rung %d", t);
    if (T > 1 && betas[T - 1] != 0.0) return fail(PSFMC_EINVAL, "the last rung of the ladder must be beta = 0");
    const int half = W / 2, P = c->layouts[0].n_params;
    const int E = L * T;                          // ensembles: ensemble e = l T + t is rung t of ladder l
    const size_t TW = (size_t)E * W, n_rand = (size_t)n_iter * TW,
                 n_swap = swaps ? (size_t)n_iter * L * (T - 1) * W : 0;
    // every index is checked here: the kernels address walkers by them
    for (size_t i = 0; i < n_rand; ++i)
        if (partner[i] < 0 || partner[i] >= half) {
            if (fields)
                return fail(PSFMC_EINVAL, "partner index %d outside [0, %d) (field %d)", partner[i], half,
                            (int)(i / half % E / T));
            return fail(PSFMC_EINVAL, "partner index %d outside [0, %d)", partner[i], half);
        }
    // the moves: kind [n_iter][L] a move code; a DE iteration of a ladder needs W >= 4 and, in both half-steps of
    // every rung, a second partner in range and distinct from the first (partner_b is not read otherwise)
    for (size_t k = 0; moves && k < (size_t)n_iter * L; ++k) {
        const int it = (int)(k / L), l = (int)(k % L);
        if (kind[k] != MOVE_STRETCH && kind[k] != MOVE_DE)
            return fail(PSFMC_EINVAL, "kind[%d] = %d is not a move (0 stretch, 1 differential evolution)", (int)k,
                        kind[k]);
        if (kind[k] != MOVE_DE) continue;
        if (W < 4)
            return fail(PSFMC_EINVAL, "a differential-evolution move needs W >= 4 (two distinct partners in each "
                        "half-ensemble); W = %d", W);
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < T * half; ++j) {
                const size_t i = (((size_t)it * 2 + h) * E + (size_t)l * T) * half + j;
                const int a = partner[i], b = partner_b[i];
                if (b < 0 || b >= half)
                    return fail(PSFMC_EINVAL, "partner index %d out of range [0, %d) at iteration %d", b, half, it);
                if (a == b)
                    return fail(PSFMC_EINVAL, "the two partners of a differential-evolution proposal must differ "
                                "(a == b == %d at iteration %d)", a, it);
            }
    }
    for (size_t i = 0; i < n_swap; ++i)
        if (swap_i[i] < 0 || swap_i[i] >= W || swap_j[i] < 0 || swap_j[i] >= W)
            return fail(PSFMC_EINVAL, "swap index outside [0, %d)", W);
    // swap pairs must form a matching (the swap kernel gives each pair its own thread); a row of W pairs per
    // (iteration, ladder, rung pair)
    if (n_swap) {
        std::vector<int> seen((size_t)2 * W, -1);
        for (size_t r = 0; r < n_swap / W; ++r)
            for (int k = 0; k < W; ++k) {
                const int a = swap_i[r * W + k], b = W + swap_j[r * W + k];
                if (seen[a] == (int)r || seen[b] == (int)r) return fail(PSFMC_EINVAL, "swap indices are not permutations");
                seen[a] = seen[b] = (int)r;
            }
    }
    // one allocation: doubles, then long longs, then ints, each piece 256-byte aligned
    size_t bytes = 0;
    auto take = [&](size_t n, size_t elem) { const size_t at = bytes; bytes += (n * elem + 255) / 256 * 256; return at; };
    // (q: the half-step's proposals; with several ladders also their beta = 1 rungs gathered for the image sums)
    const size_t n_q = fields && accumulate && T == 1 ? (size_t)L * W : (size_t)E * half;
    const size_t o_beta = take(E, 8), o_pos = take(TW * P, 8), o_lnL = take(TW, 8), o_lnpi = take(TW, 8),
                 o_lnp = take(TW, 8), o_q = take(n_q * P, 8), o_rand = take(3 * n_rand, 8),
                 o_slu = take(n_swap, 8), o_chain = take(chain ? TW * n_iter * P : 0, 8),
                 o_lnpc = take(lnprob_chain ? (size_t)L * W * n_iter : 0, 8),
                 o_lnlc = take(lnlike_chain ? TW * n_iter : 0, 8), o_lnqc = take(lnprior_chain ? TW * n_iter : 0, 8),
                 o_nacc = take(TW, 8), o_nswap = take(E, 8),
                 o_partner = take(n_rand, 4), o_si = take(n_swap, 4), o_sj = take(n_swap, 4),
                 o_kind = take(moves ? (size_t)n_iter * L : 0, 4), o_pb = take(moves ? n_rand : 0, 4);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(hipStreamSynchronize(st));            // a previous call may still use the blob
    RC_TRY(grow(&c->pt_blob, &c->pt_cap, bytes));
    unsigned char* base = c->pt_blob;
    double* d_beta = reinterpret_cast<double*>(base + o_beta);
    double* d_pos = reinterpret_cast<double*>(base + o_pos);
    double* d_lnL = reinterpret_cast<double*>(base + o_lnL);
    double* d_lnpi = reinterpret_cast<double*>(base + o_lnpi);
    double* d_lnp = reinterpret_cast<double*>(base + o_lnp);
    double* d_q = reinterpret_cast<double*>(base + o_q);
    double* d_z = reinterpret_cast<double*>(base + o_rand);
    double* d_lz = d_z + n_rand;
    double* d_logu = d_z + 2 * n_rand;
    double* d_slu = reinterpret_cast<double*>(base + o_slu);
    double* d_chain = chain ? reinterpret_cast<double*>(base + o_chain) : nullptr;
    double* d_lnpc = lnprob_chain ? reinterpret_cast<double*>(base + o_lnpc) : nullptr;
    double* d_lnlc = lnlike_chain ? reinterpret_cast<double*>(base + o_lnlc) : nullptr;
    double* d_lnqc = lnprior_chain ? reinterpret_cast<double*>(base + o_lnqc) : nullptr;
    long long* d_nacc = reinterpret_cast<long long*>(base + o_nacc);
    long long* d_nswap = reinterpret_cast<long long*>(base + o_nswap);
    int* d_partner = reinterpret_cast<int*>(base + o_partner);
    int* d_si = reinterpret_cast<int*>(base + o_si);
    int* d_sj = reinterpret_cast<int*>(base + o_sj);
    int* d_kind = reinterpret_cast<int*>(base + o_kind);
    int* d_pb = reinterpret_cast<int*>(base + o_pb);
    auto up = [&](void* dst, const void* src, size_t n) -> int {
        if (n) HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st));
        return PSFMC_OK;
    };
    for (int l = 0; l < L; ++l) RC_TRY(up(d_beta + (size_t)l * T, betas, T * sizeof(double)));   // the ladder, per ensemble
    RC_TRY(up(d_pos, pos, TW * P * sizeof(double)));
    RC_TRY(up(d_nacc, naccepted, TW * sizeof(long long)));
    if (T > 1) RC_TRY(up(d_nswap, nswap, (size_t)L * (T - 1) * sizeof(long long)));
    RC_TRY(up(d_z, z, n_rand * sizeof(double)));
    RC_TRY(up(d_lz, lz, n_rand * sizeof(double)));
    RC_TRY(up(d_logu, log_u, n_rand * sizeof(double)));
    RC_TRY(up(d_partner, partner, n_rand * sizeof(int)));
    RC_TRY(up(d_si, swap_i, n_swap * sizeof(int)));
    RC_TRY(up(d_sj, swap_j, n_swap * sizeof(int)));
    RC_TRY(up(d_slu, swap_log_u, n_swap * sizeof(double)));
    if (moves) {
        RC_TRY(up(d_kind, kind, (size_t)n_iter * L * sizeof(int)));
        RC_TRY(up(d_pb, partner_b, n_rand * sizeof(int)));
    }
    if (state_valid) {
        RC_TRY(up(d_lnL, lnlike, TW * sizeof(double)));
        RC_TRY(up(d_lnpi, lnprior, TW * sizeof(double)));
    } else {                                      // every rung's start positions in one batch of L T W F records
        const double* d_start_lnpi = c->d_lnprior;
        if (fields) RC_TRY(eval_fields_split_device(c, L, T * W, d_pos, d_lnL, st));
        else RC_TRY(eval_theta_split_device(c, joint, (int)TW, d_pos, nullptr, d_lnL, &d_start_lnpi, st));
        HIP_TRY(hipMemcpyAsync(d_lnpi, d_start_lnpi, TW * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    hipLaunchKernelGGL(k_pt_tempered, dim3(((int)TW + 255) / 256), dim3(256), 0, st, d_beta, d_lnL, d_lnpi, d_lnp,
                       (int)TW, W);
    if (accumulate) RC_TRY(stretch_prepare_accumulation(c));
    // one iteration is seven launches whatever T is: per half-step the T rungs' proposals (one k_theta_prep),
    // one pipeline pass over T half records, one accept kernel; then one swap kernel.  A joint fit adds one
    // proposal-and-prior kernel per half-step, whatever T and F are; its pass is over T half F records.  Several
    // ladders add one proposal kernel per half-step, whatever their number: the L T rungs' proposals
    // (k_pt_fields_propose), their records (one k_theta_prep launch, blockIdx.y the field), one pass over
    // L T half records, the accept kernel over L T ensembles; the swap kernel with one workgroup per ladder.
    // With moves every mode proposes with k_pt_move_propose and derives the records from d_q as given vectors:
    // one launch more per half-step for one-field and joint ladders, none more for several ladders
    const auto finish = joint ? k_pt_finish<true> : k_pt_finish<false>;     // (one-field: nf = 1 compiled in)
    const int move_blocks = (int)(((size_t)E * half * P + kMoveThreads - 1) / kMoveThreads);
    for (int it = 0; it < n_iter; ++it) {
        for (int h = 0; h < 2; ++h) {
            const int n = E * half;
            if (moves) {                          // by kind to d_q, then the records of the given vectors
                hipLaunchKernelGGL(k_pt_move_propose, dim3(move_blocks), dim3(kMoveThreads), 0, st, d_pos, d_q, d_kind,
                                   d_partner, d_pb, d_z, it, E, T, half, h, P);
                if (joint) launch_joint_records(c, n, d_q, st);
                else launch_theta_prep(c, T * half, d_q, nullptr, nullptr, st, StretchIn{}, 0, 0, L);
            } else if (joint) launch_joint_propose(c, d_pos, d_q, d_z, d_partner, it, T, half, h, st);
            else if (fields) {
                hipLaunchKernelGGL(k_pt_fields_propose, dim3(move_blocks), dim3(kMoveThreads), 0, st, d_pos, d_q, d_z,
                                   d_partner, it, E, half, h, P);
                launch_theta_prep(c, T * half, d_q, nullptr, nullptr, st, StretchIn{}, 0, 0, L);
            } else launch_theta_prep(c, n, nullptr, nullptr, nullptr, st,
                                     StretchIn{d_pos, d_q, d_z, d_partner, nullptr, it, half, h, 0, 0, 0, 0, T});
            RC_TRY(run_pipeline(c, n * F, c->d_skip, st));
            hipLaunchKernelGGL(finish, dim3(finish_blocks(n)), dim3(kFinishThreads), 0, st, c->d_partial,
                               c->d_skip, c->d_lnprior, c->nblk, d_beta, d_pos, d_lnL, d_lnpi, d_lnp, d_q, d_lz,
                               d_logu, d_nacc, it, E, half, h, P, F, n);
        }
        hipLaunchKernelGGL(k_pt_swap, dim3(L), dim3(kPtSwapThreads), 0, st, d_beta, d_pos, d_lnL, d_lnpi, d_lnp,
                           d_si, d_sj, d_slu, d_nswap, d_chain, d_lnpc, d_lnlc, d_lnqc, it, n_iter, T, W, P);
        if (accumulate && fields) {               // every ladder's beta = 1 rung, gathered: field f's sums
            hipLaunchKernelGGL(k_pt_gather_cold, dim3((int)(((size_t)L * W * P + kMoveThreads - 1) / kMoveThreads)),
                               dim3(kMoveThreads), 0, st, d_pos, d_q, L, T, W, P);
            launch_theta_prep(c, W, d_q, nullptr, nullptr, st, StretchIn{}, 0, 0, L);
            RC_TRY(accumulate_from_prep(c, W * L, st, 0, L, W));
        } else if (accumulate) {                  // the beta = 1 rung: the first W walkers, every field's sums
            if (joint) launch_theta_prep_joint(c, W, d_pos, nullptr, st);
            else launch_theta_prep(c, W, d_pos, nullptr, nullptr, st, StretchIn{});
            RC_TRY(accumulate_from_prep(c, W * F, st, 0, F, W));
        }
    }
    HIP_TRY(hipGetLastError());
    auto down = [&](void* dst, const void* src, size_t n) -> int {
        if (n) HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, st));
        return PSFMC_OK;
    };
    RC_TRY(down(pos, d_pos, TW * P * sizeof(double)));
    RC_TRY(down(lnlike, d_lnL, TW * sizeof(double)));
    RC_TRY(down(lnprior, d_lnpi, TW * sizeof(double)));
    RC_TRY(down(naccepted, d_nacc, TW * sizeof(long long)));
    if (T > 1) RC_TRY(down(nswap, d_nswap, (size_t)L * (T - 1) * sizeof(long long)));
    if (chain) RC_TRY(down(chain, d_chain, TW * n_iter * P * sizeof(double)));
    if (lnprob_chain) RC_TRY(down(lnprob_chain, d_lnpc, (size_t)L * W * n_iter * sizeof(double)));
    if (lnlike_chain) RC_TRY(down(lnlike_chain, d_lnlc, TW * n_iter * sizeof(double)));
    if (lnprior_chain) RC_TRY(down(lnprior_chain, d_lnqc, TW * n_iter * sizeof(double)));
    HIP_TRY(hipStreamSynchronize(st));
    if (hipGetLastError() != hipSuccess) return fail(PSFMC_EHIP, "kernel launch failed");
    return PSFMC_OK;
}

extern "C" int psfmc_pt_run(psfmc_ctx* c, int T, int W, int n_iter, const double* betas, double* pos,
                            double* lnlike, double* lnprior, int state_valid, const double* z, const double* lz,
                            const int* partner, const double* log_u, const int* swap_i, const int* swap_j,
                            const double* swap_log_u, double* chain, double* lnprob_chain, double* lnlike_chain,
                            double* lnprior_chain, long long* naccepted, long long* nswap, int accumulate) {
    return pt_run_impl(c, PT_ONE, T, W, n_iter, betas, pos, lnlike, lnprior, state_valid, z, lz, partner, log_u,
                       swap_i, swap_j, swap_log_u, chain, lnprob_chain, lnlike_chain, lnprior_chain, naccepted,
                       nswap, accumulate);
}

// psfmc_pt_run with the move of every iteration named (pt_run_impl): z the move's scalar, lz its Hastings term
extern "C" int psfmc_pt_move_run(psfmc_ctx* c, int T, int W, int n_iter, const double* betas, double* pos,
                                 double* lnlike, double* lnprior, int state_valid, const double* z, const double* lz,
                                 const int* partner, const double* log_u, const int* kind, const int* partner_b,
                                 const int* swap_i, const int* swap_j, const double* swap_log_u, double* chain,
                                 double* lnprob_chain, double* lnlike_chain, double* lnprior_chain,
                                 long long* naccepted, long long* nswap, int accumulate) {
    if (!kind || !partner_b) return fail(PSFMC_EINVAL, "NULL buffer");
    return pt_run_impl(c, PT_ONE, T, W, n_iter, betas, pos, lnlike, lnprior, state_valid, z, lz, partner, log_u,
                       swap_i, swap_j, swap_log_u, chain, lnprob_chain, lnlike_chain, lnprior_chain, naccepted,
                       nswap, accumulate, kind, partner_b);
}

// ---------------------------------------------------------------------------
// Joint fits: ONE parameter vector per walker for every field of the context (several exposures of one
// object, some parameters shared and some per field).  A walker is F field records -- field f's copy at
// f W + w of the per-walker arrays, an ordinary multi-field pass of the pipeline -- all derived from the
// same row of theta through each field's own slot -> column map.  Its log-posterior is
// ((ll_0 + ll_1) + ... + ll_{F-1}) + the joint log-prior, which k_joint_prior evaluates once per walker
// from the joint table (psfmc_set_joint_priors) and every field's axis-ratio rule; the fields' records
// take it as their `extra` from layouts whose own prior columns are all PRIOR_HOST (joint.fields), so a
// walker outside the joint support is skipped in every field and no prior is counted twice.
// ---------------------------------------------------------------------------
extern "C" int psfmc_set_joint_priors(psfmc_ctx* c, int n_params, const int* family, const double* params) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    for (int f = 0; f < c->n_fields; ++f) {
        if (!c->has_layout[f] || c->layouts[f].n_params != n_params)
            return fail(PSFMC_EINVAL, "field %d has no layout of %d columns (psfmc_set_layout[_field] first)", f,
                        n_params);
    }
    if (n_params < 1) return fail(PSFMC_EINVAL, "a joint fit needs at least one free parameter");
    std::vector<double> tab;
    RC_TRY(prior_table(n_params, family, params, tab));
    for (int i = 0; i < n_params; ++i)
        if (family[i] == PRIOR_HOST)
            return fail(PSFMC_EINVAL, "column %d: a joint prior needs a device family (PSFMC_PRIOR_UNIFORM ...)", i);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());                          // no launch may read the tables being replaced
    free_joint(c);
    psfmc_ctx::Joint& J = c->joint;
    const int P = n_params;
    // the prior table: family | pa | pb | pc | pd | pk
    const size_t fam_bytes = ((size_t)P * sizeof(int) + 7) / 8 * 8;
    void* blob = nullptr;
    HIP_TRY(hipMalloc(&blob, fam_bytes + tab.size() * sizeof(double)));
    J.blobs.push_back(blob);
    HIP_TRY(hipMemcpy(blob, family, P * sizeof(int), hipMemcpyHostToDevice));
    double* dp = reinterpret_cast<double*>(static_cast<unsigned char*>(blob) + fam_bytes);
    HIP_TRY(hipMemcpy(dp, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    J.prior = ThetaLayout{};
    J.prior.n_params = P;
    J.prior.family = static_cast<const int*>(blob);
    J.prior.pa = dp; J.prior.pb = dp + P; J.prior.pc = dp + 2 * P; J.prior.pd = dp + 3 * P; J.prior.pk = dp + 4 * P;
    // each field's layout blob (set_layout_impl: int tables from slot_col on, then the double tables) copied,
    // its prior families set to PRIOR_HOST
    const int ns = n_slots(c->layouts[0].n_sky, c->n_ps, c->n_sersic);
    const size_t int_bytes = (((size_t)ns + c->n_ps + c->n_sersic + P) * sizeof(int) + 7) / 8 * 8;
    const size_t bytes = int_bytes + ((size_t)ns + 5 * (size_t)P) * sizeof(double);
    for (int f = 0; f < c->n_fields; ++f) {
        const ThetaLayout& L = c->layouts[f];
        const unsigned char* old_base = reinterpret_cast<const unsigned char*>(L.slot_col);
        void* copy = nullptr;
        HIP_TRY(hipMalloc(&copy, bytes));
        J.blobs.push_back(copy);
        unsigned char* base = static_cast<unsigned char*>(copy);
        HIP_TRY(hipMemcpy(copy, old_base, bytes, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemset(base + (reinterpret_cast<const unsigned char*>(L.family) - old_base), 0, P * sizeof(int)));
        auto at = [&](const void* p) { return base + (static_cast<const unsigned char*>(p) - old_base); };
        ThetaLayout G = L;
        G.slot_col = reinterpret_cast<const int*>(at(L.slot_col));
        G.ps_method = reinterpret_cast<const int*>(at(L.ps_method));
        G.sersic_deg = reinterpret_cast<const int*>(at(L.sersic_deg));
        G.family = reinterpret_cast<const int*>(at(L.family));
        G.slot_const = reinterpret_cast<const double*>(at(L.slot_const));
        G.pa = reinterpret_cast<const double*>(at(L.pa));
        G.pb = reinterpret_cast<const double*>(at(L.pb));
        G.pc = reinterpret_cast<const double*>(at(L.pc));
        G.pd = reinterpret_cast<const double*>(at(L.pd));
        G.pk = reinterpret_cast<const double*>(at(L.pk));
        J.fields.push_back(G);
    }
    HIP_TRY(hipMalloc(&J.d_fields, (size_t)c->n_fields * sizeof(ThetaLayout)));
    HIP_TRY(hipMemcpy(J.d_fields, J.fields.data(), (size_t)c->n_fields * sizeof(ThetaLayout), hipMemcpyHostToDevice));
    if (!J.d_lp) HIP_TRY(hipMalloc(&J.d_lp, (size_t)c->max_walkers * sizeof(double)));
    J.ready = true;
    return PSFMC_OK;
}

static int eval_theta_joint(psfmc_ctx* c, int W, const double* d_theta, double* d_lnprob, hipStream_t st) {
    const int F = c->n_fields;
    launch_joint_records(c, W, d_theta, st);
    RC_TRY(run_pipeline(c, W * F, c->d_skip, st));
    hipLaunchKernelGGL(k_finish_posterior, dim3(finish_blocks(W)), dim3(kFinishThreads), 0, st, c->d_partial,
                       c->d_skip, c->d_lnprior, d_lnprob, W, c->nblk, F, W);
    HIP_TRY(hipGetLastError());
    return PSFMC_OK;
}

extern "C" int psfmc_eval_theta_joint_device(psfmc_ctx* c, int W, const double* d_theta, double* d_lnprob,
                                             void* stream) {
    RC_TRY(joint_check(c, W));
    if (W == 0) return PSFMC_OK;
    if (!d_theta || !d_lnprob) return fail(PSFMC_EINVAL, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    return eval_theta_joint(c, W, d_theta, d_lnprob, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int psfmc_eval_theta_joint(psfmc_ctx* c, int W, const double* theta, double* lnprob) {
    RC_TRY(joint_check(c, W));
    if (W == 0) return PSFMC_OK;
    if (!theta || !lnprob) return fail(PSFMC_EINVAL, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(c->d_theta, theta, (size_t)W * c->layouts[0].n_params * sizeof(double),
                           hipMemcpyHostToDevice, st));
    RC_TRY(eval_theta_joint(c, W, c->d_theta, c->d_like, st));
    HIP_TRY(hipMemcpyAsync(lnprob, c->d_like, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PSFMC_OK;
}

// psfmc_eval_theta_joint with the two terms apart: lnlike the fields' sum (walker_lnprob's, without the prior),
// lnprior the joint log-prior as k_joint_prior writes it
extern "C" int psfmc_eval_theta_joint_split(psfmc_ctx* c, int W, const double* theta, double* lnlike,
                                            double* lnprior) {
    RC_TRY(joint_check(c, W));
    if (W == 0) return PSFMC_OK;
    if (!theta || !lnlike || !lnprior) return fail(PSFMC_EINVAL, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(c->d_theta, theta, (size_t)W * c->layouts[0].n_params * sizeof(double),
                           hipMemcpyHostToDevice, st));
    const double* d_lnpi = nullptr;
    RC_TRY(eval_theta_split_device(c, true, W, c->d_theta, nullptr, c->d_like, &d_lnpi, st));
    HIP_TRY(hipMemcpyAsync(lnlike, c->d_like, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(lnprior, d_lnpi, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PSFMC_OK;
}

// psfmc_pt_run for every field of the context, each its own ladder of T ensembles of W walkers (pt_run_impl)
extern "C" int psfmc_pt_run_fields(psfmc_ctx* c, int T, int W, int n_iter, const double* betas, double* pos,
                                   double* lnlike, double* lnprior, int state_valid, const double* z,
                                   const double* lz, const int* partner, const double* log_u, const int* swap_i,
                                   const int* swap_j, const double* swap_log_u, double* chain, double* lnprob_chain,
                                   double* lnlike_chain, double* lnprior_chain, long long* naccepted,
                                   long long* nswap, int accumulate) {
    return pt_run_impl(c, PT_FIELDS, T, W, n_iter, betas, pos, lnlike, lnprior, state_valid, z, lz, partner, log_u,
                       swap_i, swap_j, swap_log_u, chain, lnprob_chain, lnlike_chain, lnprior_chain, naccepted,
                       nswap, accumulate);
}

// psfmc_pt_run for T ensembles of W joint walkers (pt_run_impl)
extern "C" int psfmc_pt_run_joint(psfmc_ctx* c, int T, int W, int n_iter, const double* betas, double* pos,
                                  double* lnlike, double* lnprior, int state_valid, const double* z,
                                  const double* lz, const int* partner, const double* log_u, const int* swap_i,
                                  const int* swap_j, const double* swap_log_u, double* chain, double* lnprob_chain,
                                  double* lnlike_chain, double* lnprior_chain, long long* naccepted,
                                  long long* nswap, int accumulate) {
    return pt_run_impl(c, PT_JOINT, T, W, n_iter, betas, pos, lnlike, lnprior, state_valid, z, lz, partner, log_u,
                       swap_i, swap_j, swap_log_u, chain, lnprob_chain, lnlike_chain, lnprior_chain, naccepted,
                       nswap, accumulate);
}

// psfmc_pt_move_run for every field of the context: kind [n_iter][n_fields], each ladder its own move
extern "C" int psfmc_pt_move_run_fields(psfmc_ctx* c, int T, int W, int n_iter, const double* betas, double* pos,
                                        double* lnlike, double* lnprior, int state_valid, const double* z,
                                        const double* lz, const int* partner, const double* log_u, const int* kind,
                                        const int* partner_b, const int* swap_i, const int* swap_j,
                                        const double* swap_log_u, double* chain, double* lnprob_chain,
                                        double* lnlike_chain, double* lnprior_chain, long long* naccepted,
                                        long long* nswap, int accumulate) {
    if (!kind || !partner_b) return fail(PSFMC_EINVAL, "NULL buffer");
    return pt_run_impl(c, PT_FIELDS, T, W, n_iter, betas, pos, lnlike, lnprior, state_valid, z, lz, partner, log_u,
                       swap_i, swap_j, swap_log_u, chain, lnprob_chain, lnlike_chain, lnprior_chain, naccepted,
                       nswap, accumulate, kind, partner_b);
}

// psfmc_pt_move_run for T ensembles of W joint walkers
extern "C" int psfmc_pt_move_run_joint(psfmc_ctx* c, int T, int W, int n_iter, const double* betas, double* pos,
                                       double* lnlike, double* lnprior, int state_valid, const double* z,
                                       const double* lz, const int* partner, const double* log_u, const int* kind,
                                       const int* partner_b, const int* swap_i, const int* swap_j,
                                       const double* swap_log_u, double* chain, double* lnprob_chain,
                                       double* lnlike_chain, double* lnprior_chain, long long* naccepted,
                                       long long* nswap, int accumulate) {
    if (!kind || !partner_b) return fail(PSFMC_EINVAL, "NULL buffer");
    return pt_run_impl(c, PT_JOINT, T, W, n_iter, betas, pos, lnlike, lnprior, state_valid, z, lz, partner, log_u,
                       swap_i, swap_j, swap_log_u, chain, lnprob_chain, lnlike_chain, lnprior_chain, naccepted,
                       nswap, accumulate, kind, partner_b);
}

// The plain half-step loop of psfmc_move_run (one-field walkers, proposals by kind), psfmc_stretch_run_joint and
// psfmc_move_run_joint (ONE ensemble of W joint walkers).  No whole-iteration launches and no hipGraph: a DE
// proposal of the second half depends on the outcomes of two walkers of the first, and the joint chain is the
// one of psfmc_stretch_run's rules either way.  A half-step: the proposals to S.q (k_move_propose, or
// k_joint_propose with their joint priors), their records (a joint walker's are F field records, F W / 2 in
// one pipeline pass), the pipeline, and k_stretch_finish, which sums each proposal's fields.  accumulate:
// after every iteration, each field's posterior-image sums get the current positions mapped to that field.
// One-field walkers come here only with moves: psfmc_stretch_run has its own loop (stretch_run_impl).
static int half_step_run(psfmc_ctx* c, bool joint, bool moves, int W, int n_iter, double* pos, double* lnprob,
                         int lnprob_valid, const double* z, const double* lz, const int* partner,
                         const double* log_u, const int* kind, const int* partner_b, double* chain,
                         double* lnprob_chain, long long* naccepted, int accumulate) {
    if (joint) {
        RC_TRY(joint_check(c, W));
        if (W < 2 || (W & 1)) return fail(PSFMC_EINVAL, "W must be even and >= 2");
    } else {
        RC_TRY(stretch_check(c, W, 1));              // one field, a layout, W even, every prior on the device
    }
    if (n_iter < 0 || !pos || !lnprob || !naccepted || (n_iter && (!z || !lz || !partner || !log_u)))
        return fail(PSFMC_EINVAL, "NULL buffer");
    if (moves) RC_TRY(moves_check(W, n_iter, kind, partner, partner_b));
    HIP_TRY(hipSetDevice(c->device));
    const int F = joint ? c->n_fields : 1, half = W / 2;
    hipStream_t st = c->stream;
    psfmc_ctx::Stretch& S = c->stretch;
    int rc = stretch_upload(c, W, n_iter, pos, lnprob, lnprob_valid, z, lz, partner, log_u, naccepted,
                            chain != nullptr, st);
    S.spec = false;
    if (rc == PSFMC_OK && moves) rc = moves_upload(c, kind, partner_b, st);
    if (rc == PSFMC_OK && !lnprob_valid)
        rc = joint ? eval_theta_joint(c, W, S.pos, S.lnp, st) : stretch_eval_positions(c, st);
    if (rc == PSFMC_OK && accumulate) rc = stretch_prepare_accumulation(c);
    for (int it = 0; it < n_iter && rc == PSFMC_OK; ++it) {
        for (int h = 0; h < 2 && rc == PSFMC_OK; ++h) {
            if (moves) move_propose(c, it, h, st);
            if (!joint) launch_theta_prep(c, half, S.q, nullptr, nullptr, st, StretchIn{});
            else if (moves) launch_joint_records(c, half, S.q, st);
            else launch_joint_propose(c, S.pos, S.q, S.rand, S.partner, it, 1, half, h, st);
            rc = run_pipeline(c, half * F, c->d_skip, st);
            if (rc == PSFMC_OK) stretch_accept(c, it, h, nullptr, false, st, F);
        }
        if (rc == PSFMC_OK && accumulate) {
            if (joint) launch_theta_prep_joint(c, W, S.pos, nullptr, st);
            else launch_theta_prep(c, W, S.pos, nullptr, nullptr, st, StretchIn{});
            rc = accumulate_from_prep(c, W * F, st, 0, F, W);
        }
    }
    return stretch_end_run(c, rc, pos, lnprob, chain, lnprob_chain, naccepted, st);
}

extern "C" int psfmc_move_run(psfmc_ctx* c, int W, int n_iter, double* pos, double* lnprob, int lnprob_valid,
                              const double* scal, const double* lz, const int* partner, const double* log_u,
                              const int* kind, const int* partner_b, double* chain, double* lnprob_chain,
                              long long* naccepted, int accumulate) {
    return half_step_run(c, false, true, W, n_iter, pos, lnprob, lnprob_valid, scal, lz, partner, log_u, kind,
                         partner_b, chain, lnprob_chain, naccepted, accumulate);
}

extern "C" int psfmc_stretch_run_joint(psfmc_ctx* c, int W, int n_iter, double* pos, double* lnprob,
                                       int lnprob_valid, const double* z, const double* lz, const int* partner,
                                       const double* log_u, double* chain, double* lnprob_chain,
                                       long long* naccepted, int accumulate) {
    return half_step_run(c, true, false, W, n_iter, pos, lnprob, lnprob_valid, z, lz, partner, log_u, nullptr,
                         nullptr, chain, lnprob_chain, naccepted, accumulate);
}

// psfmc_move_run for ONE ensemble of W joint walkers
extern "C" int psfmc_move_run_joint(psfmc_ctx* c, int W, int n_iter, double* pos, double* lnprob, int lnprob_valid,
                                    const double* scal, const double* lz, const int* partner, const double* log_u,
                                    const int* kind, const int* partner_b, double* chain, double* lnprob_chain,
                                    long long* naccepted, int accumulate) {
    return half_step_run(c, true, true, W, n_iter, pos, lnprob, lnprob_valid, scal, lz, partner, log_u, kind,
                         partner_b, chain, lnprob_chain, naccepted, accumulate);
}

// ---------------------------------------------------------------------------
// The same sampler, one half-step at a time, for walkers sharded over several GPUs: every
// rank holds ALL walkers and the same random numbers, evaluates the log-posterior of ITS
// block of each half-step's proposals, the blocks are all-gathered by the caller (RCCL /
// torch.distributed: the one collective of the path), and every rank applies the identical
// accept / move.  Per-walker log-posteriors do not depend on the batch they are evaluated
// in, so the chain equals the single-GPU chain bit for bit.
// ---------------------------------------------------------------------------
extern "C" int psfmc_stretch_open(psfmc_ctx* c, int W, int n_iter, const double* pos, const double* lnprob,
                                  const double* z, const double* lz, const int* partner,
                                  const double* log_u, const long long* naccepted, int store_chain) {
    RC_TRY(stretch_check(c, W));
    if (n_iter < 1 || !pos || !lnprob || !naccepted || !z || !lz || !partner || !log_u)
        return fail(PSFMC_EINVAL, "NULL buffer or n_iter < 1");
    RC_TRY(stretch_upload(c, W, n_iter, pos, lnprob, 1, z, lz, partner, log_u, naccepted, store_chain != 0,
                          c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PSFMC_OK;
}

// Between psfmc_stretch_open and the first psfmc_stretch_half_eval: the open run proposes by kind[it] (the
// arrays psfmc_move_run adds to psfmc_stretch_run's; open's z is the moves' scalar, its partner their first
// partner).  psfmc_stretch_half_eval then forms the half's proposals with k_move_propose.
extern "C" int psfmc_stretch_set_moves(psfmc_ctx* c, const int* kind, const int* partner_b) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    psfmc_ctx::Stretch& S = c->stretch;
    if (!S.open) return fail(PSFMC_EINVAL, "psfmc_stretch_open has not been called");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int> partner((size_t)S.n_iter * S.W);          // the first partners, as open uploaded them
    HIP_TRY(hipMemcpy(partner.data(), S.partner, partner.size() * sizeof(int), hipMemcpyDeviceToHost));
    RC_TRY(moves_check(S.W, S.n_iter, kind, partner.data(), partner_b));
    RC_TRY(moves_upload(c, kind, partner_b, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PSFMC_OK;
}

static int stretch_step_check(psfmc_ctx* c, int it, int h) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (!c->stretch.open) return fail(PSFMC_EINVAL, "psfmc_stretch_open has not been called");
    if (it < 0 || it >= c->stretch.n_iter || (h != 0 && h != 1))
        return fail(PSFMC_EINVAL, "iteration %d / half %d out of range", it, h);
    return PSFMC_OK;
}

extern "C" int psfmc_stretch_half_eval(psfmc_ctx* c, int it, int h, int lo, int n, double* d_newlnp_block,
                                       void* stream) {
    RC_TRY(stretch_step_check(c, it, h));
    const int half = c->stretch.W / 2;
    if (lo < 0 || n < 0 || lo + n > half) return fail(PSFMC_EINVAL, "block [%d, %d) outside the half-ensemble of %d", lo, lo + n, half);
    if (n > 0 && !d_newlnp_block) return fail(PSFMC_EINVAL, "NULL output");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (c->stretch.moves) move_propose_records(c, it, h, st);     // (psfmc_stretch_set_moves)
    else stretch_propose(c, it, h, false, st);
    if (n > 0) {
        RC_TRY(run_pipeline(c, n, c->d_skip, st, lo));
        hipLaunchKernelGGL(k_finish_posterior, dim3(finish_blocks(n)), dim3(kFinishThreads), 0, st,
                           c->d_partial + (size_t)lo * c->nblk, c->d_skip + lo, c->d_lnprior + lo,
                           d_newlnp_block, n, c->nblk, 1, 0);
    }
    HIP_TRY(hipGetLastError());
    return PSFMC_OK;
}

extern "C" int psfmc_stretch_half_accept(psfmc_ctx* c, int it, int h, const double* d_newlnp_half, void* stream) {
    RC_TRY(stretch_step_check(c, it, h));
    if (!d_newlnp_half) return fail(PSFMC_EINVAL, "NULL input");
    HIP_TRY(hipSetDevice(c->device));
    stretch_accept(c, it, h, d_newlnp_half, false, stream ? (hipStream_t)stream : c->stream);
    HIP_TRY(hipGetLastError());
    return PSFMC_OK;
}

extern "C" int psfmc_stretch_accumulate(psfmc_ctx* c, int lo, int n, void* stream) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    psfmc_ctx::Stretch& S = c->stretch;
    if (!S.open) return fail(PSFMC_EINVAL, "psfmc_stretch_open has not been called");
    if (lo < 0 || n < 0 || lo + n > S.W) return fail(PSFMC_EINVAL, "block outside the ensemble");
    if (n == 0) return PSFMC_OK;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    RC_TRY(stretch_prepare_accumulation(c));
    launch_theta_prep(c, n, S.pos + (size_t)lo * c->layouts[0].n_params, nullptr, nullptr, st, StretchIn{});
    RC_TRY(accumulate_from_prep(c, n, st));
    HIP_TRY(hipGetLastError());
    return PSFMC_OK;
}

extern "C" int psfmc_stretch_close(psfmc_ctx* c, double* pos, double* lnprob, double* chain,
                                   double* lnprob_chain, long long* naccepted, void* stream) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (!c->stretch.open) return fail(PSFMC_EINVAL, "psfmc_stretch_open has not been called");
    if (!pos || !lnprob || !naccepted) return fail(PSFMC_EINVAL, "NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    const int rc = stretch_download(c, pos, lnprob, chain, lnprob_chain, naccepted,
                                    stream ? (hipStream_t)stream : c->stream);
    c->stretch.open = false;
    return rc;
}

// raw sums of the posterior images ([4][ny][nx]: raw, convolved, model variance, PS-only
// convolved) and their sample count, for adding up the ranks' shares
extern "C" int psfmc_get_accumulated_sums(psfmc_ctx* c, double* sums, long long* count) {
    if (!c || !sums || !count) return fail(PSFMC_EINVAL, "NULL argument");
    if (c->n_fields > 1) return fail(PSFMC_EINVAL, "this entry point serves contexts of one field");
    HIP_TRY(hipSetDevice(c->device));
    RC_TRY(flush_linear_sums(c));
    *count = c->acc_count[0];
    const WrapDesc& wr = c->wraps[0];
    const size_t S_img = img_pixels(c, 0);
    if (!c->d_acc) { memset(sums, 0, 4 * S_img * sizeof(double)); return PSFMC_OK; }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!c->embed) {
        HIP_TRY(hipMemcpy(sums, c->d_acc, 4 * S_img * sizeof(double), hipMemcpyDeviceToHost));
        return PSFMC_OK;
    }
    std::vector<double> full((size_t)4 * c->S);              // transform shape -> the image's window
    HIP_TRY(hipMemcpy(full.data(), c->d_acc, full.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; ++k)
        for (int y = 0; y < wr.ly; ++y)
            memcpy(sums + k * S_img + (size_t)y * wr.lx,
                   &full[(size_t)k * c->S + (size_t)(y + wr.ay) * c->nx + wr.ax], (size_t)wr.lx * sizeof(double));
    return PSFMC_OK;
}

extern "C" int psfmc_set_accumulated_sums(psfmc_ctx* c, const double* sums, long long count) {
    if (!c || !sums || count < 0) return fail(PSFMC_EINVAL, "bad argument");
    if (c->n_fields > 1) return fail(PSFMC_EINVAL, "this entry point serves contexts of one field");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->d_acc) RC_TRY(psfmc_reset_accumulated(c));
    if (c->d_lin) HIP_TRY(hipMemset(c->d_lin, 0, (size_t)c->n_psf * 3 * c->S * sizeof(double)));
    c->lin_pending = 0;                                  // the new sums replace everything gathered so far
    if (!c->embed) {
        HIP_TRY(hipMemcpy(c->d_acc, sums, (size_t)4 * c->S * sizeof(double), hipMemcpyHostToDevice));
    } else {
        const WrapDesc& wr = c->wraps[0];
        const size_t S_img = img_pixels(c, 0);
        std::vector<double> full((size_t)4 * c->S, 0.0);     // only the image's window is ever read back
        for (int k = 0; k < 4; ++k)
            for (int y = 0; y < wr.ly; ++y)
                memcpy(&full[(size_t)k * c->S + (size_t)(y + wr.ay) * c->nx + wr.ax],
                       sums + k * S_img + (size_t)y * wr.lx, (size_t)wr.lx * sizeof(double));
        HIP_TRY(hipMemcpy(c->d_acc, full.data(), full.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    c->acc_count[0] = count;
    return PSFMC_OK;
}

static int get_accumulated_impl(psfmc_ctx* c, int field, double* raw, double* conv, double* resid, double* ivm,
                                double* ps_sub, long long* count) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (field < 0 || field >= c->n_fields) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    const long long n = c->acc_count[field];
    if (count) *count = n;
    if (n == 0 || !c->d_acc) return PSFMC_OK;
    HIP_TRY(hipSetDevice(c->device));
    RC_TRY(flush_linear_sums(c));
    double* d_out = nullptr;
    const size_t S_img = img_pixels(c, field);              // the field's own image shape
    HIP_TRY(hipMalloc(&d_out, S_img * sizeof(double)));
    const double inv_n = 1.0 / (double)n;
    const size_t px = (size_t)field * c->S;                 // this field's pixels in d_sci / d_var
    struct { double* host; int slot, op; } outs[] = {{raw, 0, 0}, {conv, 1, 0}, {resid, 1, 1},
                                                     {ivm, 2, 2}, {ps_sub, 3, 1}};
    int rc = PSFMC_OK;
    for (auto& o : outs) {
        if (!o.host) continue;
        hipLaunchKernelGGL(k_accumulated_out, dim3(256), dim3(256), 0, c->stream,
                           c->d_acc + ((size_t)field * 4 + o.slot) * c->S, c->d_sci + px, c->d_var + px, d_out,
                           inv_n, o.op, img_window(c, field));
        if (hipMemcpyAsync(o.host, d_out, S_img * sizeof(double), hipMemcpyDeviceToHost, c->stream) !=
                hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
            rc = fail(PSFMC_EHIP, "accumulated image copy failed");
            break;
        }
    }
    (void)hipFree(d_out);
    return rc;
}

extern "C" int psfmc_get_accumulated(psfmc_ctx* c, double* raw, double* conv, double* resid, double* ivm,
                                     double* ps_sub, long long* count) {
    return get_accumulated_impl(c, 0, raw, conv, resid, ivm, ps_sub, count);
}

// the posterior images of one field of a psfmc_ctx_create_fields context
extern "C" int psfmc_get_accumulated_field(psfmc_ctx* c, int field, double* raw, double* conv, double* resid,
                                           double* ivm, double* ps_sub, long long* count) {
    return get_accumulated_impl(c, field, raw, conv, resid, ivm, ps_sub, count);
}

extern "C" int psfmc_get_spectra(psfmc_ctx* c, double* psf_spec, double* var_spec) {
    if (!c || !psf_spec || !var_spec) return fail(PSFMC_EINVAL, "NULL argument");
    if (c->embed) return fail(PSFMC_EINVAL, "the image is embedded in a %d x %d transform: its kernel spectra are not "
                              "those of the %d x %d image", c->ny, c->nx, c->wraps[0].ly, c->wraps[0].lx);
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)c->n_psf * c->F * sizeof(double2);
    if (c->backend == PSFMC_BACKEND_HIPFFT) {
        HIP_TRY(hipMemcpy(psf_spec, c->d_pspec, bytes, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(var_spec, c->d_vspec, bytes, hipMemcpyDeviceToHost));
        return PSFMC_OK;
    }
    cd* tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, bytes));
    int rc = PSFMC_OK;
    for (int comp = 0; comp < 2 && rc == PSFMC_OK; ++comp) {
        hipLaunchKernelGGL(k_untranspose_spectrum, dim3(256), dim3(256), 0, c->stream, c->d_Kraw, tmp,
                           c->n_psf, comp, c->ny, c->nxh, c->rg_log2, c->d_rho);
        if (hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(comp ? var_spec : psf_spec, tmp, bytes, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(PSFMC_EHIP, "spectrum copy failed");
    }
    (void)hipFree(tmp);
    return rc;
}

// ---------------------------------------------------------------------------
// psfmc_group: ONE process driving several GPUs: a context per
// device with the field replicated, walkers split into contiguous blocks, every device's
// upload / evaluation / download enqueued on its own stream before any is waited for, the
// blocks landing at their offsets of the caller's host array (for a host-side result that
// is the whole "gather"; the one-process-per-GPU form with an RCCL all-gather of device
// tensors is psfmc_amd/parallel.py).
// ---------------------------------------------------------------------------
struct psfmc_group {
    std::vector<psfmc_ctx*> ctx;
};

static void group_block(int W, int n, int r, int* lo, int* hi) {
    const int base = W / n, extra = W % n;
    *lo = r * base + (r < extra ? r : extra);
    *hi = *lo + base + (r < extra ? 1 : 0);
}

extern "C" int psfmc_group_create(psfmc_group** out, int n_dev, const int* devices, int ny, int nx,
                                  const double* sci, const double* obs_var, const uint8_t* bad_px,
                                  int n_psf, int psf_ny, int psf_nx, const double* psf,
                                  const double* psf_var, int n_ps, int n_sersic, int max_walkers,
                                  int backend) {
    if (!out) return fail(PSFMC_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_dev < 1 || n_dev > 64 || !devices) return fail(PSFMC_EINVAL, "need 1..64 devices");
    psfmc_group* g = new psfmc_group;
    // every device may be handed the whole batch's share rounded up
    const int per_dev = (max_walkers + n_dev - 1) / n_dev;
    for (int i = 0; i < n_dev; ++i) {
        psfmc_ctx* c = nullptr;
        const int rc = psfmc_ctx_create(&c, devices[i], ny, nx, sci, obs_var, bad_px, n_psf, psf_ny, psf_nx,
                                        psf, psf_var, n_ps, n_sersic, per_dev < 1 ? 1 : per_dev, backend);
        if (rc != PSFMC_OK) {
            const std::string keep = g_err;
            for (psfmc_ctx* d : g->ctx) psfmc_ctx_destroy(d);
            delete g;
            g_err = keep;
            return rc;
        }
        g->ctx.push_back(c);
    }
    *out = g;
    return PSFMC_OK;
}

extern "C" int psfmc_group_destroy(psfmc_group* g) {
    if (!g) return PSFMC_OK;
    for (psfmc_ctx* c : g->ctx) psfmc_ctx_destroy(c);
    delete g;
    return PSFMC_OK;
}

extern "C" int psfmc_group_size(const psfmc_group* g) { return g ? (int)g->ctx.size() : PSFMC_EINVAL; }

extern "C" int psfmc_group_set_layout(psfmc_group* g, int n_sky, int n_params, const int* slot_col,
                                      const double* slot_const, const int* ps_method,
                                      const int* sersic_degrees, double mag_zeropoint, const int* family,
                                      const double* p0, const double* p1, const double* p2) {
    if (!g) return fail(PSFMC_EINVAL, "group is NULL");
    for (psfmc_ctx* c : g->ctx)
        RC_TRY(psfmc_set_layout(c, n_sky, n_params, slot_col, slot_const, ps_method, sersic_degrees,
                                mag_zeropoint, family, p0, p1, p2));
    return PSFMC_OK;
}

extern "C" int psfmc_group_set_priors(psfmc_group* g, int n_params, const int* family, const double* params) {
    if (!g) return fail(PSFMC_EINVAL, "group is NULL");
    for (psfmc_ctx* c : g->ctx) RC_TRY(psfmc_set_priors(c, 0, n_params, family, params));
    return PSFMC_OK;
}

extern "C" int psfmc_group_set_ties(psfmc_group* g, int n_ties, const int* src_col, const int* ratio_col,
                                    const double* ratio_const, const int* offset_col, const double* offset_const) {
    if (!g) return fail(PSFMC_EINVAL, "group is NULL");
    for (psfmc_ctx* c : g->ctx)
        RC_TRY(psfmc_set_ties(c, 0, n_ties, src_col, ratio_col, ratio_const, offset_col, offset_const));
    return PSFMC_OK;
}

extern "C" int psfmc_group_set_aux_layout(psfmc_group* g, int n_aux, const int* aux_col, const double* aux_const,
                                          const int* sky_slope_flags, const int* sersic_general_flags) {
    if (!g) return fail(PSFMC_EINVAL, "group is NULL");
    for (psfmc_ctx* c : g->ctx)
        RC_TRY(psfmc_set_aux_layout(c, 0, n_aux, aux_col, aux_const, sky_slope_flags, sersic_general_flags));
    return PSFMC_OK;
}

// block b of the one field of every context of the group
static int group_set_block_layout(psfmc_group* g, int b, int n_sersic, const int* tags, const int* col,
                                  const double* konst) {
    if (!g) return fail(PSFMC_EINVAL, "group is NULL");
    for (psfmc_ctx* c : g->ctx) RC_TRY(set_block_layout(c, b, 0, n_sersic, tags, col, konst));
    return PSFMC_OK;
}

extern "C" int psfmc_group_set_fourier_layout(psfmc_group* g, int n_sersic, const int* mode_mask, const int* col,
                                              const double* konst) {
    return group_set_block_layout(g, kBlkFou, n_sersic, mode_mask, col, konst);
}

extern "C" int psfmc_group_set_spiral_layout(psfmc_group* g, int n_sersic, const int* flags, const int* col,
                                             const double* konst) {
    return group_set_block_layout(g, kBlkSpi, n_sersic, flags, col, konst);
}

extern "C" int psfmc_group_set_radial_layout(psfmc_group* g, int n_sersic, const int* kinds, const int* col,
                                             const double* konst) {
    return group_set_block_layout(g, kBlkRad, n_sersic, kinds, col, konst);
}

extern "C" int psfmc_group_set_truncation_layout(psfmc_group* g, int n_sersic, const int* flags, const int* col,
                                                 const double* konst) {
    return group_set_block_layout(g, kBlkTru, n_sersic, flags, col, konst);
}

extern "C" int psfmc_group_set_bending_layout(psfmc_group* g, int n_sersic, const int* mode_mask, const int* col,
                                              const double* konst) {
    return group_set_block_layout(g, kBlkBnd, n_sersic, mode_mask, col, konst);
}

extern "C" int psfmc_group_set_general_mean(psfmc_group* g, int n_sersic, const int* flags) {
    if (!g) return fail(PSFMC_EINVAL, "group is NULL");
    for (psfmc_ctx* c : g->ctx) RC_TRY(psfmc_set_general_mean(c, 0, n_sersic, flags));
    return PSFMC_OK;
}

extern "C" int psfmc_group_set_sersic_integrate(psfmc_group* g, int n_sersic, const int* integrate) {
    if (!g) return fail(PSFMC_EINVAL, "group is NULL");
    for (psfmc_ctx* c : g->ctx) RC_TRY(psfmc_set_sersic_integrate(c, 0, n_sersic, integrate));
    return PSFMC_OK;
}

// rows != nullptr: log-likelihoods of derived rows; else log-posteriors of raw vectors
static int group_eval(psfmc_group* g, int W, const double* rows, const uint8_t* skip, const double* theta,
                      const double* extra, double* out) {
    if (!g) return fail(PSFMC_EINVAL, "group is NULL");
    if (W < 0 || (W > 0 && (!out || (!rows && !theta)))) return fail(PSFMC_EINVAL, "bad argument");
    const int n = (int)g->ctx.size();
    int rc = PSFMC_OK;
    // one device's share: enqueue its copies and kernels.  An error ends the enqueueing but NEVER
    // skips the synchronize loop below: earlier devices still have copies in flight out of `theta`
    // / `rows` and into `out`, which the caller may free as soon as this function returns.
    auto enqueue = [&](int r) -> int {
        int lo, hi;
        group_block(W, n, r, &lo, &hi);
        psfmc_ctx* c = g->ctx[r];
        const int w = hi - lo;
        if (w == 0) return PSFMC_OK;
        if (w > c->max_walkers) return fail(PSFMC_EINVAL, "W=%d exceeds the group's max_walkers", W);
        HIP_TRY(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        if (rows) {
            HIP_TRY(hipMemcpyAsync(c->d_rows, rows + (size_t)lo * c->rlen, (size_t)w * c->rlen * sizeof(double),
                                   hipMemcpyHostToDevice, st));
            if (skip) HIP_TRY(hipMemcpyAsync(c->d_skip, skip + lo, (size_t)w, hipMemcpyHostToDevice, st));
            RC_TRY(eval_device(c, w, c->d_rows, skip ? c->d_skip : nullptr, c->d_like, st));
        } else {
            RC_TRY(check_theta_call(c, w, theta, out));
            const int P = c->layouts[0].n_params;
            if (P) HIP_TRY(hipMemcpyAsync(c->d_theta, theta + (size_t)lo * P, (size_t)w * P * sizeof(double),
                                          hipMemcpyHostToDevice, st));
            if (extra) HIP_TRY(hipMemcpyAsync(c->d_extra, extra + lo, (size_t)w * sizeof(double),
                                              hipMemcpyHostToDevice, st));
            RC_TRY(eval_theta_device(c, w, c->d_theta, extra ? c->d_extra : nullptr, c->d_like, st));
        }
        HIP_TRY(hipMemcpyAsync(out + lo, c->d_like, (size_t)w * sizeof(double), hipMemcpyDeviceToHost, st));
        return PSFMC_OK;
    };
    std::string first_error;
    for (int r = 0; r < n && rc == PSFMC_OK; ++r) {          // enqueue everything ...
        rc = enqueue(r);
        if (rc != PSFMC_OK) first_error = psfmc_last_error();
    }
    for (int r = 0; r < n; ++r) {                             // ... then wait for every device
        psfmc_ctx* c = g->ctx[r];
        if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
            if (rc == PSFMC_OK) rc = fail(PSFMC_EHIP, "device %d failed: %s", c->device,
                                          hipGetErrorString(hipGetLastError()));
    }
    if (!first_error.empty()) (void)fail(rc, "%s", first_error.c_str());   // the enqueue error is the one to report
    return rc;
}

extern "C" int psfmc_group_eval_batch(psfmc_group* g, int W, const double* rows, const uint8_t* skip,
                                      double* loglike) {
    if (W > 0 && !rows) return fail(PSFMC_EINVAL, "NULL rows");
    return group_eval(g, W, rows, skip, nullptr, nullptr, loglike);
}

extern "C" int psfmc_group_eval_theta(psfmc_group* g, int W, const double* theta, const double* extra_lnprior,
                                      double* lnprob) {
    if (W > 0 && !theta) return fail(PSFMC_EINVAL, "NULL theta");
    return group_eval(g, W, nullptr, nullptr, theta, extra_lnprior, lnprob);
}

// ---------------------------------------------------------------------------
// Fisher matrix and gradient of stencils of walkers (psfmc_fisher.h): the image flow of psfmc_eval_images, each pass's
// images stashed, then one Gram launch over every stencil
// ---------------------------------------------------------------------------
extern "C" int psfmc_fisher_rows(psfmc_ctx* c, int field, int n_base, int K, const double* rows, const double* inv2h,
                                 double* F, double* g, double* lnlike) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (field < 0 || field >= c->n_fields) return fail(PSFMC_EINVAL, "field %d of %d", field, c->n_fields);
    if (!rows || !inv2h || !F || !g || !lnlike) return fail(PSFMC_EINVAL, "NULL buffer");
    if (c->t_f32)
        return fail(PSFMC_EINVAL, "psfmc_fisher_rows needs fp64 storage: differences of complex64-stored images over a "
                    "1e-4 step are rounding noise");
    const int n_pix = (int)img_pixels(c, field);
    FisherPlan plan;
    if (const char* why = fisher_plan(n_base, K, c->max_walkers, (size_t)n_pix, &plan))
        return fail(PSFMC_EINVAL, "psfmc_fisher_rows: %s (n_base=%d, K=%d, max_walkers=%d)", why, n_base, K,
                    c->max_walkers);
    const int W = plan.W;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const bool fused = c->backend == PSFMC_BACKEND_FUSED;
    const size_t px = (size_t)field * c->S;                          // this field's pixels
    RC_TRY(images_begin(c, field, W, rows, st));
    psfmc_ctx::Fisher& fi = c->fisher;
    RC_TRY(grow(&fi.stash, &fi.cap_stash, plan.stash_doubles));
    RC_TRY(grow(&fi.partial, &fi.cap_partial, plan.partial_doubles));
    RC_TRY(grow(&fi.io, &fi.cap_io, plan.io_doubles));
    double* d_inv2h = fi.io;
    double* d_F = d_inv2h + (size_t)n_base * K;
    double* d_g = d_F + (size_t)n_base * K * K;
    HIP_TRY(hipMemcpyAsync(d_inv2h, inv2h, (size_t)n_base * K * sizeof(double), hipMemcpyHostToDevice, st));
    // where the convolved model / model variance of walker w live after a pass (as eval_images_impl)
    const double* conv_src = fused ? c->d_img0 : c->d_real;
    const double* var_src = fused ? c->d_img1 : c->d_real;
    const int stride = fused ? 1 : 2, var_c = fused ? 0 : 1;
    for (int w0 = 0; w0 < W; w0 += c->chunk) {
        const int n = W - w0 < c->chunk ? W - w0 : c->chunk;
        const double* prep = c->d_prep + (size_t)w0 * c->plen;
        double* partial = c->d_partial + (size_t)w0 * c->nblk;
        RC_TRY(image_pass(c, n, prep, 0, nullptr, partial, st));
        if (!fused)
            hipLaunchKernelGGL(k_chi2, dim3(c->nblk, n), dim3(256), 0, st, c->d_real, c->d_sci + px, c->d_var + px,
                               c->d_bad + px, (const uint8_t*)nullptr, partial, c->S);
        hipLaunchKernelGGL(k_fisher_stash, dim3(16, n), dim3(256), 0, st, conv_src, var_src,
                           fi.stash + (size_t)w0 * 2 * n_pix, c->S, stride, var_c, img_window(c, field));
    }
    hipLaunchKernelGGL(k_finish, dim3(finish_blocks(W)), dim3(kFinishThreads), 0, st, c->d_partial,
                       (const uint8_t*)nullptr, c->d_like, W, c->nblk);
    const FisherStencil src{fi.stash, d_inv2h, c->d_sci + px, c->d_var + px, c->d_bad + px, img_window(c, field)};
    launch_fisher_gram(src, n_base, K, n_pix, plan, fi.partial, d_F, d_g, st);
    HIP_TRY(hipGetLastError());
    std::vector<double> like(W);
    HIP_TRY(hipMemcpyAsync(F, d_F, (size_t)n_base * K * K * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(g, d_g, (size_t)n_base * K * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(like.data(), c->d_like, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int b = 0; b < n_base; ++b) lnlike[b] = like[(size_t)b * (2 * K + 1)];
    return PSFMC_OK;
}

// Stencils of different fields in one call (psfmc_fisher_rows_fields; with `joint`, psfmc_fisher_rows_joint): the
// records derived per run of equal field (as fields_records_pass derives them from theta), the image passes over
// the mixed records -- fused_forward / fused_inverse take a record's field from its kernel-spectrum index, as the
// log-posterior pipeline's mixed passes do, and write walker w's images to image w of d_img0 / d_img1 whatever its
// field -- each pass stashed through the stencils' table, then ONE Gram and ONE finish launch (and the link).
struct FisherJointCall {
    int n_base, K_joint;
    const int* field_col;            // host [n_fields][K_joint] (fisher_joint_plan)
    FisherJointPlan plan;
};
static int fisher_fields_impl(psfmc_ctx* c, const char* who, int n_stencils, int K, const int* field,
                              const double* rows, const double* inv2h, double* F, double* g, double* lnlike,
                              const FisherJointCall* joint) {
    if (c->backend != PSFMC_BACKEND_FUSED)
        return fail(PSFMC_EINVAL, "%s serves the fused back end (every shared context's)", who);
    if (c->t_f32)
        return fail(PSFMC_EINVAL, "%s needs fp64 storage: differences of complex64-stored images over a 1e-4 step are "
                    "rounding noise", who);
    std::vector<FisherFieldShape> shapes(c->n_fields);
    for (int f = 0; f < c->n_fields; ++f) {
        const WrapDesc& w = c->wraps[f];
        shapes[f] = FisherFieldShape{(long long)((size_t)f * c->S), c->ny, c->nx, w.ly, w.lx, w.ay, w.ax};
    }
    std::vector<FisherFieldRec> recs(n_stencils > 0 ? n_stencils : 0);
    FisherFieldsPlan plan;
    if (const char* why = fisher_fields_plan(n_stencils, K, c->max_walkers, c->n_fields, field, shapes.data(),
                                             recs.data(), &plan))
        return fail(PSFMC_EINVAL, "%s: %s (n_stencils=%d, K=%d, max_walkers=%d)", who, why, n_stencils, K,
                    c->max_walkers);
    const int W = plan.W, n_st = 2 * K + 1;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    RC_TRY(take_aux_rows(c, W));
    HIP_TRY(hipMemcpyAsync(c->d_rows, rows, (size_t)W * c->rlen * sizeof(double), hipMemcpyHostToDevice, st));
    c->prep_tabs_valid = false;                       // d_prep is being rewritten
    for (int s0 = 0; s0 < n_stencils;) {              // one record derivation per run of stencils of one field
        int s1 = s0 + 1;
        while (s1 < n_stencils && field[s1] == field[s0]) ++s1;
        const int f = field[s0], w_lo = s0 * n_st, n = (s1 - s0) * n_st;
        hipLaunchKernelGGL(k_prep, dim3((n + 127) / 128), dim3(128), 0, st, c->d_rows + (size_t)w_lo * c->rlen,
                           c->d_prep + (size_t)w_lo * c->plen, n, c->n_ps, c->n_sersic, c->wraps[f].ly, c->wraps[f].lx,
                           c->d_rho, c->n_psf_field, f * c->n_psf_field);
        launch_pow_tables(c, n, w_lo, nullptr, st);
        s0 = s1;
    }
    RC_TRY(ensure_image_staging(c));
    psfmc_ctx::Fisher& fi = c->fisher;
    RC_TRY(grow(&fi.stash, &fi.cap_stash, plan.stash_doubles));
    RC_TRY(grow(&fi.partial, &fi.cap_partial, plan.partial_doubles));
    RC_TRY(grow(&fi.io, &fi.cap_io, plan.io_doubles));
    RC_TRY(grow(&fi.recs, &fi.cap_recs, (size_t)n_stencils));
    if (joint) {
        RC_TRY(grow(&fi.field_col, &fi.cap_field_col, (size_t)c->n_fields * joint->K_joint));
        RC_TRY(grow(&fi.link, &fi.cap_link, joint->plan.link_doubles));
    }
    double* d_inv2h = fi.io;
    double* d_F = fi.io + fisher_fields_F_at(n_stencils, K, 0);
    double* d_g = fi.io + fisher_fields_g_at(n_stencils, K, 0);
    HIP_TRY(hipMemcpyAsync(d_inv2h, inv2h, (size_t)n_stencils * K * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(fi.recs, recs.data(), (size_t)n_stencils * sizeof(FisherFieldRec), hipMemcpyHostToDevice, st));
    for (int w0 = 0; w0 < W; w0 += c->chunk) {
        const int n = W - w0 < c->chunk ? W - w0 : c->chunk;
        const int rc = image_pass(c, n, c->d_prep + (size_t)w0 * c->plen, 0, nullptr,
                                  c->d_partial + (size_t)w0 * c->nblk, st);
        if (rc != PSFMC_OK) {                         // (the table's copy out of `recs` may still be in flight)
            (void)hipStreamSynchronize(st);
            return rc;
        }
        hipLaunchKernelGGL(k_fisher_stash_fields, dim3(16, n), dim3(256), 0, st, c->d_img0, c->d_img1, fi.stash, c->S,
                           fi.recs, w0, n_st);
    }
    hipLaunchKernelGGL(k_finish, dim3(finish_blocks(W)), dim3(kFinishThreads), 0, st, c->d_partial,
                       (const uint8_t*)nullptr, c->d_like, W, c->nblk);
    const FisherFieldStencils src{fi.recs, fi.stash, d_inv2h, c->d_sci, c->d_var, c->d_bad};
    launch_fisher_gram_fields(src, K, plan, fi.partial, d_F, d_g, st);
    std::vector<double> like(W);
    if (joint) {
        const int nf = c->n_fields, Kj = joint->K_joint;
        HIP_TRY(hipMemcpyAsync(fi.field_col, joint->field_col, (size_t)nf * Kj * sizeof(int), hipMemcpyHostToDevice, st));
        const size_t n_el = joint->plan.link_elems;
        hipLaunchKernelGGL(k_fisher_link, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, st, d_F, d_g, fi.field_col,
                           joint->n_base, nf, Kj, K, n_el, fi.link);
        HIP_TRY(hipGetLastError());
        const size_t nF = (size_t)joint->n_base * Kj * Kj;
        HIP_TRY(hipMemcpyAsync(F, fi.link, nF * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(g, fi.link + nF, (size_t)joint->n_base * Kj * sizeof(double), hipMemcpyDeviceToHost, st));
    } else {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(F, d_F, (size_t)n_stencils * K * K * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(g, d_g, (size_t)n_stencils * K * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(like.data(), c->d_like, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (joint) {                                      // ((ll_0 + ll_1) + ...) + ll_{F-1}, psfmc_eval_theta_joint_split's sum
        const int nf = c->n_fields;
        for (int b = 0; b < joint->n_base; ++b) {
            double ll = like[(size_t)b * nf * n_st];
            for (int f = 1; f < nf; ++f) ll += like[((size_t)b * nf + f) * n_st];
            lnlike[b] = ll;
        }
    } else {
        for (int s = 0; s < n_stencils; ++s) lnlike[s] = like[(size_t)s * n_st];
    }
    return PSFMC_OK;
}

extern "C" int psfmc_fisher_rows_fields(psfmc_ctx* c, int n_stencils, int K, const int* field, const double* rows,
                                        const double* inv2h, double* F, double* g, double* lnlike) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (!field || !rows || !inv2h || !F || !g || !lnlike) return fail(PSFMC_EINVAL, "NULL buffer");
    return fisher_fields_impl(c, "psfmc_fisher_rows_fields", n_stencils, K, field, rows, inv2h, F, g, lnlike, nullptr);
}

extern "C" int psfmc_fisher_rows_joint(psfmc_ctx* c, int n_base, int K_joint, int K_field, const int* col_of,
                                       const double* rows, const double* inv2h, double* F, double* g, double* lnlike) {
    if (!c) return fail(PSFMC_EINVAL, "ctx is NULL");
    if (!col_of || !rows || !inv2h || !F || !g || !lnlike) return fail(PSFMC_EINVAL, "NULL buffer");
    const int nf = c->n_fields;
    FisherJointCall joint{n_base, K_joint, nullptr, FisherJointPlan{}};
    std::vector<int> field_col;
    if (K_joint >= 1 && K_joint <= (1 << 20)) field_col.resize((size_t)nf * K_joint);
    if (const char* why = fisher_joint_plan(n_base, nf, K_joint, K_field, c->max_walkers, col_of,
                                            field_col.empty() ? nullptr : field_col.data(), &joint.plan))
        return fail(PSFMC_EINVAL, "psfmc_fisher_rows_joint: %s (n_base=%d, n_fields=%d, K_joint=%d, K_field=%d, "
                    "max_walkers=%d)", why, n_base, nf, K_joint, K_field, c->max_walkers);
    joint.field_col = field_col.data();
    std::vector<int> field((size_t)joint.plan.n_stencils);
    for (size_t s = 0; s < field.size(); ++s) field[s] = (int)(s % nf);
    return fisher_fields_impl(c, "psfmc_fisher_rows_joint", joint.plan.n_stencils, K_field, field.data(), rows, inv2h,
                              F, g, lnlike, &joint);
}

// the Gram and finish kernels alone on caller-supplied vectors: a, b [K][n_pix], c, d [n_pix] -> F [K][K], g [K]
extern "C" int psfmc_debug_fisher_gram(int device, int K, int n_pix, const double* a, const double* b, const double* c,
                                       const double* d, double* F, double* g) {
    if (!a || !b || !c || !d || !F || !g) return fail(PSFMC_EINVAL, "NULL buffer");
    FisherPlan plan;
    if (const char* why = fisher_plan(1, K, 2 * kFisherMaxK + 1, n_pix < 0 ? 0 : (size_t)n_pix, &plan))
        return fail(PSFMC_EINVAL, "psfmc_debug_fisher_gram: %s (K=%d, n_pix=%d)", why, K, n_pix);
    HIP_TRY(hipSetDevice(device));
    const size_t vec = (size_t)K * n_pix;
    const size_t total = 2 * vec + 2 * (size_t)n_pix + plan.partial_doubles + plan.io_doubles;
    double* buf = nullptr;
    HIP_TRY(hipMalloc(&buf, total * sizeof(double)));
    double *d_a = buf, *d_b = d_a + vec, *d_c = d_b + vec, *d_d = d_c + n_pix, *d_part = d_d + n_pix;
    double *d_F = d_part + plan.partial_doubles + K, *d_g = d_F + (size_t)K * K;
    int rc = PSFMC_OK;
    auto step = [&](hipError_t e) { if (e != hipSuccess && rc == PSFMC_OK) rc = fail(PSFMC_EHIP, "psfmc_debug_fisher_gram: %s", hipGetErrorString(e)); };
    step(hipMemcpy(d_a, a, vec * sizeof(double), hipMemcpyHostToDevice));
    step(hipMemcpy(d_b, b, vec * sizeof(double), hipMemcpyHostToDevice));
    step(hipMemcpy(d_c, c, (size_t)n_pix * sizeof(double), hipMemcpyHostToDevice));
    step(hipMemcpy(d_d, d, (size_t)n_pix * sizeof(double), hipMemcpyHostToDevice));
    if (rc == PSFMC_OK) {
        launch_fisher_gram(FisherVectors{d_a, d_b, d_c, d_d}, 1, K, n_pix, plan, d_part, d_F, d_g, nullptr);
        step(hipGetLastError());
        step(hipMemcpy(F, d_F, (size_t)K * K * sizeof(double), hipMemcpyDeviceToHost));
        step(hipMemcpy(g, d_g, (size_t)K * sizeof(double), hipMemcpyDeviceToHost));
    }
    (void)hipFree(buf);
    return rc;
}

// ---------------------------------------------------------------------------
// diagnostic: device elementary functions on host arrays
// ---------------------------------------------------------------------------
__global__ void k_debug_math(int op, int n, const double* __restrict__ in, double* __restrict__ out) {
    __shared__ __align__(16) double tab[4][kLogTabBytes / sizeof(double)];   // one copy per wave, as in k_rows_fwd
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (op >= 100) {
        // op = 100: x^p through the rasteriser's power tables, p = in[n]; the tables are built in `out + n`
        // (kPowTab doubles of scratch behind the n results) by this wave, as k_pow_tables builds them
        __shared__ __align__(16) double ptab[4][kRasterLdsDoubles];
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const double p = in[n];
        double* g = out + n + (size_t)(blockIdx.x * 4 + wave) * kPowTab;
        build_pow_table(p, g, lane);
        __threadfence_block();
        wave_lds_sync();
        load_a_table(ptab[wave], lane);
        load_pow_table(ptab[wave], g, lane);
        wave_lds_sync();
        if (i < n) out[i] = fast_pow_tab(in[i], pow_poly(p), ptab[wave]);
        return;
    }
    load_log_table(tab[threadIdx.x >> 6], threadIdx.x & 63);
    wave_lds_sync();
    if (i >= n) return;
    const double x = in[i];
    out[i] = op == 0 ? fast_log2(x) : op == 1 ? fast_exp2(x) : op == 2 ? fast_rcp(x) : op == 3 ? fast_rcp1(x)
             : op == 4 ? fast_exp2_noclamp(x) : op == 5 ? fast_log2_tab(x, tab[threadIdx.x >> 6]) : fast_exp2_floor(x);
}

// ---------------------------------------------------------------------------
// Diagnostic: the plain memory sweeps the three kernels of a pass correspond to (no arithmetic),
// timed with HIP events -- what this GPU gives the data flow at best.  mode 0: every 16 bytes
// written once (k_rows_fwd), 1: read and written back in place (k_cols), 2: read once (k_rows_inv).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sweep(double2* __restrict__ buf, size_t n, int mode, double* __restrict__ sink) {
    const size_t stride = (size_t)gridDim.x * 1024;
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x; i + 768 < n; i += stride) {
        if (mode == 0) {
            const double2 v = {1.0, 2.0};
            buf[i] = v; buf[i + 256] = v; buf[i + 512] = v; buf[i + 768] = v;
        } else {
            double2 a = buf[i], b = buf[i + 256], c = buf[i + 512], d = buf[i + 768];
            if (mode == 1) {
                a.x += 1.0; b.x += 1.0; c.x += 1.0; d.x += 1.0;
                buf[i] = a; buf[i + 256] = b; buf[i + 512] = c; buf[i + 768] = d;
            } else {
                s += a.x + b.x + c.x + d.x;
            }
        }
    }
    if (s == 12345.678) sink[0] = s;            // keeps the loads of mode 2
}

extern "C" int psfmc_debug_sweep(int device, int mode, size_t nbytes, int reps, double* us_per_sweep) {
    if (mode < 0 || mode > 2 || nbytes < (1u << 20) || reps < 1 || !us_per_sweep) return fail(PSFMC_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(device));
    double2* buf = nullptr;
    double* sink = nullptr;
    HIP_TRY(hipMalloc(&buf, nbytes));
    int rc = PSFMC_OK;
    hipEvent_t a = nullptr, b = nullptr;
    if (hipMalloc(&sink, 64) != hipSuccess || hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
        rc = fail(PSFMC_ENOMEM, "hipMalloc / hipEventCreate");
    } else {
        (void)hipMemset(buf, 0, nbytes);
        const size_t n = nbytes / sizeof(double2);
        for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(k_sweep, dim3(2048), dim3(256), 0, 0, buf, n, mode, sink);
        (void)hipEventRecord(a, 0);
        for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_sweep, dim3(2048), dim3(256), 0, 0, buf, n, mode, sink);
        (void)hipEventRecord(b, 0);
        float ms = 0.f;
        if (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess)
            rc = fail(PSFMC_EHIP, "sweep failed: %s", hipGetErrorString(hipGetLastError()));
        *us_per_sweep = (double)ms * 1e3 / reps;
    }
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    if (sink) (void)hipFree(sink);
    (void)hipFree(buf);
    return rc;
}

// ---------------------------------------------------------------------------
// diagnostic: the rate at which THIS chip issues fp64 vector instructions when every SIMD is busy -- the
// other ceiling of the path besides the memory sweeps (psfmc_debug_sweep): with two and four Sersic components
// the 512^2 / 1024^2 passes carry more VALU time than sweep time.  64 v_fma_f64 per loop iteration (8 chains
// x 8, inline asm), `waves` waves per SIMD on every CU, timed with HIP events: nanoseconds per wave-instruction
// per SIMD.  (tools/clock_probe.hip is the stand-alone version with the in-kernel clock.)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_valu_rate(double* __restrict__ out, int iters) {
    double a[8];
    for (int i = 0; i < 8; ++i) a[i] = 1.0 + 1e-9 * (threadIdx.x + i);
    double m = 1.0000001, c = 1e-12;
    asm volatile("" : "+v"(m), "+v"(c));
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int rep = 0; rep < 8; ++rep)
#pragma unroll
            for (int i = 0; i < 8; ++i) asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(a[i]) : "v"(m), "v"(c));
    }
    double acc = 0.0;
    for (int i = 0; i < 8; ++i) acc += a[i];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

extern "C" int psfmc_debug_valu_rate(int device, int waves_per_simd, int iters, double* ns_per_instruction) {
    if (waves_per_simd < 1 || waves_per_simd > 8 || iters < 1 || !ns_per_instruction) return fail(PSFMC_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    const int blocks = prop.multiProcessorCount * waves_per_simd;        // 4 waves per block: one per SIMD
    double* out = nullptr;
    HIP_TRY(hipMalloc(&out, (size_t)blocks * 256 * sizeof(double)));
    int rc = PSFMC_OK;
    hipEvent_t a = nullptr, b = nullptr;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
        rc = fail(PSFMC_ENOMEM, "hipEventCreate");
    } else {
        hipLaunchKernelGGL(k_valu_rate, dim3(blocks), dim3(256), 0, 0, out, iters);          // warm-up (clocks settle)
        (void)hipEventRecord(a, 0);
        hipLaunchKernelGGL(k_valu_rate, dim3(blocks), dim3(256), 0, 0, out, iters);
        (void)hipEventRecord(b, 0);
        float ms = 0.f;
        if (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess)
            rc = fail(PSFMC_EHIP, "rate probe failed: %s", hipGetErrorString(hipGetLastError()));
        // every SIMD issued waves_per_simd x iters x 64 wave-instructions
        *ns_per_instruction = (double)ms * 1e6 / ((double)waves_per_simd * iters * 64.0);
    }
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    (void)hipFree(out);
    return rc;
}

// op 100: in[n] holds the exponent p of x^p through the rasteriser's power tables (in has n + 1 values)
extern "C" int psfmc_debug_math(int device, int op, int n, const double* in, double* out) {
    const bool pw = op == 100;
    if (n < 0 || op < 0 || (op > 6 && !pw) || (n > 0 && (!in || !out))) return fail(PSFMC_EINVAL, "bad argument");
    if (n == 0) return PSFMC_OK;
    HIP_TRY(hipSetDevice(device));
    double *d_in = nullptr, *d_out = nullptr;
    const int blocks = (n + 255) / 256;
    const size_t n_in = (size_t)n + (pw ? 1 : 0), n_out = (size_t)n + (pw ? (size_t)blocks * 4 * kPowTab : 0);
    HIP_TRY(hipMalloc(&d_in, n_in * sizeof(double)));
    int rc = PSFMC_OK;
    if (hipMalloc(&d_out, n_out * sizeof(double)) != hipSuccess) rc = fail(PSFMC_ENOMEM, "hipMalloc");
    if (rc == PSFMC_OK) {
        (void)hipMemcpy(d_in, in, n_in * sizeof(double), hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k_debug_math, dim3(blocks), dim3(256), 0, 0, op, n, d_in, d_out);
        if (hipMemcpy(out, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(PSFMC_EHIP, "debug_math copy failed: %s", hipGetErrorString(hipGetLastError()));
    }
    (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    return rc;
}

#endif  // PSFMC_PART == 0
