// vet_host.hpp — host-side state shared by the translation units of libvet_hip.so (not part of the C-ABI).
//
//   vet_context.hip     library / context / profiling / device-memory helpers, the test / development switches (parsed once)
//   vet_plan.hip        device tables of a plan: direction table, lattices, nearest-tile LUTs, alias and weight tables,
//                       error bounds; parity read-back hooks; angular distances; tile boundary geometry
//   vet_spatial.hip     launch logic of the spatial-entropy kernels (single videos and batches)
//   vet_transition.hip  launch logic of the transition-entropy kernels (single videos and batches)
//   vet_window.hip      the sliding-window spatial- and transition-entropy kernels (frame windows pooled) and their launch logic
//   vet_user.hip        the per-viewer spatial-entropy kernels (one histogram per user over time) and their launch logic
//   vet_user_divergence.hip
//                       the pairwise viewer divergence kernels (a U x U Jensen-Shannon matrix per row) and their launch logic
//   vet_window_divergence.hip
//                       the window-to-window divergence kernels (a lag band of Jensen-Shannon distances per row) and their launch logic
//   vet_coverage.hip    the attention coverage kernels (a window's tiles ranked in LDS, the top-k tile sets that hold given shares of
//                       its mass, and the share of later windows' mass they still hold) and their launch logic
//   vet_markov.hip      the windowed Markov transition statistics (a row's (source, destination) tile pairs sorted in LDS into integer
//                       pair counts; entropy rate, stationary and destination entropy, mutual information, stay share; the dense
//                       transition matrix) and their launch logic
//   vet_motion.hip      the head-motion statistics (one angle per (frame pair, viewer) from the direction table; per row the moments,
//                       exact order statistics — an LDS sort, or a radix selection over chunks — and an edge histogram of the
//                       angles) and their launch logic
//   vet_dispersion.hip  the audience dispersion (the angle between two viewers' directions in one frame over all pairs: per (frame,
//                       viewer) partials from unit vectors staged in LDS, then per row the block-ordered sums) and its launch logic
//   vet_cluster.hip     the viewer clusters (per row the LINKED pairs of viewers as bit words from a pair walk over the direction
//                       table, then the connected components by label propagation in LDS, their sizes, entropy and centroids) and
//                       their launch logic
//   vet_fixation.hip    the fixation and tile-dwell events (per viewer the maximal runs of frames whose consecutive directions stay within
//                       a cone, or on one tile: a segmented max-scan over the viewer's frames in order with a carry between chunks; the
//                       events per row, their histogram, labels, list and centroids) and their launch logic
//   vet_saliency.hip    the saliency maps (the spherical kernel density of a row's viewing directions on an equirectangular map: the
//                       row's distinct directions and multiplicities, the map from the list staged in LDS, the row statistics), the
//                       saliency similarity of two audiences (their maps by the same kernels, compared row by row), the viewer
//                       congruency, the saliency scoring of a predicted map (its rows sorted in LDS, sampled and ranked at the list
//                       entries' directions) and their launch logic
//   vet_crowd.hip       the viewer-to-crowd divergence kernels (each viewer's KL from the pooled row histogram) and their launch logic
//   vet_bootstrap.hip   the bootstrap kernels (viewers resampled with replacement: an FP64 MFMA contraction of resample counts with
//                       the per-viewer histograms, the entropy epilogue, the per-row summary) and their launch logic
//   vet_group.hip       the two-audience permutation test (labellings ranked in LDS, an FP64 MFMA contraction of 0/1 group masks with
//                       the per-viewer histograms, the Jensen-Shannon epilogue, the per-row summary) and its launch logic
//   vet_heatmap.hip     the heatmap kernels (pixel -> tile / cell maps, palettes, fill, markers) and their launch logic
//   vet_tiling.hip      the tiling kernels (arcs -> chords, splat, compose) and their launch logic
//   vet_hostapi.hip     host-buffer entry points (one staged-run helper for the entropy entries, one block-download pipeline
//                       for heatmaps and tilings), device-resident results, the heatmap and tiling handles (no kernels)
// Every kernel header is included by exactly one of them (the per-viewer units share the device helpers of vet_user_dirs.hpp, the windowed units those of vet_window_hist.hpp, both those of vet_row_hist.hpp).  There is no CPU compute path anywhere.
#pragma once
#include "../../include/vet.h"
#include "vet_layout.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace vh {

int fail(int code, const char* fmt, ...);      // records the thread's error message, returns code
const char* last_error();

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return vh::fail(VET_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                            __FILE__, __LINE__);                                                  \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t b) { return hipMalloc(&p, b ? b : 8); }
};

enum { KID_GRID = 0, KID_NEAREST = 1, KID_SPATIAL = 2, KID_TRANSITION = 3, KID_FINALIZE = 4, KID_WTAB = 5, KID_WEIGHTS = 6, KID_COUNT = 7 };

struct EventPair {
    int kid;
    hipEvent_t a, b;
};

// What the weights-only pass of the precise sweep needs of a plan (tile_weights VALUES at the reference's precision:
// exact FP64 weights summed in the reference's column order, calculate_tile_weights / compute_spatial_entropy,
// utilities/entropy_utils.py:108-144, 179-192).  The two device tables are shared with the plan, so a device-resident
// result (vet_result) that recomputes its weight rows on fetch may outlive the plan and its context.
struct WeightsCore {
    int device = 0;
    size_t lds_max = 64 * 1024;
    int n_cu = 256;
    std::shared_ptr<void> dir_unit;    // [n_dirs][3] f64 unit directions
    std::shared_ptr<void> tiles0;      // [n0][3] f64 unit tile centres of lattice 0
    int n0 = 0;
    int64_t n_dirs = 0;
    double cos_cull = 0.0, max_ang = 0.0, power = 2.0;
    // Exact weight rows of lattice 0 (k_wexact, built on the first request for weights): one ELL row per canonical
    // direction holding the tile and the exact FP64 weight of every tile with distance < fov/2 — zero-valued keys included.
    // The weights pass then gathers rows (k_weights_gather) instead of sweeping every tile with acos / pow per sample.
    struct Exact {
        int state = 0;                 // 0 not decided, 1 ready, -1 not usable (too large for the device, or no memory at the
                                       // first request): precise sweep instead.  Decided once (ensure_exact_weights, on the
                                       // plan's single thread) and never changed afterwards: results that share this core
                                       // read it from other threads
        int stride = 0, n_rows = 0;
        std::shared_ptr<void> alias;   // [n_dirs] u32  direction -> row | mirrored << 31
        std::shared_ptr<void> idx;     // [n_rows][stride] u16 tiles
        std::shared_ptr<void> w;       // [n_rows][stride] f64 weights
        std::shared_ptr<void> len;     // [n_rows] u32 entries in use
    } ex;
};

// One slot of the batch-descriptor ring (vet_ctx::stage)
struct BatchStage {
    void* h = nullptr;          // pinned host copy
    void* d = nullptr;          // device copy
    size_t cap = 0;
    hipEvent_t done = nullptr;  // recorded behind the last launch that reads d
    bool pending = false;
};
constexpr int kBatchStages = 4;

// Test and development switches.  The environment is read ONCE, in vet_create; nothing between a C-ABI entry point and
// its kernel launches calls getenv.  Each forces a path that real inputs can also reach, or (VET_LUT_TIMELINE) adds
// output to a development build: none changes a result.
struct Tuning {
    int no_fused = 0;           // VET_NO_FUSED: per-lattice tables instead of the fused one (test_fused_table_kernels_agree)
    int fused_single = 0;       // VET_FUSED: fused table also for one-lattice plans (test_fused_table_kernels_agree)
    int t_global = 0;           // VET_T_GLOBAL: transition through k_transition_any whatever the shape
                                // (test_transition_global_hash_variant_on_small_frames)
    std::string lut_timeline;   // VET_LUT_TIMELINE=path (make DEV=1 builds only): per-workgroup wall-clock timeline of the
                                // fused table kernel, read by tools/timeline_summary.py
    int no_exact_rows = 0;      // VET_NO_EXACT_ROWS: the weights pass never builds the exact weight rows (as if they did not fit
                                // the device): the precise sweep in weights-only mode serves — the fallback's test switch
                                // (include/vet.h; test_fp64_formulation.py, test_hip_shapes.py)
    int no_row_cap = 0;         // vet_test_no_row_cap (no environment variable): one-lattice tables keep cap = stride (every row whole, no side table) — the
                                // layout of plans where no cap qualifies; so a test can compare the two layouts (test_row_cap.py)
    int rec8 = 0;               // vet_test_rec8 (no environment variable): capped plans that have the compact record table launch the
                                // kernels of the 8-byte record all the same; read at every launch, so one plan runs both (test_rec32.py)
    int user_transition_hash = 0;   // vet_test_user_transition_hash (no environment variable): per-viewer transition rows of up to 64
                                // pairs run k_user_transition's hash shape instead of k_user_transition_wave; read at every
                                // launch, so one plan runs both (test_user_transition_gpu.py)
    int divergence_chunk_rows = 0;  // vet_test_divergence_chunk_rows (no environment variable): rows per histogram chunk of
                                // vet_user_divergence* (0 = sized by the workspace budget); read at every launch; the results do
                                // not depend on it (test_user_divergence_gpu.py)
    int window_divergence_chunk_rows = 0;   // vet_test_window_divergence_chunk_rows (no environment variable): pair rows per
                                // histogram chunk of vet_window_divergence* (0 = sized by the workspace budget); read at every
                                // launch; the results do not depend on it (test_window_divergence_gpu.py)
    int crowd_divergence_chunk_rows = 0;    // vet_test_crowd_divergence_chunk_rows (no environment variable): rows per chunk of
                                // vet_crowd_divergence* (0 = sized by the workspace budget); read at every launch; the results do
                                // not depend on it (test_crowd_divergence_gpu.py)
    int bootstrap_chunk_rows = 0;   // vet_test_bootstrap_chunk_rows (no environment variable): rows per histogram chunk of
                                // vet_bootstrap_entropy* (0 = sized by the workspace budget); read at every launch; the results do
                                // not depend on it (test_bootstrap_gpu.py)
    int group_chunk_rows = 0;       // vet_test_group_chunk_rows (no environment variable): rows per histogram chunk of
                                // vet_group_divergence* (0 = sized by the workspace budget); read at every launch; the results do
                                // not depend on it (test_group_divergence_gpu.py)
    int coverage_chunk_rows = 0;    // vet_test_coverage_chunk_rows (no environment variable): rows per histogram chunk of
                                // vet_coverage* (0 = sized by the workspace budget); read at every launch; the results do
                                // not depend on it (test_coverage_gpu.py)
    int markov_chunk_rows = 0;      // vet_test_markov_chunk_rows (no environment variable): rows per pass of the chunked shape of
                                // vet_transition_markov* (0 = sized by the workspace budget); read at every launch; the results do
                                // not depend on it (test_markov_gpu.py)
    int motion_lds_values = 0;      // vet_test_motion_lds_values (no environment variable): the most values of a row that one
                                // workgroup of vet_head_motion* takes (rounded down to a multiple of 1024, at least 1024; 0 = 16384);
                                // longer rows run the chunked shape; read at every launch; the results do not depend on it
                                // (test_head_motion_gpu.py)
    int dispersion_tile = 0;        // vet_test_dispersion_tile (no environment variable): the most viewers of a frame that
                                // k_dispersion_pairs stages in LDS at a time (0 = 1024); read at every launch; the results do not
                                // depend on it (test_dispersion_gpu.py)
    int saliency_tile = 0;          // vet_test_saliency_tile (no environment variable): the most list entries of a row that
                                // k_saliency_map, k_saliency_points and k_congruency_points stage in LDS at a time (0 = 1024); read at
                                // every launch; the results do not depend on it (test_saliency_gpu.py,
                                // test_saliency_similarity_gpu.py, test_congruency_gpu.py)
    int cluster_rows = 0;           // vet_test_cluster_tile (no environment variable): the most rows of a pass of vet_viewer_clusters*
                                // (0 = sized by the workspace budget) ...
    int cluster_tile = 0;           // ... and the most partners of one workgroup of k_cluster_links (0 = 128); read at every launch;
                                // the results do not depend on them (test_viewer_clusters_gpu.py)
    int fixation_chunk = 0;         // vet_test_fixation_chunk (no environment variable): the frames of one chunk of the walk of
                                // vet_fixations* (a multiple of 4, at most 1024; 0 = 1024); read at every launch; the results do not
                                // depend on it (test_fixations_gpu.py)
    void from_environment();
};

}  // namespace vh

struct vet_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int n_cu = 256;
    size_t lds_max = 64 * 1024;
    vh::Tuning tune;
    // grow-only workspace for per-lattice entropies + status words of the host variants
    void* ws = nullptr;
    size_t ws_bytes = 0;
    double* d_log2 = nullptr;      // log2(k), k = 0..4096
    bool attrs_set = false;        // dynamic-LDS limits of the run kernels raised (first plan)
    // grow-only device staging buffers (no hipMalloc per call): 0-6 host-buffer entry points (the SLOT_* names of
    // vet_hostapi.hip), 7 the still counts of vet_head_motion_host (batch descriptors live in the blob ring below), 8 transition scratch, 9 resolve list,
    // 10-11 the centroids and link words of vet_viewer_clusters_host (the events and centroids of vet_fixations_host), 12 the sweep counts of vet_viewer_clusters*
    void* pool[14] = {};
    size_t pool_cap[14] = {};
    // descriptor blobs of the batch entry points: a ring of (pinned host, device) buffer pairs, each guarded by an event
    // recorded behind the last launch that reads it (vh::BatchBlob) — the calls only enqueue work, so neither the host
    // copy nor the device copy of one batch may be reused while an earlier batch (possibly on another stream) is pending
    vh::BatchStage stage[vh::kBatchStages];
    int stage_next = 0;
    // profiling
    bool profiling = false;
    std::vector<vh::EventPair> pending;
    std::vector<hipEvent_t> free_events;
    double prof_ms[vh::KID_COUNT] = {};
    int64_t prof_n[vh::KID_COUNT] = {};
};

namespace vh {

struct Lattice {
    int n = 0;
    double* d_tiles = nullptr;     // [n][3] unit
    std::vector<double> h_unit;    // host copy of the unit tiles
    uint16_t* d_nearest = nullptr; // [n_dirs]
    double hmax = 0.0;
    // direction weight table (ELL), built on first use when the video has more samples than the
    // plan has directions
    uint32_t* d_tab_w = nullptr;   // [n_rows+1][stride] u32 mantissas (block floating point per row)
    uint16_t* d_tab_i = nullptr;   // [n_rows+1][stride]
    uint32_t* d_tab_meta = nullptr;// [n_rows+1] entries in use | row shift << 16
    uint8_t* d_row_s = nullptr;    // [n_dirs+1] row shift (k_row_stats)
    uint16_t* d_row_e = nullptr;   // [n_dirs+1] unclamped row exponent (FP table)
    bool fp_table = false;         // the table holds FP32 weights (plans whose integer bound is outside the contract)
    // k_row_stats: worst-case relative entropy error of integer histograms over every possible frame
    bool stats_done = false;
    double crit_tab = 0.0;         // table formulation (step 2^(e_row - 33) per entry)
    double crit_base = 0.0;        // times the step of the sweep formulation
    long ultra = 0;                // in-FoV (direction, tile) pairs whose weight is below 2^-1048 (k_row_stats): the
                                   // reference's NaN frames; such plans never use an integer formulation
    int markers = 0;               // marker entries of the FP table (k_wtab): frames they decide go to the precise sweep
    int last_form = -1;            // formulation of the last weighted call (parity / bench introspection)
    int stride = 0;                // 0 = not built, -1 = not usable (too large)
    // capped rows (vet_layout.hpp): stride == cap < the longest row; the longer rows' tails live in the side table
    bool capped = false;
    int n_ovf = 0;                 // rows with a block in the side table
    uint32_t* d_ovf_w = nullptr;   // [n_ovf+1][ROW_BLOCK] (the last row all zero)
    uint16_t* d_ovf_i = nullptr;   // [n_ovf+1][ROW_BLOCK]
    uint32_t* d_ovf_of_row = nullptr;  // [n_rows] block of the row in the side table, NO_OVERFLOW = none
    int gs_log2 = 4;               // lanes per gather group (log2); fixed when the table is built
    bool interleaved = false;      // well-filled row blocks are dealt by LDS bank class (k_wtab)
    bool binned = false;           // caller-supplied direction -> bin table (naive lat/lon tiling)
    int norm_n = 0;                // tile count used by the normaliser rule
    // exact FP64 weight rows of this lattice for the `dtable` formulation (k_wexact; lattices k > 0 only — lattice 0's are
    // the plan's WeightsCore::Exact, shared with device-resident results).  Rows use the plan's alias numbering (no alias
    // copy); decided once per plan like lattice 0's (ensure_exact_rows)
    WeightsCore::Exact ex;
};

}  // namespace vh

struct vet_plan {
    vet_ctx* ctx = nullptr;
    int W = 0, H = 0;
    bool grid = false;
    int64_t n_dirs = 0;
    double* d_dir_raw = nullptr;
    double* d_dir_unit = nullptr;
    std::vector<vh::Lattice> lat;
    double fov = 120.0, max_ang = 0.0, power = 2.0;
    int weighted = 1;
    double cos_cull = 0.0;
    int table_policy = 0;          // 0 by call size, 1 table whenever it is inside the contract, -1 never
    bool raw_weights = false;      // tile_weights = the formulation's own histogram (diagnostic) instead of the exact pass
    uint32_t* d_alias = nullptr;   // [n_dirs] direction id -> table row (dense) | mirrored << 31 (ensure_alias)
    bool mirror = false;           // rows are shared between mirror-image directions
    uint2* d_dirrec = nullptr;     // [n_dirs] alias | nearest tile | lattice-0 row meta (k_dirrec), dedup-capable plans
    uint32_t* d_dirrec32 = nullptr;// [n_dirs] the same in 4 bytes (k_dirrec32; vet_layout.hpp: REC32_*): capped tables whose rows
                                   // and tiles fit the fields; null otherwise — the capped kernels then read d_dirrec
    int n_rows = 0;                // table rows in use = canonical directions, densely numbered (ensure_alias)
    int* d_canon = nullptr;        // [n_rows] table row -> its direction
    // fused table: one row per distinct direction over ALL lattices (vet_layout.hpp)
    struct Fused {
        int state = 0;             // 0 not built, 1 ready, -1 not usable for this plan
        int R = 0, stride = 0, gs_log2 = 4;
        bool interleaved = false;
        vet::FusedLayout lay;
        uint32_t* d_meta = nullptr;// [R+1] entries in use | row shift << 16
        uint2* d_dirrec = nullptr; // [n_dirs] k_spatial_lut's per-direction record over the fused rows (k_dirrec)
        uint8_t* d_row_s = nullptr;// [R+1] fused row shifts
        uint32_t* d_w = nullptr;   // [R+1][stride]
        uint16_t* d_i = nullptr;   // [R+1][stride]
    } fused;
    std::shared_ptr<vh::WeightsCore> wcore;   // owner of d_dir_unit and lat[0].d_tiles (shared with device-resident results)
    bool stats_all = false;        // k_row_stats has run for every weighted lattice
    bool ultra = false;            // some lattice has ultra-tiny in-FoV weights: FP64 formulations only (plan-wide)
    bool fp64 = false;             // vet_plan_set_fp64: weighted Fibonacci lattices run `dtable` or `precise` only
    size_t exact_bytes = 0;        // device bytes of the exact weight rows of all lattices (one cap for the plan)
    uint32_t last_table_kernel = 0;// the k_spatial_lut instantiation and geometry of the last table launch (launch_lut,
                                   // launch_lut_fused; include/vet.h: VET_TK_*), 0 = none yet
};

namespace vh {

// the capped kernels of this plan read the 4-byte record (launches with the set of distinct rows; vet_test_rec8 forces the other)
inline bool use_rec32(const vet_plan* pl) {
    return pl->d_dirrec32 && !pl->ctx->tune.rec8 && !pl->lat.empty() && pl->lat[0].capped;
}

// hipEvent pair around the launches of a scope, on the launch stream (vet_profile_*)
struct ProfScope {
    vet_ctx* c;
    hipStream_t s;
    int kid;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(vet_ctx* c_, hipStream_t s_, int kid_) : c(c_), s(s_), kid(kid_) {
        if (!c->profiling) return;
        auto get = [&]() {
            hipEvent_t e = nullptr;
            if (!c->free_events.empty()) { e = c->free_events.back(); c->free_events.pop_back(); }
            else (void)hipEventCreate(&e);
            return e;
        };
        a = get(); b = get();
        (void)hipEventRecord(a, s);
    }
    ~ProfScope() {
        if (!a) return;
        (void)hipEventRecord(b, s);
        c->pending.push_back({kid, a, b});
    }
};

// The descriptor blob of ONE batch call: acquire() takes the ring's next slot (waiting only if the batch that used it
// kBatchStages calls ago has not finished), the caller fills host(), upload() enqueues the copy, the launches follow, and
// the destructor records the slot's event on the launch stream.
struct BatchBlob {
    vet_ctx* c = nullptr;
    BatchStage* st = nullptr;
    hipStream_t s = nullptr;
    size_t bytes = 0;
    bool uploaded = false;
    int acquire(vet_ctx* ctx, size_t nbytes);
    void* host() const { return st->h; }
    void* dev() const { return st->d; }
    int upload(hipStream_t stream);
    ~BatchBlob();
};

int ensure_ws(vet_ctx* c, size_t bytes);                          // grow-only workspace (c->ws)
// A workspace layout, described once: take<T>(count) places the next array — 16-byte padded, in the order of the calls — and
// returns its byte offset; `at` ends as the bytes to ask ensure_ws for.  (An array that starts behind another unit's share,
// WindowFrames::bytes, begins the layout there.)
inline size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }
struct WsLayout {
    size_t at = 0;
    template <class T> size_t take(size_t count) {
        const size_t off = at;
        at += pad16(count * sizeof(T));
        return off;
    }
};
int pooled(vet_ctx* c, int slot, size_t bytes, void** out);       // slot-indexed grow-only device buffer
int grid_for(long work, int block, int n_cu);
int check_run_args(const vet_plan* pl, int U, int T, const void* out);
// What the extern "C" device entries of the row calls check after their own arguments, and the stream they launch on (the
// caller's, or the context's).  ids_entry != null: the (d_mu, d_mv) entry — the plan needs a pixel grid ("...; use <ids_entry>")
// and both arrays; null: the _ids entry — d_ids.
int entry_samples(const vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, const char* ids_entry,
                  void* stream, hipStream_t* s);

constexpr size_t kMaxTableBytes = (size_t)24 << 30;   // per lattice; HBM is 288 GB
constexpr double kContractMargin = 1e-7;              // bound on |dH|/H an integer formulation may have (contract: 1e-6)
constexpr size_t kWholeLds = 160 * 1024 - 512;        // a single workgroup per CU may take the whole LDS

// vet_plan.hip: tables built on first use (each synchronises once)
int ensure_alias(vet_plan* pl);
int ensure_all_stats(vet_plan* pl, hipStream_t s);
int ensure_wtab(vet_plan* pl, int k, hipStream_t s);
int ensure_fused(vet_plan* pl, hipStream_t s);
bool any_binned(const vet_plan* pl);

// vet_spatial.hip: tile_weights of lattice 0 for frames [0, T) of a sample array given as direction ids, by the precise
// sweep in weights-only mode (users in column order); prof = context to attribute the launch to, or null
int weights_pass_ids(const WeightsCore& w, const int32_t* d_ids, int U, int T, double* d_weights, hipStream_t s, vet_ctx* prof);
// vet_plan.hip: the exact weight rows of lattice 0 (first use; synchronises once).  Leaves ex.state = -1 when they do not fit.
int ensure_exact_weights(vet_plan* pl, hipStream_t s);
// the same for lattice k (k = 0: ensure_exact_weights); exact_rows(pl, k) = its tables
int ensure_exact_rows(vet_plan* pl, int k, hipStream_t s);
const WeightsCore::Exact& exact_rows(const vet_plan* pl, int k);
vet::ExactRows exact_rows_arg(const vet_plan* pl, int k);         // ... as the kernels take them (the rows must exist)
// which instance of a kernel templated on S walks rows of this stride: S = 64-entry chunks of the longest row, 1, 2, 4, or 0 for
// any number (add_exact_rows); VET_KERNEL_BY_S(k, S) names the instance
inline int row_chunk_class(int stride) {
    const int chunks = stride / vet::WAVE;
    return chunks <= 1 ? 1 : chunks <= 2 ? 2 : chunks <= 4 ? 4 : 0;
}
#define VET_KERNEL_BY_S(kernel, S)                                                                                       \
    ((S) == 1 ? (const void*)kernel<1> : (S) == 2 ? (const void*)kernel<2> : (S) == 4 ? (const void*)kernel<4> : (const void*)kernel<0>)
// vet_spatial.hip: per-frame tile sums of weighted lattice k from its exact rows (which must exist), [T][n_k] in the dense
// tile_weights encoding, `dtable`'s bits — stage 1 of the windowed entry points (samples as d_mu / d_mv, or d_ids)
int exact_frame_rows(vet_plan* pl, int k, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, double* out,
                     hipStream_t s);
// (mu, mv) -> direction ids [n] (-1 absent or out of range) on the plan's pixel grid
int sample_ids(const vet_plan* pl, const double* d_mu, const double* d_mv, long n, int32_t* d_out, hipStream_t s);

// vet_heatmap.hip: per-frame tile-attention heatmaps.  heatmap_map: W x H pixel -> nearest tile of the n unit centres
// d_unit_tiles (k_heatmap_map).  heatmap_render: frames [0, T) -> d_rgb [T][H][W][3] (k_heatmap_palette into d_pal
// [T][n], k_heatmap_fill, then k_heatmap_markers when d_mu / d_mv are given), enqueued on s.  Wt = double (tile_weights
// [T][n]) or int32_t (a transition result's source-tile counts [T][n]); both are instantiated in vet_heatmap.hip.
struct HeatmapGeom {
    const uint16_t* d_map = nullptr;   // [H][W] tile index
    int n = 0, W = 0, H = 0;           // lattice size, frame size
    int VW = 0, VH = 0, radius = 0;    // video size of the samples (marker quantiser), marker half-width
};
int heatmap_map(vet_ctx* c, const double* d_unit_tiles, int n, int W, int H, uint16_t* d_map, hipStream_t s);
template <typename Wt>
int heatmap_render(vet_ctx* c, const HeatmapGeom& g, const Wt* d_weights, const int32_t* d_present, const double* d_mu,
                   const double* d_mv, int U, int T, uint32_t* d_pal, uint8_t* d_rgb, hipStream_t s);
// Lat/lon cells of a naive tiling (n_lat cells per lon column).  heatmap_map_latlon: W x H pixel -> the slot lj * n_lon + li
// of its cell li * n_lat + lj (k_heatmap_map_latlon).  heatmap_render_binned: frames [0, T) of the samples d_mu / d_mv
// [T][U] -> d_rgb: k_heatmap_bin_palette (the cell counts of each frame through the plan's LUT d_lut, straight into the
// slot-ordered d_pal [T][n]), k_heatmap_fill, then k_heatmap_markers when `markers`.
// heatmap_bin_layout: the LDS histogram of U users over n cells (ok = false: it does not fit, VET_ERR_UNSUPPORTED).
struct BinLayout {
    bool ok = false, pack = false;     // pack: two 16-bit counts per LDS word (U <= 65535)
    int words = 0, FPW = 0;            // LDS words per frame, frames per workgroup
    size_t lds = 0;                    // dynamic LDS bytes of a workgroup
};
BinLayout heatmap_bin_layout(int n, int U);
int heatmap_map_latlon(vet_ctx* c, int tile_width, int tile_height, int W, int H, uint16_t* d_map, hipStream_t s);
int heatmap_bin_chunk(int n);
int heatmap_render_binned(vet_ctx* c, const HeatmapGeom& g, int n_lat, const uint16_t* d_lut, const double* d_mu,
                          const double* d_mv, int U, int T, bool markers, uint32_t* d_pal, uint8_t* d_rgb, hipStream_t s);

// vet_tiling.hip: tilings drawn on the unit sphere.  tiling_chords: arcs [n][2][3] -> 50 slerp points per arc
// (k_tiling_chords).  tiling_render: frames [0, T) -> d_rgb [T][H][W][3]: clear d_flags [T][H][W], k_tiling_splat,
// k_tiling_compose, enqueued on s.  The cameras are computed on the host (vet_hostapi.hip).
struct TilingCam {
    double F[3], r[3], u[3], nd[3];    // focal point; right, up and -view direction (unit vectors)
    double s;                          // world size of a pixel
    double X0, Y0;                     // image position of the origin (the sphere's centre)
};
struct TilingGeom {
    const double* d_pts = nullptr;     // [n_arcs][50][3] slerp points (NaN: the arc draws nothing)
    const double* d_centres = nullptr; // [n_centres][3]
    long n_arcs = 0, n_centres = 0;
    int W = 0, H = 0;
    uint32_t colour[6] = {};           // packed RGB: background, red, black, then each blended with the sphere
};
int tiling_chords(vet_ctx* c, const double* d_arcs, long n_arcs, double* d_pts, hipStream_t s);
int tiling_render(vet_ctx* c, const TilingGeom& g, const TilingCam* d_cam, int T, uint32_t* d_flags, uint8_t* d_rgb,
                  hipStream_t s);

// dynamic-LDS limits of the run kernels (once per context, from vet_plan_create)
int spatial_set_attrs(vet_ctx* c);
int transition_set_attrs(vet_ctx* c);
int window_set_attrs(vet_ctx* c);
int user_set_attrs(vet_ctx* c);
int user_transition_set_attrs(vet_ctx* c);
int user_divergence_set_attrs(vet_ctx* c);
int window_divergence_set_attrs(vet_ctx* c);
int crowd_set_attrs(vet_ctx* c);
int bootstrap_set_attrs(vet_ctx* c);
int group_set_attrs(vet_ctx* c);
int markov_set_attrs(vet_ctx* c);
int motion_set_attrs(vet_ctx* c);
int dispersion_set_attrs(vet_ctx* c);
int saliency_set_attrs(vet_ctx* c);
int cluster_set_attrs(vet_ctx* c);

// vet_window.hip, shared with vet_window_divergence.hip: what the windowed spatial calls refuse about their arguments, and their
// stage 1.  window_frames_layout places, behind head_bytes of the caller's own, present[T] and per lattice the per-frame array
// (weighted: [T][n_k] f64 tile sums in the dense tile_weights encoding; counting: [T][U] i32 tiles) in the context's workspace,
// refuses plans that cannot run windowed and builds the exact weight rows on first use; the caller calls ensure_ws(wf.bytes or
// more) and then window_frames_run, which fills them (k_window_tiles, k_weights_gather) and raises d_status[0].
struct WindowFrames {
    size_t present_off = 0, off[64] = {}, bytes = 0;
};
int check_window_args(const vet_plan* pl, int U, int T, int window, int stride, const void* out);
int window_frames_layout(vet_plan* pl, int U, int T, size_t head_bytes, WindowFrames& wf, hipStream_t s);
int window_frames_run(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T,
                      const WindowFrames& wf, int32_t* d_status, hipStream_t s);

// vet_window_divergence.hip, shared with vet_crowd.hip and vet_coverage.hip: lattice k's pooled row histograms of rows [h0, h_end) from
// window_frames_run's arrays (k_window_hist_w/_c) — hist [h_end - h0][n_k] f64 (+0.0 = no key), tot and flag per row (1: no sample,
// or the row's own S is NaN); rows >= r_new also write samples[r] and add to status[1] where those are given.  Charged to k_finalize.
int window_hist_run(vet_plan* pl, int k, int U, const WindowFrames& wf, int window, int stride, long h0, long h_end, long r_new,
                    double* hist, double* tot, int32_t* flag, int32_t* samples, int32_t* status, hipStream_t s);

// vet_user.hip, shared with vet_user_divergence.hip and vet_crowd.hip (which build the same per-viewer histograms): lattice k counts integers
// (unweighted / binned); waves per row of the weighted histogram kernel (a function of the window and the plan alone); what
// the per-viewer spatial calls refuse about the plan (VET_ERR_UNSUPPORTED; builds the exact weight rows on first use) — their
// arguments are the windowed calls' (check_window_args)
bool counts_lattice(const vet_plan* pl, int k);
int user_nw(size_t lds_max, int n, int window);
int check_user_plan(vet_plan* pl, const char* what, hipStream_t s);
// stage 1 of every per-viewer call: k_user_dirs<d_ids given> over the samples -> dirs [U][T], raising d_status[0]; charged to
// k_spatial.  One grid row per 64 frames: check_user_dirs_frames refuses (VET_ERR_UNSUPPORTED, "<what>: ...") what the grid
// cannot hold — user_dirs_run calls it, and so does a call that must refuse before anything is staged or allocated
int check_user_dirs_frames(int T, const char* what);
int user_dirs_run(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int32_t* dirs,
                  int32_t* d_status, const char* what, hipStream_t s);

// vet_user_divergence.hip, shared with vet_bootstrap.hip: lattice k's per-viewer row histograms of rows [r0, r0 + cr) from dirs
// (k_user_hist_w/_c) — hist [cr][U][n_k] f64 (+0.0 = no key, or a key whose value is 0.0), tot and flag per (row, viewer) (1: no
// sample, or the viewer's own S is NaN); samples [U][R] and status[1] where those are given.  Charged as vet_user_entropy's stage 2.
int user_hist_run(vet_plan* pl, int k, const int32_t* dirs, int U, int T, int window, int stride, long R, long r0, long cr,
                  double* hist, double* tot, int32_t* flag, int32_t* samples, int32_t* status, hipStream_t s);

// vet_bootstrap.hip: what vet_bootstrap_entropy* refuse about their own arguments (VET_ERR_INVALID / VET_ERR_UNSUPPORTED), before
// anything is staged, allocated or launched — after check_window_args
int check_bootstrap_args(const vet_plan* pl, int U, int replicates, double confidence);

// vet_bootstrap.hip, shared with vet_group.hip: k_bootstrap_zero_keys on the chunk of a weighted lattice k behind user_hist_run — for
// the flagged (row, viewer) slots the tiles that are keys of the viewer with the value 0.0, zmask [cr][U][ceil(n_k / 32)] and
// zflag [cr][U].  Charged to k_finalize.
int zero_keys_run(vet_plan* pl, int k, const int32_t* dirs, int U, int T, int window, int stride, long r0, long cr, const double* hist,
                  const int32_t* flag, uint32_t* zmask, int32_t* zflag, hipStream_t s);

// vet_group.hip: what vet_group_divergence* refuse about their own arguments (VET_ERR_INVALID / VET_ERR_UNSUPPORTED), before
// anything is staged, allocated or launched — after check_window_args.  groups is host memory [U].
int check_group_args(const vet_plan* pl, int U, const int8_t* groups, int permutations, double confidence);

// vet_window.hip, for vet_markov.hip: stage 1 of the windowed transition call for lattice k alone — one launch of k_window_tiles over
// frames [0, T): tiles [T][U] i32 (-1 absent), d_status[0] raised where given.  Charged to k_spatial.
int window_tiles_lattice(vet_plan* pl, int k, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int32_t* tiles,
                         int32_t* d_status, hipStream_t s);

// vet_markov.hip: what vet_transition_markov* refuse about their arguments (VET_ERR_INVALID / VET_ERR_UNSUPPORTED), before anything is
// staged, allocated or launched
int check_markov_args(const vet_plan* pl, int U, int T, int window, int stride, int lag, const void* stats, const void* matrix);

// vet_motion.hip: what vet_head_motion* refuse about their arguments (VET_ERR_INVALID / VET_ERR_UNSUPPORTED), before anything is
// staged, allocated or launched.  fractions [Q] and edges [B + 1] are host memory.
int check_motion_args(const vet_plan* pl, int U, int T, int window, int stride, int lag, int per_user, const double* fractions, int Q,
                      const double* edges, int B, const void* stats);

// vet_dispersion.hip: what vet_dispersion* refuse about their arguments (VET_ERR_INVALID / VET_ERR_UNSUPPORTED), before anything is
// staged, allocated or launched.  edges [B + 1] is host memory.
int check_dispersion_args(const vet_plan* pl, int U, int T, int window, int stride, int per_user, const double* edges, int B);

// vet_cluster.hip: what vet_viewer_clusters* refuse about their arguments (VET_ERR_INVALID / VET_ERR_UNSUPPORTED), before anything is
// staged, allocated or launched.  fractions [Q] is host memory.
int check_cluster_args(const vet_plan* pl, int U, int T, int window, int stride, double cos_threshold, double min_share,
                       const double* fractions, int Q);

// vet_fixation.hip: what vet_fixations* refuse about their arguments (VET_ERR_INVALID / VET_ERR_UNSUPPORTED), before anything is
// staged, allocated or launched.  edges [B + 1] is host memory; events and centroids are the outputs of those names (or NULL).
int check_fixation_args(const vet_plan* pl, int U, int T, int window, int stride, int mode, double cos_threshold, int min_frames,
                        const int32_t* edges, int B, int64_t max_events, const void* events, const void* centroids);

// vet_saliency.hip: what vet_saliency* refuse about their arguments (VET_ERR_INVALID / VET_ERR_UNSUPPORTED), before anything is
// staged, allocated or launched.
int check_saliency_args(const vet_plan* pl, int U, int T, int window, int stride, int per_user, double sigma, int W, int H, int scale);
// ... and what vet_saliency_similarity* refuse: the above for the pooled layout, groups NULL (host memory [U]), an audience without a
// viewer.
int check_similarity_args(const vet_plan* pl, int U, int T, int window, int stride, const int8_t* groups, double sigma, int W, int H);
// ... and what vet_congruency* refuse: check_saliency_args' sigma, window and stride for both layouts, fewer than two viewers.
int check_congruency_args(const vet_plan* pl, int U, int T, int window, int stride, double sigma);
// ... and what vet_saliency_score* refuse: check_saliency_args for the pooled layout, pred NULL, n_pred other than 1 or the rows.
int check_score_args(const vet_plan* pl, int U, int T, int window, int stride, double sigma, int W, int H, const double* pred,
                     int n_pred);

// vet_coverage.hip: what vet_coverage* refuse about their own arguments (VET_ERR_INVALID / VET_ERR_UNSUPPORTED), before anything is
// staged, allocated or launched — after check_window_args.  R = the rows of the call; fractions is host memory [Q].
int check_coverage_args(const vet_plan* pl, long R, int max_lag, const double* fractions, int Q, const void* hit);

// vet_user_transition.hip: what vet_user_transition_entropy* refuse (VET_ERR_INVALID / VET_ERR_UNSUPPORTED), before anything is
// staged, allocated or launched
int check_user_transition_args(const vet_plan* pl, int U, int T, int window, int stride, const void* out);

}  // namespace vh
