// vet_hostapi.hip — host-buffer entry points of the C-ABI (include/vet.h).  Two file-local helpers carry them: StagedRun
// (the entropy entries: samples and status words through the context's grow-only device buffers, the device-pointer entry
// points in between, synchronous; staged_rows is the whole run of the thirteen row calls) and BlockDownload (heatmaps and
// tilings: frames rendered in blocks, the download of one block overlapping the render of the next).  Also here:
// device-resident results (vet_result), heatmaps (vet_heatmap: the map, the palette and the uploads of a block; the kernels
// are vet_heatmap.hip's) and tilings (vet_tiling: the cameras; the kernels are vet_tiling.hip's).  File-local types and
// templates come first, then the one extern "C" block.  No kernels of its own and no CPU compute path.
#include "vet_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

using namespace vh;

// vet_ctx::pool slots of the entropy host entries (8 and 9 belong to vet_transition.hip and vet_spatial.hip, vet_host.hpp):
// the samples (h_mu or h_ids, h_mv), the entropies, output 0 (assignments / pairs), output 1 (weights / source counts), the
// count per row (present / common / samples) and the two status words
enum { SLOT_MU = 0, SLOT_IDS = 0, SLOT_MV = 1, SLOT_ENTROPY = 2, SLOT_OUT0 = 3, SLOT_OUT1 = 4, SLOT_COUNT = 5, SLOT_STATUS = 6,
       SLOT_STILL = 7 };    // 7: the second count per row of vet_head_motion_host; the predicted maps of vet_saliency_score_host
#define POOL(slot, bytes, var) do { int rc_ = pooled(c, slot, bytes, (void**)&var); if (rc_) return rc_; } while (0)

struct vet_result {
    int device = 0;                      // the result may outlive its context: only the device id is kept
    bool transition = false;
    void* d[2] = {nullptr, nullptr};     // 0: assign / pairs, 1: weights / srccount (null when the weights are lazy)
    size_t row_bytes[2] = {0, 0};
    int64_t rows = 0;
    // Weighted spatial results whose direction ids [T][U] i32 are not larger than the weight rows [T][n_0] f64 do not store
    // tile_weights: they keep the ids and the plan's shared tables, and a fetched block of weight rows is computed by the
    // weights pass (k_weights_gather over the exact FP64 rows of lattice 0; the precise sweep in weights-only mode where
    // those do not fit) — the reference's values whatever formulation produced the entropy, and no 120 MB weights pass on
    // the hot path of BASELINE config 3 (1024 users, 501 tiles: the two footprints are equal).  Audiences with
    // U * 4 > n_0 * 8 (9000 users on 51 tiles: ids would be 88 x the weights) store the weight rows instead.
    // The weights path (exact rows or precise sweep) was decided once for the plan before the result was created
    // (ensure_exact_weights never revisits it), and `core` is immutable from then on: eager == fetched, same bits.
    bool lazy_weights = false;
    std::shared_ptr<WeightsCore> core;
    int32_t* d_ids = nullptr;
    int U = 0;
    void* d_tmp = nullptr;               // grow-only staging of the fetched weight rows
    size_t tmp_cap = 0;
    std::mutex fetch_mu;                 // d_tmp is one buffer: concurrent fetches of one result take turns
};

namespace {         // file-local types: nothing here is exported

// A handle while it is being built: destroyed by its own C-ABI function unless release()d into the caller's *out
template <typename T, int (*Destroy)(T*)>
struct HandleDeleter { void operator()(T* p) const { (void)Destroy(p); } };
using ResultPtr = std::unique_ptr<vet_result, HandleDeleter<vet_result, vet_result_free>>;
using HeatmapPtr = std::unique_ptr<vet_heatmap, HandleDeleter<vet_heatmap, vet_heatmap_destroy>>;
using TilingPtr = std::unique_ptr<vet_tiling, HandleDeleter<vet_tiling, vet_tiling_destroy>>;

// Grows a lazy result's staging buffer to n weight rows (the caller holds fetch_mu).
static int result_tmp_rows(vet_result* r, int64_t n) {
    const size_t bytes = (size_t)n * r->row_bytes[1];
    if (r->tmp_cap >= bytes) return VET_OK;
    if (r->d_tmp) { HIP_TRY(hipFree(r->d_tmp)); r->d_tmp = nullptr; r->tmp_cap = 0; }
    HIP_TRY(hipMalloc(&r->d_tmp, bytes));
    r->tmp_cap = bytes;
    return VET_OK;
}

// The arguments of the single-video entries; the samples are (h_mu, h_mv) on the plan's pixel grid, or h_ids.
static int check_host_args(const vet_plan* pl, int U, int T, const double* h_entropy, const double* h_mu, const double* h_mv,
                           const int32_t* h_ids) {
    int rc = check_run_args(pl, U, T, h_entropy);
    if (rc) return rc;
    if (!h_ids && (!h_mu || !h_mv)) return fail(VET_ERR_INVALID, "need h_mu and h_mv, or h_ids");
    if (!h_ids && !pl->grid) return fail(VET_ERR_INVALID, "plan has no pixel grid; pass h_ids");
    return VET_OK;
}

// The prologue of the row-call host entries, before anything is staged: check_host_args, then the rows of the call, *R =
// vet_window_rows over the frames (pairs: over the n_frames - 1 frame pairs), refused where the window does not fit.
static int check_row_args(const vet_plan* pl, int U, int T, int window, int stride, bool pairs, const double* h_out,
                          const double* h_mu, const double* h_mv, const int32_t* h_ids, int64_t* R) {
    int rc = check_host_args(pl, U, T, h_out, h_mu, h_mv, h_ids);
    if (rc) return rc;
    *R = vet_window_rows(pairs ? T - 1 : T, window, stride);
    if (*R < 0)
        return fail(VET_ERR_INVALID, "need 1 <= window <= %s and stride >= 1 (got window %d, stride %d, %d frames)",
                    pairs ? "n_frames - 1" : "n_frames", window, stride, T);
    return VET_OK;
}

// The message of VET_ERR_EMPTY for the per-frame entries (one %d: the rows without a sample).
static const char* empty_rows_message(bool transition) {
    return transition ? "%d frame pair(s) without a user present in both frames"
                      : "%d frame(s) without any user (Empty vector dictionary)";
}

// One synchronous run of an entropy host entry on the context's stream.  begin() stages the S samples (h_ids when given,
// else h_mu / h_mv); the entry then takes its output slots, clear_status()es, launches (drain() on a launch error) and
// enqueues its downloads; finish() reads the status words back and synchronises (sync), then decodes them (decode).
struct StagedRun {
    vet_ctx* c = nullptr;
    hipStream_t s = nullptr;
    double *mu = nullptr, *mv = nullptr;
    int32_t *ids = nullptr, *status = nullptr;
    int32_t h_status[2] = {0, 0};

    int begin(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, size_t S) {
        c = pl->ctx;
        HIP_TRY(hipSetDevice(c->device));
        s = c->stream;
        if (h_ids) {
            POOL(SLOT_IDS, S * 4, ids);
            HIP_TRY(hipMemcpyAsync(ids, h_ids, S * 4, hipMemcpyHostToDevice, s));
        } else {
            POOL(SLOT_MU, S * 8, mu);
            POOL(SLOT_MV, S * 8, mv);
            HIP_TRY(hipMemcpyAsync(mu, h_mu, S * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(mv, h_mv, S * 8, hipMemcpyHostToDevice, s));
        }
        return VET_OK;
    }
    int clear_status() {                 // the last thing enqueued before the launches
        POOL(SLOT_STATUS, 8, status);
        HIP_TRY(hipMemsetAsync(status, 0, 8, s));
        return VET_OK;
    }
    int drain(int rc) { (void)hipStreamSynchronize(s); return rc; }
    int sync(bool read_status) {
        if (read_status) HIP_TRY(hipMemcpyAsync(h_status, status, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return VET_OK;
    }
    // empty_msg: the entry's message for rows without a sample, with one %d for their number
    int decode(const char* empty_msg) const {
        if (h_status[0]) return fail(VET_ERR_RANGE, "Normalized coordinates must be between 0 and 1");
        if (h_status[1]) return fail(VET_ERR_EMPTY, empty_msg, h_status[1]);
        return VET_OK;
    }
    int finish(const char* empty_msg) {
        int rc = sync(true);
        return rc ? rc : decode(empty_msg);
    }
    // the tail of the calls whose rows without a sample are data (NaN, samples 0): only VET_ERR_RANGE is decoded
    int finish_rows_are_data() {
        int rc = sync(true);
        if (rc) return rc;
        h_status[1] = 0;
        return decode("");
    }
};

// The fourteen row-call host entries (windowed / per-viewer spatial entropy, viewer / crowd / window divergence, coverage, windowed /
// per-viewer transition entropy, the Markov transition statistics, the head-motion statistics, the audience dispersion, the saliency
// maps, the saliency similarity, the viewer congruency; and the saliency scoring, the viewer clusters and the fixation events, a fifteenth to a seventeenth) after their
// refusals: one staged run.  outs = the primary output, the optional one (kNoOut where the call has none) and the count per row; a
// null h = not wanted: no slot is taken, the launch gets nullptr and nothing is downloaded — except the count, whose slot the device
// entries always write.  (vet_coverage_host has two primary outputs: four entries, each on a slot of its own.)  launch(run, d) enqueues
// the call on the staged samples and the device outputs d[]; empty_msg as StagedRun::decode, or kRowsAreData (finish_rows_are_data).
struct RowOut { void* h; size_t bytes; int slot; };
constexpr RowOut kNoOut = {nullptr, 0, SLOT_OUT1};
constexpr const char* kRowsAreData = nullptr;

// the _ids entry on the staged ids, else the (mu, mv) entry: both take the same arguments after the samples
template <typename IdsEntry, typename GridEntry, typename... Args>
static int launch_rows(const StagedRun& run, IdsEntry ids_entry, GridEntry grid_entry, vet_plan* pl, Args... args) {
    return run.ids ? ids_entry(pl, run.ids, args...) : grid_entry(pl, run.mu, run.mv, args...);
}

template <size_t N, typename Launch>
static int staged_rows(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T,
                       const RowOut (&outs)[N], const char* empty_msg, Launch launch) {
    StagedRun run;
    int rc = run.begin(pl, h_mu, h_mv, h_ids, (size_t)U * T);
    if (rc) return rc;
    vet_ctx* c = run.c;
    void* d[N] = {};
    for (size_t i = 0; i < N; ++i)
        if (outs[i].h || outs[i].slot == SLOT_COUNT) POOL(outs[i].slot, outs[i].bytes, d[i]);
    rc = run.clear_status();
    if (rc) return rc;
    rc = launch(run, d);
    if (rc) return run.drain(rc);
    for (size_t i = 0; i < N; ++i)
        if (outs[i].h) HIP_TRY(hipMemcpyAsync(outs[i].h, d[i], outs[i].bytes, hipMemcpyDeviceToHost, run.s));
    return empty_msg ? run.finish(empty_msg) : run.finish_rows_are_data();
}

// Frames rendered on the device in blocks and brought to the caller's host array, the download of one block overlapping
// the render of the next: two device blocks the render stream fills in turn, two pinned blocks a second, non-blocking
// stream copies them into, and the host's memcpy of block k - 1 out of its pinned block while block k runs.  The render
// stream never waits for a download except to reuse a device block (block k waits for the copy of block k - 2).
struct BlockDownload {
    bool in_stream = false;              // the owner's choice, before the first run: no second stream, the downloads follow
                                         // their renders on the render stream (vet_tiling_create says when)
    hipStream_t copy = nullptr;
    hipEvent_t computed[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
    uint8_t* d_blk[2] = {nullptr, nullptr};
    uint8_t* h_pin[2] = {nullptr, nullptr};
    size_t cap = 0;                      // bytes of each of the four blocks

    void free_blocks() {
        for (int i = 0; i < 2; ++i) {
            if (d_blk[i]) (void)hipFree(d_blk[i]);
            if (h_pin[i]) (void)hipHostFree(h_pin[i]);
            d_blk[i] = nullptr; h_pin[i] = nullptr;
        }
        cap = 0;
    }

    // grow-only; s = the render stream
    int ensure(hipStream_t s, size_t bytes) {
        if (cap >= bytes) return VET_OK;
        HIP_TRY(hipStreamSynchronize(s));                  // a pending render or download may still use the old blocks
        if (copy) HIP_TRY(hipStreamSynchronize(copy));
        free_blocks();
        if (!in_stream && !copy) HIP_TRY(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            if (!computed[i]) HIP_TRY(hipEventCreateWithFlags(&computed[i], hipEventDisableTiming));
            if (!copied[i]) HIP_TRY(hipEventCreateWithFlags(&copied[i], hipEventDisableTiming));
            HIP_TRY(hipMalloc((void**)&d_blk[i], bytes));
            HIP_TRY(hipHostMalloc((void**)&h_pin[i], bytes, hipHostMallocDefault));
        }
        cap = bytes;
        return VET_OK;
    }

    // `total` bytes to h_dst in blocks of `block` bytes (the last one may be shorter): render(k, d_dst) enqueues block k
    // on s into d_dst and returns a VET_* code.  Synchronous; both streams are drained on any error.
    template <typename Render>
    int run(hipStream_t s, size_t total, size_t block, uint8_t* h_dst, Render render) {
        int rc = ensure(s, block);
        if (rc) return rc;
        hipStream_t cs = in_stream ? s : copy;
        auto drain = [&](int code) {
            (void)hipStreamSynchronize(s);
            if (cs != s) (void)hipStreamSynchronize(cs);
            return code;
        };
        const int64_t nb = (int64_t)((total + block - 1) / block);
        auto bytes_of = [&](int64_t k) { return std::min(block, total - (size_t)k * block); };
        for (int64_t k = 0; k <= nb; ++k) {
            const int st = (int)(k & 1), ps = st ^ 1;
            if (k < nb) {
                if (k >= 2 && hipStreamWaitEvent(s, copied[st], 0) != hipSuccess)     // the copy of block k-2 has left d_blk[st]
                    return drain(fail(VET_ERR_DEVICE, "hipStreamWaitEvent failed"));
                rc = render(k, d_blk[st]);
                if (rc) return drain(rc);
                if ((cs != s && (hipEventRecord(computed[st], s) != hipSuccess ||
                                 hipStreamWaitEvent(cs, computed[st], 0) != hipSuccess)) ||
                    hipMemcpyAsync(h_pin[st], d_blk[st], bytes_of(k), hipMemcpyDeviceToHost, cs) != hipSuccess ||
                    hipEventRecord(copied[st], cs) != hipSuccess)
                    return drain(fail(VET_ERR_DEVICE, "download of block %lld failed", (long long)k));
            }
            if (k >= 1) {                                       // block k-1 to the caller while block k (if any) runs
                if (hipEventSynchronize(copied[ps]) != hipSuccess) return drain(fail(VET_ERR_DEVICE, "hipEventSynchronize failed"));
                std::memcpy(h_dst + (size_t)(k - 1) * block, h_pin[ps], bytes_of(k - 1));
            }
        }
        HIP_TRY(hipStreamSynchronize(s));
        return VET_OK;
    }

    // the owner has synchronised the render stream
    void release() {
        if (copy) (void)hipStreamSynchronize(copy);
        free_blocks();
        for (int i = 0; i < 2; ++i) {
            if (computed[i]) (void)hipEventDestroy(computed[i]);
            if (copied[i]) (void)hipEventDestroy(copied[i]);
        }
        if (copy) (void)hipStreamDestroy(copy);
    }
};

}  // namespace

// ---- per-frame tile-attention heatmaps (include/vet.h) ----------------------------------------------------------------
struct vet_heatmap {
    vet_ctx* ctx = nullptr;
    int device = 0;
    HeatmapGeom g;
    bool latlon = false;                 // lat/lon cells of a naive tiling (vet_heatmap_create_latlon), not a lattice's tiles
    int n_lat = 0;                       // lat/lon: cells per lon column (the map holds slots lj * n_lon + li)
    uint16_t* d_map = nullptr;           // [H][W]
    uint32_t* d_pal = nullptr;           // grow-only palette [T][n] (both render entries)
    size_t pal_cap = 0;
    // the host entries: sub-blocks of B frames; everything but the RGB blocks is consumed in stream order on the context's
    // stream, so one copy of the uploads suffices; the RGB blocks and their pinned copies are the download pipeline's
    int B = 0, U = -1;
    int32_t* d_present = nullptr;
    double *d_mu = nullptr, *d_mv = nullptr;
    BlockDownload dl;
};

static void heatmap_release_staging(vet_heatmap* hm) {
    if (hm->d_present) (void)hipFree(hm->d_present);
    if (hm->d_mu) (void)hipFree(hm->d_mu);
    if (hm->d_mv) (void)hipFree(hm->d_mv);
    hm->d_present = nullptr; hm->d_mu = hm->d_mv = nullptr;
    hm->B = 0; hm->U = -1;
}

static int heatmap_palette(vet_heatmap* hm, int T, hipStream_t s) {
    const size_t bytes = (size_t)T * hm->g.n * 4;
    if (hm->pal_cap >= bytes) return VET_OK;
    if (hm->d_pal) {
        HIP_TRY(hipStreamSynchronize(s));      // a pending render of the same heatmap may still read it
        HIP_TRY(hipFree(hm->d_pal));
        hm->d_pal = nullptr; hm->pal_cap = 0;
    }
    HIP_TRY(hipMalloc((void**)&hm->d_pal, bytes));
    hm->pal_cap = bytes;
    return VET_OK;
}

// both device-pointer entries: checks first, then the palette, fill and markers of frames [0, T) on `stream`
template <typename Wt>
static int heatmap_render_device(vet_heatmap* hm, const Wt* d_weights, const int32_t* d_present, const double* d_mu,
                                 const double* d_mv, int U, int T, uint8_t* d_rgb, void* stream) {
    if (!hm || !d_weights || !d_present || !d_rgb) return fail(VET_ERR_INVALID, "heatmap, weights, present or rgb is NULL");
    if (hm->latlon) return fail(VET_ERR_INVALID, "a lat/lon heatmap renders samples (vet_heatmap_render_binned*)");
    if (T < 0) return fail(VET_ERR_INVALID, "n_frames must be >= 0 (got %d)", T);
    if (!d_mu != !d_mv) return fail(VET_ERR_INVALID, "pass both d_mu and d_mv, or neither");
    if (d_mu && U <= 0) return fail(VET_ERR_INVALID, "n_users must be positive with samples (got %d)", U);
    if ((uintptr_t)d_rgb % 4) return fail(VET_ERR_INVALID, "d_rgb must be 4-byte aligned");
    if (T == 0) return VET_OK;
    HIP_TRY(hipSetDevice(hm->device));
    hipStream_t s = stream ? (hipStream_t)stream : hm->ctx->stream;
    int rc = heatmap_palette(hm, T, s);
    if (rc) return rc;
    return heatmap_render(hm->ctx, hm->g, d_weights, d_present, d_mu, d_mv, U, T, hm->d_pal, d_rgb, s);
}

// The render pipeline of the host entries: frames [row0, row0 + n_rows) in sub-blocks of B frames through the download
// pipeline.  Each block's h_present (when given) and samples are uploaded first, after the pipeline's wait for the block's
// RGB buffer; render_block(f0, b, d_mu, d_mv, d_rgb) then enqueues frames [f0, f0 + b) on the context's stream (d_mu /
// d_mv: the block's samples, or null without h_mu).  The palette holds pal_frames frames.
template <typename Render>
static int heatmap_render_blocks(vet_heatmap* hm, int B, int pal_frames, const int32_t* h_present, const double* h_mu,
                                 const double* h_mv, int U, int64_t row0, int64_t n_rows, uint8_t* h_rgb,
                                 Render render_block) {
    hipStream_t s = hm->ctx->stream;
    const size_t frame = (size_t)hm->g.W * hm->g.H * 3;
    if (hm->B < B || (h_mu && hm->U < U)) {                 // grow-only staging of the uploads
        HIP_TRY(hipStreamSynchronize(s));
        heatmap_release_staging(hm);
        const int UU = h_mu ? U : 0;
        HIP_TRY(hipMalloc((void**)&hm->d_present, (size_t)B * 4));
        HIP_TRY(hipMalloc((void**)&hm->d_mu, (size_t)B * std::max(UU, 1) * 8));
        HIP_TRY(hipMalloc((void**)&hm->d_mv, (size_t)B * std::max(UU, 1) * 8));
        hm->B = B; hm->U = UU;
    }
    int rc = heatmap_palette(hm, pal_frames, s);
    if (rc) return rc;
    return hm->dl.run(s, (size_t)n_rows * frame, (size_t)B * frame, h_rgb, [&](int64_t k, uint8_t* d_rgb) -> int {
        const int b = (int)std::min<int64_t>(B, n_rows - k * B);
        if (h_present && hipMemcpyAsync(hm->d_present, h_present + k * B, (size_t)b * 4, hipMemcpyHostToDevice, s) != hipSuccess)
            return fail(VET_ERR_DEVICE, "upload of the user counts failed");
        if (h_mu && (hipMemcpyAsync(hm->d_mu, h_mu + k * B * (int64_t)U, (size_t)b * U * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
                     hipMemcpyAsync(hm->d_mv, h_mv + k * B * (int64_t)U, (size_t)b * U * 8, hipMemcpyHostToDevice, s) != hipSuccess))
            return fail(VET_ERR_DEVICE, "upload of the samples failed");
        return render_block(row0 + k * B, b, h_mu ? hm->d_mu : nullptr, h_mu ? hm->d_mv : nullptr, d_rgb);
    });
}

extern "C" {

static int run_host(vet_plan* pl, bool transition, const double* h_mu, const double* h_mv, const int32_t* h_ids,
                    int U, int T, double* h_entropy, int32_t* h_a, void* h_b, int32_t* h_c, vet_result** keep = nullptr) {
    int rc = check_host_args(pl, U, T, h_entropy, h_mu, h_mv, h_ids);
    if (rc) return rc;
    const size_t S = (size_t)U * T;
    const int R = transition ? T - 1 : T;
    const int n0 = pl->lat[0].n;
    StagedRun run;
    rc = run.begin(pl, h_mu, h_mv, h_ids, S);
    if (rc) return rc;
    vet_ctx* c = run.c;
    hipStream_t s = run.s;
    double* ent = nullptr;
    int32_t *a = nullptr, *cc = nullptr;
    void* b = nullptr;
    POOL(SLOT_ENTROPY, (size_t)(R > 0 ? R : 1) * 8, ent);
    const size_t a_bytes = transition ? (size_t)(R > 0 ? R : 0) * U * 2 * 4 : S * 4;
    const size_t b_bytes = transition ? (size_t)(R > 0 ? R : 0) * n0 * 4 : (size_t)T * n0 * 8;
    ResultPtr res;
    if (keep) {
        // the optional outputs stay in device memory of their own, owned by the result handle
        *keep = nullptr;
        res.reset(new vet_result());
        res->device = c->device;
        res->transition = transition;
        res->rows = R > 0 ? R : 0;
        res->row_bytes[0] = transition ? (size_t)U * 2 * 4 : (size_t)U * 4;
        res->row_bytes[1] = transition ? (size_t)n0 * 4 : (size_t)n0 * 8;
        res->lazy_weights = !transition && pl->weighted && !pl->lat[0].binned && !pl->raw_weights &&
                            (size_t)U * 4 <= (size_t)n0 * 8;
        bool ok = hipMalloc(&res->d[0], a_bytes ? a_bytes : 8) == hipSuccess;
        if (res->lazy_weights) {
            rc = ensure_exact_weights(pl, s);      // the rows a fetched block gathers (precise sweep if they do not fit)
            if (rc) return rc;
        }
        if (ok && res->lazy_weights) {
            res->core = pl->wcore; res->U = U;
            ok = hipMalloc((void**)&res->d_ids, S * 4 ? S * 4 : 8) == hipSuccess;
        } else if (ok) {
            ok = hipMalloc(&res->d[1], b_bytes ? b_bytes : 8) == hipSuccess;
        }
        if (!ok) {
            (void)hipGetLastError();
            return fail(VET_ERR_DEVICE, "out of device memory for the resident outputs (%zu B)", a_bytes + b_bytes);
        }
        a = (int32_t*)res->d[0]; b = res->d[1];
    } else {
        if (h_a) POOL(SLOT_OUT0, a_bytes, a);
        if (h_b) POOL(SLOT_OUT1, b_bytes, b);
    }
    POOL(SLOT_COUNT, (size_t)(R > 0 ? R : 1) * 4, cc);
    rc = run.clear_status();
    if (rc) return rc;
    if (transition) {
        rc = run.ids ? vet_transition_entropy_ids(pl, run.ids, U, T, ent, a, (int32_t*)b, cc, run.status, s)
                     : vet_transition_entropy(pl, run.mu, run.mv, U, T, ent, a, (int32_t*)b, cc, run.status, s);
    } else {
        rc = run.ids ? vet_spatial_entropy_ids(pl, run.ids, U, T, ent, a, (double*)b, cc, run.status, s)
                     : vet_spatial_entropy(pl, run.mu, run.mv, U, T, ent, a, (double*)b, cc, run.status, s);
    }
    if (rc) return run.drain(rc);
    if (res && res->lazy_weights) {
        // the direction ids the weight rows are recomputed from on fetch
        if (run.ids) HIP_TRY(hipMemcpyAsync(res->d_ids, run.ids, S * 4, hipMemcpyDeviceToDevice, s));
        else {
            rc = sample_ids(pl, run.mu, run.mv, (long)S, res->d_ids, s);
            if (rc) return run.drain(rc);
        }
    }
    if (R > 0) {                                            // a transition run of one frame has no row: nothing to read
        HIP_TRY(hipMemcpyAsync(h_entropy, ent, (size_t)R * 8, hipMemcpyDeviceToHost, s));
        if (h_a) HIP_TRY(hipMemcpyAsync(h_a, a, a_bytes, hipMemcpyDeviceToHost, s));
        if (h_b) HIP_TRY(hipMemcpyAsync(h_b, b, b_bytes, hipMemcpyDeviceToHost, s));
        if (h_c) HIP_TRY(hipMemcpyAsync(h_c, cc, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    }
    rc = run.sync(R > 0);
    if (rc) return rc;
    if (keep) *keep = res.release();                        // outputs are written also when a status word is set
    return run.decode(empty_rows_message(transition));
}

int vet_spatial_entropy_host_resident(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U,
                                      int T, double* h_entropy, int32_t* h_present, vet_result** out) {
    if (!out) return fail(VET_ERR_INVALID, "out is NULL");
    return run_host(pl, false, h_mu, h_mv, h_ids, U, T, h_entropy, nullptr, nullptr, h_present, out);
}

int vet_transition_entropy_host_resident(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids,
                                         int U, int T, double* h_entropy, int32_t* h_common, vet_result** out) {
    if (!out) return fail(VET_ERR_INVALID, "out is NULL");
    return run_host(pl, true, h_mu, h_mv, h_ids, U, T, h_entropy, nullptr, nullptr, h_common, out);
}

int vet_result_fetch(vet_result* r, int which, int64_t row0, int64_t n_rows, void* h_dst) {
    if (!r || !h_dst) return fail(VET_ERR_INVALID, "result or destination is NULL");
    if (which < 0 || which > 1) return fail(VET_ERR_INVALID, "which must be 0 (assignments / pairs) or 1 (weights / source counts)");
    if (row0 < 0 || n_rows < 0 || row0 + n_rows > r->rows)
        return fail(VET_ERR_INVALID, "rows [%lld, %lld) outside the result's %lld rows", (long long)row0,
                    (long long)(row0 + n_rows), (long long)r->rows);
    if (n_rows == 0) return VET_OK;
    HIP_TRY(hipSetDevice(r->device));
    if (which == 1 && r->lazy_weights) {
        // tile_weights rows [row0, row0 + n_rows): computed now, from the resident direction ids (null stream: the
        // call that made the result has synchronised its stream, and the result may have outlived its context)
        std::lock_guard<std::mutex> lock(r->fetch_mu);
        int rc = result_tmp_rows(r, n_rows);
        if (rc) return rc;
        rc = weights_pass_ids(*r->core, r->d_ids + (size_t)row0 * r->U, r->U, (int)n_rows, (double*)r->d_tmp, nullptr, nullptr);
        if (rc) return rc;
        HIP_TRY(hipMemcpy(h_dst, r->d_tmp, (size_t)n_rows * r->row_bytes[1], hipMemcpyDeviceToHost));
        return VET_OK;
    }
    HIP_TRY(hipMemcpy(h_dst, (const char*)r->d[which] + (size_t)row0 * r->row_bytes[which], (size_t)n_rows * r->row_bytes[which],
                      hipMemcpyDeviceToHost));
    return VET_OK;
}

int vet_result_free(vet_result* r) {
    if (!r) return VET_OK;
    (void)hipSetDevice(r->device);
    for (void* q : r->d) if (q) (void)hipFree(q);
    if (r->d_ids) (void)hipFree(r->d_ids);
    if (r->d_tmp) (void)hipFree(r->d_tmp);
    delete r;
    return VET_OK;
}

int vet_spatial_entropy_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U,
                             int T, double* h_entropy, int32_t* h_assign, double* h_weights, int32_t* h_present) {
    return run_host(pl, false, h_mu, h_mv, h_ids, U, T, h_entropy, h_assign, h_weights, h_present);
}

int vet_transition_entropy_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U,
                                int T, double* h_entropy, int32_t* h_pairs, int32_t* h_srccount,
                                int32_t* h_common) {
    return run_host(pl, true, h_mu, h_mv, h_ids, U, T, h_entropy, h_pairs, h_srccount, h_common);
}

// Sliding-window spatial entropy with host buffers (include/vet.h): staged like run_host, R = vet_window_rows output rows
int vet_spatial_entropy_windowed_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T,
                                      int window, int stride, double* h_entropy, double* h_weights, int32_t* h_samples) {
    int64_t R;
    int rc = check_row_args(pl, U, T, window, stride, false, h_entropy, h_mu, h_mv, h_ids, &R);
    if (rc) return rc;
    const RowOut outs[3] = {{h_entropy, (size_t)R * 8, SLOT_ENTROPY}, {h_weights, (size_t)R * pl->lat[0].n * 8, SLOT_OUT1},
                            {h_samples, (size_t)R * 4, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, "%d window(s) without any sample (Empty vector dictionary)",
                       [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_spatial_entropy_windowed_ids, vet_spatial_entropy_windowed, pl, U, T, window, stride,
                           (double*)d[0], (double*)d[1], (int32_t*)d[2], run.status, run.s);
    });
}

// Per-viewer spatial entropy with host buffers (include/vet.h): staged like the windowed entry, n_users * vet_window_rows output
// rows, user-major.  Rows without a sample are data (NaN, samples 0): only VET_ERR_RANGE is decoded from the status words.
int vet_user_entropy_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window,
                          int stride, double* h_entropy, double* h_weights, int32_t* h_samples) {
    int64_t R;
    int rc = check_row_args(pl, U, T, window, stride, false, h_entropy, h_mu, h_mv, h_ids, &R);
    if (rc) return rc;
    const size_t rows = (size_t)R * U;
    const RowOut outs[3] = {{h_entropy, rows * 8, SLOT_ENTROPY}, {h_weights, rows * pl->lat[0].n * 8, SLOT_OUT1},
                            {h_samples, rows * 4, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_user_entropy_ids, vet_user_entropy, pl, U, T, window, stride, (double*)d[0], (double*)d[1],
                           (int32_t*)d[2], run.status, run.s);
    });
}

// Pairwise viewer divergence with host buffers (include/vet.h): vet_window_rows matrices of n_users x n_users, samples user-major.
// (row, viewer) slots without a sample are data (NaN rows and columns): only VET_ERR_RANGE is decoded from the status words.
int vet_user_divergence_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window,
                             int stride, double* h_div, int32_t* h_samples) {
    int64_t R;
    int rc = check_row_args(pl, U, T, window, stride, false, h_div, h_mu, h_mv, h_ids, &R);
    if (rc) return rc;
    const size_t rows = (size_t)R * U;
    const RowOut outs[3] = {{h_div, rows * U * 8, SLOT_ENTROPY}, kNoOut, {h_samples, rows * 4, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_user_divergence_ids, vet_user_divergence, pl, U, T, window, stride, (double*)d[0],
                           (int32_t*)d[2], run.status, run.s);
    });
}

// Viewer-to-crowd divergence with host buffers (include/vet.h): n_users * vet_window_rows values, user-major, and the three row
// series.  (row, viewer) slots without a sample are data (NaN): only VET_ERR_RANGE is decoded from the status words.
int vet_crowd_divergence_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window,
                              int stride, double* h_div, double* h_rows, int32_t* h_samples) {
    int64_t R;
    int rc = check_row_args(pl, U, T, window, stride, false, h_div, h_mu, h_mv, h_ids, &R);
    if (rc) return rc;
    const size_t slots = (size_t)R * U;
    const RowOut outs[3] = {{h_div, slots * 8, SLOT_ENTROPY}, {h_rows, (size_t)3 * R * 8, SLOT_OUT1}, {h_samples, slots * 4, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_crowd_divergence_ids, vet_crowd_divergence, pl, U, T, window, stride, (double*)d[0],
                           (double*)d[1], (int32_t*)d[2], run.status, run.s);
    });
}

// Bootstrap confidence bands with host buffers (include/vet.h): the summary [4][R], and where wanted the replicates [R][B], lattice
// 0's replicate histograms [R][B][n_0] and the finite replicates per row.  Four outputs, so its own staged run.  Replicates without
// a sample are data (NaN): only VET_ERR_RANGE is decoded from the status words.
int vet_bootstrap_entropy_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window,
                               int stride, int replicates, uint64_t seed, double confidence, double* h_summary, double* h_replicates,
                               double* h_weights, int32_t* h_valid) {
    int64_t R;
    int rc = check_row_args(pl, U, T, window, stride, false, h_summary, h_mu, h_mv, h_ids, &R);
    if (!rc) rc = check_bootstrap_args(pl, U, replicates, confidence);
    if (rc) return rc;
    StagedRun run;
    rc = run.begin(pl, h_mu, h_mv, h_ids, (size_t)U * T);
    if (rc) return rc;
    vet_ctx* c = run.c;
    const size_t reps = (size_t)R * replicates;
    struct { void* h; size_t bytes; int slot; void* d; } outs[4] = {
        {h_summary, (size_t)4 * R * 8, SLOT_ENTROPY, nullptr}, {h_replicates, reps * 8, SLOT_OUT0, nullptr},
        {h_weights, reps * pl->lat[0].n * 8, SLOT_OUT1, nullptr}, {h_valid, (size_t)R * 4, SLOT_COUNT, nullptr}};
    for (auto& o : outs)
        if (o.h) POOL(o.slot, o.bytes, o.d);
    rc = run.clear_status();
    if (rc) return rc;
    rc = launch_rows(run, vet_bootstrap_entropy_ids, vet_bootstrap_entropy, pl, U, T, window, stride, replicates, seed, confidence,
                     (double*)outs[0].d, (double*)outs[1].d, (double*)outs[2].d, (int32_t*)outs[3].d, run.status, run.s);
    if (rc) return run.drain(rc);
    for (auto& o : outs)
        if (o.h) HIP_TRY(hipMemcpyAsync(o.h, o.d, o.bytes, hipMemcpyDeviceToHost, run.s));
    return run.finish_rows_are_data();
}

// The two-audience permutation test with host buffers (include/vet.h): the summary [5][R], and where wanted the null distribution
// [R][P], labelling 0's two histograms of lattice 0 [R][2][n_0], the observed groups' samples [2][R] and the finite null values per
// row.  Five outputs on four slots: samples and valid share the count slot.  Rows in which a group has no sample are data (NaN):
// only VET_ERR_RANGE is decoded from the status words.
int vet_group_divergence_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window,
                              int stride, const int8_t* groups, int permutations, uint64_t seed, double confidence, double* h_summary,
                              double* h_null, double* h_weights, int32_t* h_samples, int32_t* h_valid) {
    int64_t R;
    int rc = check_row_args(pl, U, T, window, stride, false, h_summary, h_mu, h_mv, h_ids, &R);
    if (!rc) rc = check_group_args(pl, U, groups, permutations, confidence);
    if (rc) return rc;
    StagedRun run;
    rc = run.begin(pl, h_mu, h_mv, h_ids, (size_t)U * T);
    if (rc) return rc;
    vet_ctx* c = run.c;
    double *d_summary = nullptr, *d_null = nullptr, *d_weights = nullptr;
    int32_t* d_counts = nullptr;                                   // samples [2][R] | valid [R]
    const size_t null_bytes = (size_t)R * permutations * 8, w_bytes = (size_t)R * 2 * pl->lat[0].n * 8;
    POOL(SLOT_ENTROPY, (size_t)5 * R * 8, d_summary);
    if (h_null) POOL(SLOT_OUT0, null_bytes, d_null);
    if (h_weights) POOL(SLOT_OUT1, w_bytes, d_weights);
    POOL(SLOT_COUNT, (size_t)3 * R * 4, d_counts);
    rc = run.clear_status();
    if (rc) return rc;
    rc = launch_rows(run, vet_group_divergence_ids, vet_group_divergence, pl, U, T, window, stride, groups, permutations, seed,
                     confidence, d_summary, d_null, d_weights, h_samples ? d_counts : nullptr, h_valid ? d_counts + 2 * R : nullptr,
                     run.status, run.s);
    if (rc) return run.drain(rc);
    HIP_TRY(hipMemcpyAsync(h_summary, d_summary, (size_t)5 * R * 8, hipMemcpyDeviceToHost, run.s));
    if (h_null) HIP_TRY(hipMemcpyAsync(h_null, d_null, null_bytes, hipMemcpyDeviceToHost, run.s));
    if (h_weights) HIP_TRY(hipMemcpyAsync(h_weights, d_weights, w_bytes, hipMemcpyDeviceToHost, run.s));
    if (h_samples) HIP_TRY(hipMemcpyAsync(h_samples, d_counts, (size_t)2 * R * 4, hipMemcpyDeviceToHost, run.s));
    if (h_valid) HIP_TRY(hipMemcpyAsync(h_valid, d_counts + 2 * R, (size_t)R * 4, hipMemcpyDeviceToHost, run.s));
    return run.finish_rows_are_data();
}

// Window-to-window divergence with host buffers (include/vet.h): vet_window_rows rows of max_lag lags.  Rows without a sample are
// data (NaN across their band): only VET_ERR_RANGE is decoded from the status words.
int vet_window_divergence_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window,
                               int stride, int max_lag, double* h_div, int32_t* h_samples) {
    int64_t R;
    int rc = check_row_args(pl, U, T, window, stride, false, h_div, h_mu, h_mv, h_ids, &R);
    if (rc) return rc;
    if (max_lag < 1 || max_lag > R - 1)
        return fail(VET_ERR_INVALID, "max_lag must be between 1 and rows - 1 = %lld (got %d)", (long long)(R - 1), max_lag);
    const RowOut outs[3] = {{h_div, (size_t)R * max_lag * 8, SLOT_ENTROPY}, kNoOut, {h_samples, (size_t)R * 4, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_window_divergence_ids, vet_window_divergence, pl, U, T, window, stride, max_lag, (double*)d[0],
                           (int32_t*)d[2], run.status, run.s);
    });
}

// Attention coverage with host buffers (include/vet.h): tiles [R][Q], hit [R][max_lag + 1][Q], and where wanted order [R][n_0] and
// the samples per row.  Rows without a sample are data (tiles 0, hit NaN): only VET_ERR_RANGE is decoded from the status words.
int vet_coverage_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window,
                      int stride, int max_lag, const double* fractions, int Q, int32_t* h_tiles, double* h_hit, int32_t* h_order,
                      int32_t* h_samples) {
    int64_t R;
    int rc = check_row_args(pl, U, T, window, stride, false, (const double*)h_tiles, h_mu, h_mv, h_ids, &R);
    if (!rc) rc = check_coverage_args(pl, (long)R, max_lag, fractions, Q, h_hit);
    if (rc) return rc;
    const RowOut outs[4] = {{h_tiles, (size_t)R * Q * 4, SLOT_OUT0}, {h_hit, (size_t)R * (max_lag + 1) * Q * 8, SLOT_ENTROPY},
                            {h_order, (size_t)R * pl->lat[0].n * 4, SLOT_OUT1}, {h_samples, (size_t)R * 4, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_coverage_ids, vet_coverage, pl, U, T, window, stride, max_lag, fractions, Q, (int32_t*)d[0],
                           (double*)d[1], (int32_t*)d[2], (int32_t*)d[3], run.status, run.s);
    });
}

// Per-viewer transition entropy with host buffers (include/vet.h): n_users * vet_window_rows(T - 1, ..) output rows, user-major.
// Rows without a common sample are data (NaN, samples 0): only VET_ERR_RANGE is decoded from the status words.
int vet_user_transition_entropy_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T,
                                     int window, int stride, double* h_entropy, int32_t* h_srccount, int32_t* h_samples) {
    int rc = check_user_transition_args(pl, U, T, window, stride, h_entropy);     // before the samples are looked at or staged
    if (rc) return rc;
    int64_t R;
    rc = check_row_args(pl, U, T, window, stride, true, h_entropy, h_mu, h_mv, h_ids, &R);
    if (rc) return rc;
    const size_t rows = (size_t)R * U;
    const RowOut outs[3] = {{h_entropy, rows * 8, SLOT_ENTROPY}, {h_srccount, rows * pl->lat[0].n * 4, SLOT_OUT1},
                            {h_samples, rows * 4, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_user_transition_entropy_ids, vet_user_transition_entropy, pl, U, T, window, stride,
                           (double*)d[0], (int32_t*)d[1], (int32_t*)d[2], run.status, run.s);
    });
}

// Sliding-window transition entropy with host buffers (include/vet.h): R = vet_window_rows over the T - 1 frame pairs
int vet_transition_entropy_windowed_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T,
                                         int window, int stride, double* h_entropy, int32_t* h_srccount, int32_t* h_samples) {
    int64_t R;
    int rc = check_row_args(pl, U, T, window, stride, true, h_entropy, h_mu, h_mv, h_ids, &R);
    if (rc) return rc;
    if ((int64_t)window * U >= ((int64_t)1 << 19))           // before the samples are staged; the device entry says the same
        return fail(VET_ERR_UNSUPPORTED, "windowed transition: window * n_users = %lld pooled samples per row, the kernel packs "
                    "fewer than 2^19", (long long)window * U);
    const RowOut outs[3] = {{h_entropy, (size_t)R * 8, SLOT_ENTROPY}, {h_srccount, (size_t)R * pl->lat[0].n * 4, SLOT_OUT1},
                            {h_samples, (size_t)R * 4, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, "%d window(s) without a (pair, user) sample present in both frames",
                       [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_transition_entropy_windowed_ids, vet_transition_entropy_windowed, pl, U, T, window, stride,
                           (double*)d[0], (int32_t*)d[1], (int32_t*)d[2], run.status, run.s);
    });
}

// Windowed Markov transition statistics with host buffers (include/vet.h): stats [5][R], and where wanted lattice 0's matrices
// [R][n_0][n_0] and the samples per row, R = vet_window_rows over the T - lag pairs.  Rows without a pooled sample are data (NaN,
// samples 0, a zero matrix): only VET_ERR_RANGE is decoded from the status words.
int vet_transition_markov_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window,
                               int stride, int lag, double* h_stats, int32_t* h_matrix, int32_t* h_samples) {
    int rc = check_host_args(pl, U, T, h_stats, h_mu, h_mv, h_ids);
    if (!rc) rc = check_markov_args(pl, U, T, window, stride, lag, h_stats, h_matrix);
    if (rc) return rc;
    const size_t R = (size_t)vet_window_rows(T - lag, window, stride), n0 = (size_t)pl->lat[0].n;
    const RowOut outs[3] = {{h_stats, 5 * R * 8, SLOT_ENTROPY}, {h_matrix, R * n0 * n0 * 4, SLOT_OUT1}, {h_samples, R * 4, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_transition_markov_ids, vet_transition_markov, pl, U, T, window, stride, lag, (double*)d[0],
                           (int32_t*)d[1], (int32_t*)d[2], run.status, run.s);
    });
}

// Head-motion statistics with host buffers (include/vet.h): stats [4][Rows], and where wanted quantiles [Rows][Q], hist [Rows][B],
// still [Rows] and samples [Rows]; Rows = vet_window_rows over the T - lag pairs, times n_users for the per-viewer layout.  Rows
// without a sample are data: only VET_ERR_RANGE is decoded from the status words.
int vet_head_motion_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window, int stride,
                         int lag, int per_user, const double* h_fractions, int Q, const double* h_edges, int B, double* h_stats,
                         double* h_quantiles, int32_t* h_hist, int32_t* h_still, int32_t* h_samples) {
    int rc = check_host_args(pl, U, T, h_stats, h_mu, h_mv, h_ids);
    if (!rc) rc = check_motion_args(pl, U, T, window, stride, lag, per_user, h_fractions, Q, h_edges, B, h_stats);
    if (rc) return rc;
    const size_t rows = (size_t)vet_window_rows(T - lag, window, stride) * (per_user ? (size_t)U : 1);
    const RowOut outs[5] = {{h_stats, 4 * rows * 8, SLOT_ENTROPY}, {h_quantiles, rows * Q * 8, SLOT_OUT0}, {h_hist, rows * B * 4, SLOT_OUT1},
                            {h_still, rows * 4, SLOT_STILL}, {h_samples, rows * 4, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_head_motion_ids, vet_head_motion, pl, U, T, window, stride, lag, per_user, h_fractions, Q, h_edges, B,
                           (double*)d[0], (double*)d[1], (int32_t*)d[2], (int32_t*)d[3], (int32_t*)d[4], run.status, run.s);
    });
}

// Audience dispersion with host buffers (include/vet.h): where wanted stats [3][Rows], centroid [Rows][3], hist [Rows][B] and counts
// [4][Rows]; Rows = vet_window_rows over the T frames, times n_users for the per-viewer layout.  Every output may be NULL.  Rows
// without a pair are data: only VET_ERR_RANGE is decoded from the status words.
int vet_dispersion_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window, int stride,
                        int per_user, const double* h_edges, int B, double* h_stats, double* h_centroid, int64_t* h_hist,
                        int64_t* h_counts) {
    int rc = check_dispersion_args(pl, U, T, window, stride, per_user, h_edges, B);
    if (rc) return rc;
    if (!h_ids && (!h_mu || !h_mv)) return fail(VET_ERR_INVALID, "need h_mu and h_mv, or h_ids");       // no output is required
    if (!h_ids && !pl->grid) return fail(VET_ERR_INVALID, "plan has no pixel grid; pass h_ids");
    const size_t rows = (size_t)vet_window_rows(T, window, stride) * (per_user ? (size_t)U : 1);
    const RowOut outs[4] = {{h_stats, 3 * rows * 8, SLOT_ENTROPY}, {h_centroid, 3 * rows * 8, SLOT_OUT0}, {h_hist, rows * B * 8, SLOT_OUT1},
                            {h_counts, 4 * rows * 8, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_dispersion_ids, vet_dispersion, pl, U, T, window, stride, per_user, h_edges, B, (double*)d[0],
                           (double*)d[1], (int64_t*)d[2], (int64_t*)d[3], run.status, run.s);
    });
}

// Viewer clusters with host buffers (include/vet.h): where wanted labels [R][U], sizes [R][U], counts [5][R], top [R][Q], stats [3][R],
// centroids [R][U][3] and links [R][U][ceil(U / 64)]; R = vet_window_rows over the T frames.  Every output may be NULL.  Rows without
// a viewer are data: only VET_ERR_RANGE is decoded from the status words.
int vet_viewer_clusters_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window,
                             int stride, double cos_threshold, double min_share, const double* h_fractions, int Q, int32_t* h_labels,
                             int32_t* h_sizes, int64_t* h_counts, int32_t* h_top, double* h_stats, double* h_centroids,
                             uint64_t* h_links) {
    enum { SLOT_CENTROIDS = 10, SLOT_LINKS = 11 };
    int rc = check_cluster_args(pl, U, T, window, stride, cos_threshold, min_share, h_fractions, Q);
    if (rc) return rc;
    if (!h_ids && (!h_mu || !h_mv)) return fail(VET_ERR_INVALID, "need h_mu and h_mv, or h_ids");       // no output is required
    if (!h_ids && !pl->grid) return fail(VET_ERR_INVALID, "plan has no pixel grid; pass h_ids");
    const size_t rows = (size_t)vet_window_rows(T, window, stride), words = ((size_t)U + 63) / 64;
    if (!Q) h_top = nullptr;
    const RowOut outs[7] = {{h_labels, rows * U * 4, SLOT_OUT0}, {h_sizes, rows * U * 4, SLOT_OUT1}, {h_counts, 5 * rows * 8, SLOT_COUNT},
                            {h_top, rows * Q * 4, SLOT_STILL}, {h_stats, 3 * rows * 8, SLOT_ENTROPY},
                            {h_centroids, rows * U * 24, SLOT_CENTROIDS}, {h_links, rows * U * words * 8, SLOT_LINKS}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_viewer_clusters_ids, vet_viewer_clusters, pl, U, T, window, stride, cos_threshold, min_share,
                           h_fractions, Q, (int32_t*)d[0], (int32_t*)d[1], (int64_t*)d[2], (int32_t*)d[3], (double*)d[4], (double*)d[5],
                           (uint64_t*)d[6], run.status, run.s);
    });
}

// Fixation and tile-dwell events with host buffers (include/vet.h): where wanted counts [5][Rows], hist [Rows][B], labels [U][T],
// offsets [U + 1], events [max_events][4] and centroids [max_events][3]; Rows = vet_window_rows over the T frames, times n_users for
// the per-viewer layout.  Every output may be NULL.  Rows without a sample are data: only VET_ERR_RANGE is decoded from the status
// words.  The event outputs take a second call: the first, with max_events = 0 and h_offsets, gives their number, offsets[U].
int vet_fixations_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window, int stride,
                       int mode, double cos_threshold, int min_frames, int per_user, const int32_t* h_edges, int B, int64_t max_events,
                       int64_t* h_counts, int32_t* h_hist, int32_t* h_labels, int64_t* h_offsets, int32_t* h_events,
                       double* h_centroids) {
    enum { SLOT_EVENTS = 10, SLOT_CENTROIDS = 11 };
    int rc = check_fixation_args(pl, U, T, window, stride, mode, cos_threshold, min_frames, h_edges, B, max_events, h_events,
                                 h_centroids);
    if (rc) return rc;
    if (!h_ids && (!h_mu || !h_mv)) return fail(VET_ERR_INVALID, "need h_mu and h_mv, or h_ids");       // no output is required
    if (!h_ids && !pl->grid) return fail(VET_ERR_INVALID, "plan has no pixel grid; pass h_ids");
    const size_t rows = (size_t)vet_window_rows(T, window, stride) * (per_user ? (size_t)U : 1), E = (size_t)max_events;
    if (!B) h_hist = nullptr;
    if (!E) h_events = nullptr, h_centroids = nullptr;
    const RowOut outs[6] = {{h_counts, 5 * rows * 8, SLOT_COUNT}, {h_hist, rows * B * 4, SLOT_OUT1}, {h_labels, (size_t)U * T * 4, SLOT_OUT0},
                            {h_offsets, ((size_t)U + 1) * 8, SLOT_ENTROPY}, {h_events, E * 16, SLOT_EVENTS},
                            {h_centroids, E * 24, SLOT_CENTROIDS}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_fixations_ids, vet_fixations, pl, U, T, window, stride, mode, cos_threshold, min_frames, per_user,
                           h_edges, B, max_events, (int64_t*)d[0], (int32_t*)d[1], (int32_t*)d[2], (int64_t*)d[3], (int32_t*)d[4],
                           (double*)d[5], run.status, run.s);
    });
}

// Saliency maps with host buffers (include/vet.h): where wanted map [Rows][H][W], stats [4][Rows], peak [Rows] and counts [2][Rows];
// Rows = vet_window_rows over the T frames, times n_users for the per-viewer layout.  Every output may be NULL.  Rows without a
// sample are data: only VET_ERR_RANGE is decoded from the status words.
int vet_saliency_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window, int stride,
                      int per_user, double sigma_rad, int W, int H, int scale, double* h_map, double* h_stats, int32_t* h_peak,
                      int64_t* h_counts) {
    int rc = check_saliency_args(pl, U, T, window, stride, per_user, sigma_rad, W, H, scale);
    if (rc) return rc;
    if (!h_ids && (!h_mu || !h_mv)) return fail(VET_ERR_INVALID, "need h_mu and h_mv, or h_ids");       // no output is required
    if (!h_ids && !pl->grid) return fail(VET_ERR_INVALID, "plan has no pixel grid; pass h_ids");
    const size_t rows = (size_t)vet_window_rows(T, window, stride) * (per_user ? (size_t)U : 1);
    const RowOut outs[4] = {{h_stats, 4 * rows * 8, SLOT_ENTROPY}, {h_map, rows * (size_t)W * H * 8, SLOT_OUT0}, {h_peak, rows * 4, SLOT_OUT1},
                            {h_counts, 2 * rows * 8, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_saliency_ids, vet_saliency, pl, U, T, window, stride, per_user, sigma_rad, W, H, scale, (double*)d[1],
                           (double*)d[0], (int32_t*)d[2], (int64_t*)d[3], run.status, run.s);
    });
}

// Saliency similarity with host buffers (include/vet.h): where wanted maps [2][Rows][H][W], stats [9][Rows] and counts [4][Rows];
// Rows = vet_window_rows over the T frames.  Every output may be NULL; groups [U] is host memory in every entry.  Rows with an empty
// audience are data: only VET_ERR_RANGE is decoded from the status words.
int vet_saliency_similarity_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window,
                                 int stride, const int8_t* groups, double sigma_rad, int W, int H, double* h_maps, double* h_stats,
                                 int64_t* h_counts) {
    int rc = check_similarity_args(pl, U, T, window, stride, groups, sigma_rad, W, H);
    if (rc) return rc;
    if (!h_ids && (!h_mu || !h_mv)) return fail(VET_ERR_INVALID, "need h_mu and h_mv, or h_ids");       // no output is required
    if (!h_ids && !pl->grid) return fail(VET_ERR_INVALID, "plan has no pixel grid; pass h_ids");
    const size_t rows = (size_t)vet_window_rows(T, window, stride);
    const RowOut outs[3] = {{h_stats, 9 * rows * 8, SLOT_ENTROPY}, {h_maps, 2 * rows * (size_t)W * H * 8, SLOT_OUT0},
                            {h_counts, 4 * rows * 8, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_saliency_similarity_ids, vet_saliency_similarity, pl, U, T, window, stride, groups, sigma_rad, W, H,
                           (double*)d[1], (double*)d[0], (int64_t*)d[2], run.status, run.s);
    });
}

// Viewer congruency with host buffers (include/vet.h): where wanted stats [3][U][R], counts [3][U][R] and rows [4][R]; R =
// vet_window_rows over the T frames.  Every output may be NULL.  Viewers without a sample or without company in a row are data: only
// VET_ERR_RANGE is decoded from the status words.
int vet_congruency_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window, int stride,
                        double sigma_rad, int want_nss, double* h_stats, int64_t* h_counts, double* h_rows) {
    int rc = check_congruency_args(pl, U, T, window, stride, sigma_rad);
    if (rc) return rc;
    if (!h_ids && (!h_mu || !h_mv)) return fail(VET_ERR_INVALID, "need h_mu and h_mv, or h_ids");       // no output is required
    if (!h_ids && !pl->grid) return fail(VET_ERR_INVALID, "plan has no pixel grid; pass h_ids");
    const size_t R = (size_t)vet_window_rows(T, window, stride);
    const RowOut outs[3] = {{h_stats, 3 * R * U * 8, SLOT_ENTROPY}, {h_rows, 4 * R * 8, SLOT_OUT0}, {h_counts, 3 * R * U * 8, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        return launch_rows(run, vet_congruency_ids, vet_congruency, pl, U, T, window, stride, sigma_rad, want_nss, (double*)d[0],
                           (int64_t*)d[2], (double*)d[1], run.status, run.s);
    });
}

// Saliency scoring with host buffers (include/vet.h): h_pred [n_pred][H][W] is uploaded to a pool slot behind the samples; where
// wanted map [R][H][W], stats [9][R] and counts [2][R]; R = vet_window_rows over the T frames.  Every output may be NULL.  Rows
// without a sample are data: only VET_ERR_RANGE is decoded from the status words.
int vet_saliency_score_host(vet_plan* pl, const double* h_mu, const double* h_mv, const int32_t* h_ids, int U, int T, int window,
                            int stride, double sigma_rad, int W, int H, const double* h_pred, int n_pred, int want_dist, double* h_map,
                            double* h_stats, int64_t* h_counts) {
    int rc = check_score_args(pl, U, T, window, stride, sigma_rad, W, H, h_pred, n_pred);
    if (rc) return rc;
    if (!h_ids && (!h_mu || !h_mv)) return fail(VET_ERR_INVALID, "need h_mu and h_mv, or h_ids");       // no output is required
    if (!h_ids && !pl->grid) return fail(VET_ERR_INVALID, "plan has no pixel grid; pass h_ids");
    const size_t rows = (size_t)vet_window_rows(T, window, stride), pred_bytes = (size_t)n_pred * W * H * 8;
    const RowOut outs[3] = {{h_stats, 9 * rows * 8, SLOT_ENTROPY}, {h_map, rows * (size_t)W * H * 8, SLOT_OUT0},
                            {h_counts, 2 * rows * 8, SLOT_COUNT}};
    return staged_rows(pl, h_mu, h_mv, h_ids, U, T, outs, kRowsAreData, [&](const StagedRun& run, void* const* d) {
        vet_ctx* c = run.c;
        double* d_pred = nullptr;
        POOL(SLOT_STILL, pred_bytes, d_pred);
        HIP_TRY(hipMemcpyAsync(d_pred, h_pred, pred_bytes, hipMemcpyHostToDevice, run.s));
        return launch_rows(run, vet_saliency_score_ids, vet_saliency_score, pl, U, T, window, stride, sigma_rad, W, H,
                           (const double*)d_pred, n_pred, want_dist, (double*)d[1], (double*)d[0], (int64_t*)d[2], run.status, run.s);
    });
}

// Both batch entries.  Concatenated host buffers: video v's samples start at element sum_{w<v} U_w*T_w of h_mu / h_mv, its
// rows (T_v frames; transition: T_v - 1 frame pairs) at sum_{w<v} rows_w of h_entropy / h_count, and its output 0 (U_v*T_v
// assignments; transition: U_v*(T_v-1) pairs of two) at the sum of the earlier videos' in h_out0.  Two H2D copies, one
// launch (when the table formulation applies), two or three D2H copies.  Synchronous.
static int batch_host(vet_plan* pl, bool transition, int n_videos, const int* n_users, const int* n_frames, const double* h_mu,
                      const double* h_mv, double* h_entropy, int32_t* h_out0, int32_t* h_count) {
    if (!pl || n_videos <= 0 || !n_users || !n_frames || !h_mu || !h_mv || !h_entropy)
        return fail(VET_ERR_INVALID, "bad batch arguments");
    const int lost = transition ? 1 : 0;                    // frames of a video without a row
    auto rows_of = [&](int v) { return (size_t)n_frames[v] - lost; };
    auto out0_of = [&](int v) { return (size_t)n_users[v] * rows_of(v) * (transition ? 2 : 1); };
    size_t S = 0, R = 0, P = 0;
    for (int v = 0; v < n_videos; ++v) {
        if (n_users[v] <= 0 || n_frames[v] <= lost)
            return transition ? fail(VET_ERR_INVALID, "video %d: need users and at least two frames", v)
                              : fail(VET_ERR_INVALID, "video %d: bad shape", v);
        S += (size_t)n_users[v] * n_frames[v];
        R += rows_of(v);
        P += out0_of(v);
    }
    StagedRun run;
    int rc = run.begin(pl, h_mu, h_mv, nullptr, S);
    if (rc) return rc;
    vet_ctx* c = run.c;
    hipStream_t s = run.s;
    double* ent = nullptr;
    int32_t *out0 = nullptr, *cnt = nullptr;
    POOL(SLOT_ENTROPY, R * 8, ent);
    if (h_out0) POOL(SLOT_OUT0, P * 4, out0);
    if (h_count) POOL(SLOT_COUNT, R * 4, cnt);
    rc = run.clear_status();
    if (rc) return rc;
    std::vector<vet_video> vids(n_videos);
    size_t so = 0, ro = 0, po = 0;
    for (int v = 0; v < n_videos; ++v) {
        vids[v].d_mu = run.mu + so; vids[v].d_mv = run.mv + so;
        vids[v].n_users = n_users[v]; vids[v].n_frames = n_frames[v];
        vids[v].d_entropy = ent + ro;
        vids[v].d_assign = out0 ? out0 + po : nullptr;
        vids[v].d_present = cnt ? cnt + ro : nullptr;
        so += (size_t)n_users[v] * n_frames[v];
        ro += rows_of(v);
        po += out0_of(v);
    }
    rc = transition ? vet_transition_entropy_batch(pl, n_videos, vids.data(), run.status, s)
                    : vet_spatial_entropy_batch(pl, n_videos, vids.data(), run.status, s);
    if (rc) return run.drain(rc);
    HIP_TRY(hipMemcpyAsync(h_entropy, ent, R * 8, hipMemcpyDeviceToHost, s));
    if (h_out0) HIP_TRY(hipMemcpyAsync(h_out0, out0, P * 4, hipMemcpyDeviceToHost, s));
    if (h_count) HIP_TRY(hipMemcpyAsync(h_count, cnt, R * 4, hipMemcpyDeviceToHost, s));
    return run.finish(empty_rows_message(transition));
}

int vet_spatial_entropy_batch_host(vet_plan* pl, int n_videos, const int* n_users, const int* n_frames,
                                   const double* h_mu, const double* h_mv, double* h_entropy, int32_t* h_assign,
                                   int32_t* h_present) {
    return batch_host(pl, false, n_videos, n_users, n_frames, h_mu, h_mv, h_entropy, h_assign, h_present);
}

int vet_transition_entropy_batch_host(vet_plan* pl, int n_videos, const int* n_users, const int* n_frames,
                                      const double* h_mu, const double* h_mv, double* h_entropy, int32_t* h_pairs,
                                      int32_t* h_common) {
    return batch_host(pl, true, n_videos, n_users, n_frames, h_mu, h_mv, h_entropy, h_pairs, h_common);
}


// The frame checks of both create entries.
static int heatmap_frame_checks(int W, int H, int VW, int VH, int radius) {
    if (W <= 0 || H <= 0 || VW <= 0 || VH <= 0) return fail(VET_ERR_INVALID, "need width, height, video_width, video_height > 0");
    if ((int64_t)W * H > ((int64_t)1 << 31) / 3) return fail(VET_ERR_INVALID, "frame of %d x %d pixels is too large", W, H);
    if (radius < 0 || radius > 16) return fail(VET_ERR_INVALID, "marker_radius %d outside [0, 16]", radius);
    return VET_OK;
}

// Both create entries, after their checks: a new handle on the context's device with its geometry and an empty map.
static int heatmap_new(vet_ctx* c, int n, int W, int H, int VW, int VH, int radius, HeatmapPtr& hm) {
    HIP_TRY(hipSetDevice(c->device));
    hm.reset(new vet_heatmap());
    hm->ctx = c; hm->device = c->device;
    hm->g.n = n; hm->g.W = W; hm->g.H = H; hm->g.VW = VW; hm->g.VH = VH; hm->g.radius = radius;
    HIP_TRY(hipMalloc((void**)&hm->d_map, (size_t)W * H * sizeof(uint16_t)));
    hm->g.d_map = hm->d_map;
    return VET_OK;
}

int vet_heatmap_create(vet_ctx* c, const double* h_tiles, int n, int W, int H, int VW, int VH, int radius,
                       vet_heatmap** out) {
    if (!c || !h_tiles || !out) return fail(VET_ERR_INVALID, "ctx, tiles or out is NULL");
    *out = nullptr;
    if (n <= 0 || W <= 0 || H <= 0 || VW <= 0 || VH <= 0)
        return fail(VET_ERR_INVALID, "need n_tiles, width, height, video_width, video_height > 0");
    if (int rc = heatmap_frame_checks(W, H, VW, VH, radius)) return rc;
    if ((size_t)n * 3 * sizeof(double) > 160 * 1024 - 1024)
        return fail(VET_ERR_UNSUPPORTED, "lattice of %d tiles exceeds the LDS tile cache of k_heatmap_map", n);
    std::vector<double> unit((size_t)n * 3);
    for (int t = 0; t < n; ++t) {            // as vet_plan_create normalises its lattices
        const double x = h_tiles[3 * t], y = h_tiles[3 * t + 1], z = h_tiles[3 * t + 2];
        const double len = std::sqrt(x * x + y * y + z * z);
        if (!(len > 0.0)) return fail(VET_ERR_INVALID, "Vector cannot have zero length (tile %d)", t);
        unit[3 * t] = x / len; unit[3 * t + 1] = y / len; unit[3 * t + 2] = z / len;
    }
    HeatmapPtr hm;
    int rc = heatmap_new(c, n, W, H, VW, VH, radius, hm);
    if (rc) return rc;
    hipStream_t s = c->stream;
    DevBuf tiles;
    HIP_TRY(tiles.alloc(unit.size() * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(tiles.p, unit.data(), unit.size() * sizeof(double), hipMemcpyHostToDevice, s));
    rc = heatmap_map(c, (const double*)tiles.p, n, W, H, hm->d_map, s);
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    HIP_TRY(hipStreamSynchronize(s));         // 'unit' and 'tiles' go out of scope
    *out = hm.release();
    return VET_OK;
}

int vet_heatmap_create_latlon(vet_ctx* c, int tile_width, int tile_height, int W, int H, int VW, int VH, int radius,
                              vet_heatmap** out) {
    if (!c || !out) return fail(VET_ERR_INVALID, "ctx or out is NULL");
    *out = nullptr;
    if (tile_height <= 0 || tile_width <= 0) return fail(VET_ERR_INVALID, "No tile dimensions provided");
    if (180 % tile_height != 0) return fail(VET_ERR_INVALID, "Tile height must divide 180!");
    if (360 % tile_width != 0) return fail(VET_ERR_INVALID, "Tile width must divide 360!");
    if (int rc = heatmap_frame_checks(W, H, VW, VH, radius)) return rc;
    const int n = (360 / tile_width + 1) * (180 / tile_height + 1);   // the naive plan's bins: lon 180 and lat 90 open a cell
    if (n > 65535) return fail(VET_ERR_INVALID, "%d cells exceed 65535", n);
    HeatmapPtr hm;
    int rc = heatmap_new(c, n, W, H, VW, VH, radius, hm);
    if (rc) return rc;
    hm->latlon = true; hm->n_lat = 180 / tile_height + 1;
    hipStream_t s = c->stream;
    rc = heatmap_map_latlon(c, tile_width, tile_height, W, H, hm->d_map, s);
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    HIP_TRY(hipStreamSynchronize(s));
    *out = hm.release();
    return VET_OK;
}

int vet_heatmap_destroy(vet_heatmap* hm) {
    if (!hm) return VET_OK;
    (void)hipSetDevice(hm->device);
    if (hm->ctx) (void)hipStreamSynchronize(hm->ctx->stream);
    hm->dl.release();
    heatmap_release_staging(hm);
    if (hm->d_pal) (void)hipFree(hm->d_pal);
    if (hm->d_map) (void)hipFree(hm->d_map);
    delete hm;
    return VET_OK;
}

int vet_heatmap_read_map(vet_heatmap* hm, int32_t* h_map) {
    if (!hm || !h_map) return fail(VET_ERR_INVALID, "heatmap or output is NULL");
    HIP_TRY(hipSetDevice(hm->device));
    std::vector<uint16_t> tmp((size_t)hm->g.W * hm->g.H);
    HIP_TRY(hipMemcpy(tmp.data(), hm->d_map, tmp.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    const int n_lat = hm->n_lat, n_lon = hm->latlon ? hm->g.n / n_lat : 0;
    for (size_t i = 0; i < tmp.size(); ++i)                 // lat/lon: slot lj * n_lon + li -> cell li * n_lat + lj
        h_map[i] = hm->latlon ? (tmp[i] % n_lon) * n_lat + tmp[i] / n_lon : tmp[i];
    return VET_OK;
}

int vet_heatmap_render(vet_heatmap* hm, const double* d_weights, const int32_t* d_present, const double* d_mu,
                       const double* d_mv, int U, int T, uint8_t* d_rgb, void* stream) {
    return heatmap_render_device(hm, d_weights, d_present, d_mu, d_mv, U, T, d_rgb, stream);
}

int vet_heatmap_render_counts(vet_heatmap* hm, const int32_t* d_counts, const int32_t* d_present, const double* d_mu,
                              const double* d_mv, int U, int T, uint8_t* d_rgb, void* stream) {
    return heatmap_render_device(hm, d_counts, d_present, d_mu, d_mv, U, T, d_rgb, stream);
}

// The checks both result entries share, after the NULL and result-kind checks: device, lattice size (w_bytes per count or
// weight), row range, samples (u_bytes per user in a row of output 0: 4 for assignments, 8 for pairs).
static int heatmap_result_checks(vet_heatmap* hm, vet_result* r, size_t w_bytes, size_t u_bytes, const double* h_mu,
                                 const double* h_mv, int U, int64_t row0, int64_t n_rows) {
    if (hm->latlon) return fail(VET_ERR_INVALID, "a lat/lon heatmap renders samples (vet_heatmap_render_binned*), not a result");
    if (r->device != hm->device)
        return fail(VET_ERR_INVALID, "result on device %d, heatmap on device %d", r->device, hm->device);
    const int n = hm->g.n;
    if (r->row_bytes[1] != (size_t)n * w_bytes)
        return fail(VET_ERR_INVALID, "the result's lattice 0 has %zu tiles, the heatmap's lattice %d", r->row_bytes[1] / w_bytes, n);
    if (row0 < 0 || n_rows < 0 || row0 + n_rows > r->rows)
        return fail(VET_ERR_INVALID, "rows [%lld, %lld) outside the result's %lld rows", (long long)row0,
                    (long long)(row0 + n_rows), (long long)r->rows);
    if (!h_mu != !h_mv) return fail(VET_ERR_INVALID, "pass both h_mu and h_mv, or neither");
    const int RU = (int)(r->row_bytes[0] / u_bytes);
    if (h_mu && U != RU) return fail(VET_ERR_INVALID, "n_users %d, the result has %d", U, RU);
    return VET_OK;
}

// Frames per sub-block of the result entries: at most 32 MiB of RGB, at least one frame.
static int heatmap_block_frames(const vet_heatmap* hm, int64_t n_rows) {
    const size_t frame = (size_t)hm->g.W * hm->g.H * 3;
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)32 << 20, (size_t)n_rows * frame) / frame);
}

int vet_heatmap_render_result(vet_heatmap* hm, vet_result* r, const int32_t* h_present, const double* h_mu,
                              const double* h_mv, int U, int64_t row0, int64_t n_rows, uint8_t* h_rgb) {
    if (!hm || !r || !h_present || !h_rgb) return fail(VET_ERR_INVALID, "heatmap, result, present or rgb is NULL");
    if (r->transition) return fail(VET_ERR_INVALID, "a transition result has no tile weights to render");
    int rc = heatmap_result_checks(hm, r, 8, 4, h_mu, h_mv, U, row0, n_rows);
    if (rc || n_rows == 0) return rc;
    HIP_TRY(hipSetDevice(hm->device));
    const int B = heatmap_block_frames(hm, n_rows);
    // lazy weight rows: the weights pass of each block into the result's staging buffer, under its fetch lock
    std::unique_lock<std::mutex> lock(r->fetch_mu, std::defer_lock);
    if (r->lazy_weights) {
        lock.lock();
        rc = result_tmp_rows(r, B);
        if (rc) return rc;
    }
    const int n = hm->g.n;
    hipStream_t s = hm->ctx->stream;
    return heatmap_render_blocks(hm, B, B, h_present, h_mu, h_mv, U, row0, n_rows, h_rgb,
                                 [&](int64_t f0, int b, const double* d_mu, const double* d_mv, uint8_t* d_rgb) -> int {
        const double* w = (const double*)r->d[1] + (size_t)f0 * n;
        if (r->lazy_weights) {
            w = (const double*)r->d_tmp;
            int rc = weights_pass_ids(*r->core, r->d_ids + (size_t)f0 * r->U, r->U, b, (double*)r->d_tmp, s, nullptr);
            if (rc) return rc;
        }
        return heatmap_render(hm->ctx, hm->g, w, hm->d_present, d_mu, d_mv, U, b, hm->d_pal, d_rgb, s);
    });
}

int vet_heatmap_render_transition_result(vet_heatmap* hm, vet_result* r, const int32_t* h_present, const double* h_mu,
                                         const double* h_mv, int U, int64_t row0, int64_t n_rows, uint8_t* h_rgb) {
    if (!hm || !r || !h_present || !h_rgb) return fail(VET_ERR_INVALID, "heatmap, result, present or rgb is NULL");
    if (!r->transition)
        return fail(VET_ERR_INVALID, "a spatial result has no source-tile counts to render");
    int rc = heatmap_result_checks(hm, r, 4, 8, h_mu, h_mv, U, row0, n_rows);
    if (rc || n_rows == 0) return rc;
    HIP_TRY(hipSetDevice(hm->device));
    const int n = hm->g.n;
    const int B = heatmap_block_frames(hm, n_rows);
    return heatmap_render_blocks(hm, B, B, h_present, h_mu, h_mv, U, row0, n_rows, h_rgb,
                                 [&](int64_t f0, int b, const double* d_mu, const double* d_mv, uint8_t* d_rgb) -> int {
        return heatmap_render(hm->ctx, hm->g, (const int32_t*)r->d[1] + (size_t)f0 * n, hm->d_present, d_mu, d_mv, U, b,
                              hm->d_pal, d_rgb, hm->ctx->stream);
    });
}

// The checks both binned entries share, after the NULL checks: heatmap kind, the plan's lattice 0, cell count, video size
// and device; the users' LDS histogram.
static int heatmap_binned_checks(vet_heatmap* hm, vet_plan* pl, int U, int T) {
    if (T < 0) return fail(VET_ERR_INVALID, "n_frames must be >= 0 (got %d)", T);
    if (U <= 0) return fail(VET_ERR_INVALID, "n_users must be positive (got %d)", U);
    if (!hm->latlon) return fail(VET_ERR_INVALID, "a lattice heatmap has no lat/lon cells (vet_heatmap_create_latlon)");
    if (pl->lat.empty() || !pl->lat[0].binned || !pl->grid)
        return fail(VET_ERR_INVALID, "the plan's lattice 0 is not binned on a pixel grid");
    if (pl->lat[0].n != hm->g.n)
        return fail(VET_ERR_INVALID, "the plan's lattice 0 has %d bins, the heatmap %d cells", pl->lat[0].n, hm->g.n);
    if (pl->W != hm->g.VW || pl->H != hm->g.VH)
        return fail(VET_ERR_INVALID, "the plan's video is %d x %d, the heatmap's %d x %d", pl->W, pl->H, hm->g.VW, hm->g.VH);
    if (pl->ctx->device != hm->device)
        return fail(VET_ERR_INVALID, "plan on device %d, heatmap on device %d", pl->ctx->device, hm->device);
    if (!heatmap_bin_layout(hm->g.n, U).ok)
        return fail(VET_ERR_UNSUPPORTED, "%d users over %d cells exceed the LDS histogram of k_heatmap_bin_palette", U, hm->g.n);
    return VET_OK;
}

int vet_heatmap_render_binned(vet_heatmap* hm, vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T,
                              int markers, uint8_t* d_rgb, void* stream) {
    if (!hm || !pl || !d_mu || !d_mv || !d_rgb) return fail(VET_ERR_INVALID, "heatmap, plan, samples or rgb is NULL");
    if (int rc = heatmap_binned_checks(hm, pl, U, T)) return rc;
    if ((uintptr_t)d_rgb % 4) return fail(VET_ERR_INVALID, "d_rgb must be 4-byte aligned");
    if (T == 0) return VET_OK;
    HIP_TRY(hipSetDevice(hm->device));
    hipStream_t s = stream ? (hipStream_t)stream : hm->ctx->stream;
    int rc = heatmap_palette(hm, std::min(T, heatmap_bin_chunk(hm->g.n)), s);
    if (rc) return rc;
    return heatmap_render_binned(hm->ctx, hm->g, hm->n_lat, pl->lat[0].d_nearest, d_mu, d_mv, U, T, markers != 0, hm->d_pal,
                                 d_rgb, s);
}

int vet_heatmap_render_binned_host(vet_heatmap* hm, vet_plan* pl, const double* h_mu, const double* h_mv, int U, int T,
                                   int markers, uint8_t* h_rgb) {
    if (!hm || !pl || !h_mu || !h_mv || !h_rgb) return fail(VET_ERR_INVALID, "heatmap, plan, samples or rgb is NULL");
    if (int rc = heatmap_binned_checks(hm, pl, U, T)) return rc;
    if (T == 0) return VET_OK;
    HIP_TRY(hipSetDevice(hm->device));
    const int B = heatmap_block_frames(hm, T);
    return heatmap_render_blocks(hm, B, std::min(B, heatmap_bin_chunk(hm->g.n)), nullptr, h_mu, h_mv, U, 0, T, h_rgb,
                                 [&](int64_t, int b, const double* d_mu, const double* d_mv, uint8_t* d_rgb) -> int {
        return heatmap_render_binned(hm->ctx, hm->g, hm->n_lat, pl->lat[0].d_nearest, d_mu, d_mv, U, b, markers != 0,
                                     hm->d_pal, d_rgb, hm->ctx->stream);
    });
}

// ---- tilings on the unit sphere (include/vet.h) -----------------------------------------------------------------------
struct vet_tiling {
    vet_ctx* ctx = nullptr;
    int device = 0;
    TilingGeom g;
    double* d_pts = nullptr;             // [n_arcs][50][3]
    double* d_centres = nullptr;         // [n_centres][3] (null without centres)
    int B = 0;                           // frames per block: the flags of one block are B * H * W * 4 bytes
    uint32_t* d_flags = nullptr;         // [B][H][W]
    // cameras of a call, computed on the host: pinned copy (reused once the event says its upload has left) -> device
    TilingCam* h_cam = nullptr;
    TilingCam* d_cam = nullptr;
    int cam_cap = 0;
    hipEvent_t cam_up = nullptr;
    BlockDownload dl;                    // vet_tiling_render_host: blocks of B frames
};

static constexpr double kSin15 = 0.25881904510252074;      // sin(15 degrees): half of the 30-degree view angle
static constexpr size_t kTilingBlockBytes = (size_t)32 << 20;

// Camera of one frame (P, U, F) as include/vet.h defines it; false for dist == 0, d x U == 0 or a non-finite value.
static bool tiling_camera(const double* c9, int W, int H, TilingCam& o) {
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(c9[k])) return false;
    const double *P = c9, *U = c9 + 3, *F = c9 + 6;
    const double vx = P[0] - F[0], vy = P[1] - F[1], vz = P[2] - F[2];
    const double dist = std::sqrt(vx * vx + vy * vy + vz * vz);
    if (!(dist > 0.0)) return false;
    const double d[3] = {(F[0] - P[0]) / dist, (F[1] - P[1]) / dist, (F[2] - P[2]) / dist};
    const double x[3] = {d[1] * U[2] - d[2] * U[1], d[2] * U[0] - d[0] * U[2], d[0] * U[1] - d[1] * U[0]};
    const double xl = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    if (!(xl > 0.0)) return false;
    for (int k = 0; k < 3; ++k) { o.F[k] = F[k]; o.r[k] = x[k] / xl; o.nd[k] = -d[k]; }
    o.u[0] = o.r[1] * d[2] - o.r[2] * d[1];
    o.u[1] = o.r[2] * d[0] - o.r[0] * d[2];
    o.u[2] = o.r[0] * d[1] - o.r[1] * d[0];
    o.s = 2.0 * dist * kSin15 / (double)H;
    if (!(o.s > 0.0) || !std::isfinite(o.s)) return false;
    const double ox = 0.0 - F[0], oy = 0.0 - F[1], oz = 0.0 - F[2];
    o.X0 = (double)W / 2.0 + (ox * o.r[0] + oy * o.r[1] + oz * o.r[2]) / o.s;
    o.Y0 = (double)H / 2.0 - (ox * o.u[0] + oy * o.u[1] + oz * o.u[2]) / o.s;
    return true;
}

static uint32_t tiling_blend(uint32_t rgb) {                 // floor(0.3 * 128 + 0.7 x + 0.5) per channel
    uint32_t out = 0;
    for (int k = 0; k < 3; ++k) {
        const double x = (double)((rgb >> (8 * k)) & 0xFF);
        out |= (uint32_t)std::floor(0.3 * 128.0 + 0.7 * x + 0.5) << (8 * k);
    }
    return out;
}

// Checks the arguments of a render, computes its cameras and stages them on the device (stream-ordered on s).
static int tiling_begin(vet_tiling* tl, const double* h_cameras, int T, const uint8_t* bg, hipStream_t s) {
    std::vector<TilingCam> cams((size_t)T);
    for (int f = 0; f < T; ++f)
        if (!tiling_camera(h_cameras + 9 * (size_t)f, tl->g.W, tl->g.H, cams[f]))
            return fail(VET_ERR_INVALID, "camera %d: the position equals the focal point, the view-up is parallel to the view "
                                         "direction, or a value is not finite", f);
    const uint32_t base[3] = {(uint32_t)bg[0] | (uint32_t)bg[1] << 8 | (uint32_t)bg[2] << 16, 0x0000FFu, 0u};
    for (int k = 0; k < 3; ++k) { tl->g.colour[k] = base[k]; tl->g.colour[3 + k] = tiling_blend(base[k]); }
    HIP_TRY(hipSetDevice(tl->device));
    if (tl->cam_cap < T) {                                   // grow-only
        HIP_TRY(hipStreamSynchronize(s));                    // a pending render may still read them
        if (tl->cam_up) HIP_TRY(hipEventSynchronize(tl->cam_up));
        if (tl->h_cam) HIP_TRY(hipHostFree(tl->h_cam));
        if (tl->d_cam) HIP_TRY(hipFree(tl->d_cam));
        tl->h_cam = nullptr; tl->d_cam = nullptr; tl->cam_cap = 0;
        HIP_TRY(hipHostMalloc((void**)&tl->h_cam, (size_t)T * sizeof(TilingCam), hipHostMallocDefault));
        HIP_TRY(hipMalloc((void**)&tl->d_cam, (size_t)T * sizeof(TilingCam)));
        tl->cam_cap = T;
    }
    if (!tl->cam_up) HIP_TRY(hipEventCreateWithFlags(&tl->cam_up, hipEventDisableTiming));
    HIP_TRY(hipEventSynchronize(tl->cam_up));                // the previous upload has left the pinned copy
    std::memcpy(tl->h_cam, cams.data(), (size_t)T * sizeof(TilingCam));
    HIP_TRY(hipMemcpyAsync(tl->d_cam, tl->h_cam, (size_t)T * sizeof(TilingCam), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(tl->cam_up, s));
    return VET_OK;
}

int vet_tiling_create(vet_ctx* c, const double* h_arcs, int n_arcs, const double* h_centres, int n_centres, int W, int H,
                      vet_tiling** out) {
    if (!c || !h_arcs || !out) return fail(VET_ERR_INVALID, "ctx, arcs or out is NULL");
    *out = nullptr;
    if (n_arcs <= 0 || n_centres < 0 || W <= 0 || H <= 0)
        return fail(VET_ERR_INVALID, "need n_arcs, width, height > 0 and n_centres >= 0");
    if (n_centres > 0 && !h_centres) return fail(VET_ERR_INVALID, "n_centres is %d but centres is NULL", n_centres);
    if (W > 16384 || H > 16384) return fail(VET_ERR_INVALID, "frame of %d x %d pixels: at most 16384 each way", W, H);
    if (n_arcs > (1 << 22) || n_centres > (1 << 26))
        return fail(VET_ERR_INVALID, "too many arcs (%d, at most 2^22) or centres (%d, at most 2^26)", n_arcs, n_centres);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DevBuf arcs;
    HIP_TRY(arcs.alloc((size_t)n_arcs * 6 * sizeof(double)));
    TilingPtr tl(new vet_tiling());
    tl->ctx = c; tl->device = c->device;
    // render_tiling makes a tiling per call, so a copy stream would be created and destroyed per call, and a block's render
    // is short beside its download: with the second stream the 1001-tile orbit measured 2979 frames/s against 2996-3092
    // of the in-stream order (profiles/hostapi/host_path_ab.json)
    tl->dl.in_stream = true;
    tl->g.W = W; tl->g.H = H; tl->g.n_arcs = n_arcs; tl->g.n_centres = n_centres;
    const size_t frame = (size_t)W * H;
    tl->B = (int)std::min<size_t>(64, std::max<size_t>(4, kTilingBlockBytes / (frame * 3)) / 4 * 4);
    HIP_TRY(hipMalloc((void**)&tl->d_pts, (size_t)n_arcs * 50 * 3 * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&tl->d_flags, (size_t)tl->B * frame * 4));
    tl->g.d_pts = tl->d_pts;
    if (n_centres > 0) {
        HIP_TRY(hipMalloc((void**)&tl->d_centres, (size_t)n_centres * 3 * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(tl->d_centres, h_centres, (size_t)n_centres * 3 * sizeof(double), hipMemcpyHostToDevice, s));
        tl->g.d_centres = tl->d_centres;
    }
    HIP_TRY(hipMemcpyAsync(arcs.p, h_arcs, (size_t)n_arcs * 6 * sizeof(double), hipMemcpyHostToDevice, s));
    int rc = tiling_chords(c, (const double*)arcs.p, n_arcs, tl->d_pts, s);
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    HIP_TRY(hipStreamSynchronize(s));                        // 'arcs' goes out of scope; the caller's arrays are free
    *out = tl.release();
    return VET_OK;
}

int vet_tiling_destroy(vet_tiling* tl) {
    if (!tl) return VET_OK;
    (void)hipSetDevice(tl->device);
    if (tl->ctx) (void)hipStreamSynchronize(tl->ctx->stream);
    if (tl->cam_up) { (void)hipEventSynchronize(tl->cam_up); (void)hipEventDestroy(tl->cam_up); }
    tl->dl.release();
    if (tl->h_cam) (void)hipHostFree(tl->h_cam);
    if (tl->d_cam) (void)hipFree(tl->d_cam);
    if (tl->d_flags) (void)hipFree(tl->d_flags);
    if (tl->d_centres) (void)hipFree(tl->d_centres);
    if (tl->d_pts) (void)hipFree(tl->d_pts);
    delete tl;
    return VET_OK;
}

int vet_tiling_render(vet_tiling* tl, const double* h_cameras, int T, const uint8_t* background, uint8_t* d_rgb,
                      void* stream) {
    if (!tl || !h_cameras || !background || !d_rgb) return fail(VET_ERR_INVALID, "tiling, cameras, background or rgb is NULL");
    if (T <= 0) return fail(VET_ERR_INVALID, "n_frames must be > 0 (got %d)", T);
    if ((uintptr_t)d_rgb % 4) return fail(VET_ERR_INVALID, "d_rgb must be 4-byte aligned");
    hipStream_t s = stream ? (hipStream_t)stream : tl->ctx->stream;
    int rc = tiling_begin(tl, h_cameras, T, background, s);
    if (rc) return rc;
    const size_t frame = (size_t)tl->g.W * tl->g.H * 3;
    for (int f0 = 0; f0 < T; f0 += tl->B) {                  // B % 4 == 0: every block starts 4-byte aligned
        rc = tiling_render(tl->ctx, tl->g, tl->d_cam + f0, std::min(tl->B, T - f0), tl->d_flags, d_rgb + (size_t)f0 * frame, s);
        if (rc) return rc;
    }
    return VET_OK;
}

int vet_tiling_render_host(vet_tiling* tl, const double* h_cameras, int T, const uint8_t* background, uint8_t* h_rgb) {
    if (!tl || !h_cameras || !background || !h_rgb) return fail(VET_ERR_INVALID, "tiling, cameras, background or rgb is NULL");
    if (T <= 0) return fail(VET_ERR_INVALID, "n_frames must be > 0 (got %d)", T);
    hipStream_t s = tl->ctx->stream;
    int rc = tiling_begin(tl, h_cameras, T, background, s);
    if (rc) return rc;
    const int B = tl->B;
    const size_t frame = (size_t)tl->g.W * tl->g.H * 3;
    // d_flags is one block: block k + 1 clears it behind block k's compose, in stream order
    return tl->dl.run(s, (size_t)T * frame, (size_t)B * frame, h_rgb, [&](int64_t k, uint8_t* d_rgb) -> int {
        const int b = (int)std::min<int64_t>(B, T - k * B);
        return tiling_render(tl->ctx, tl->g, tl->d_cam + (size_t)k * B, b, tl->d_flags, d_rgb, s);
    });
}

}  // extern "C"
