// vet_window.hip — sliding-window spatial entropy behind vet_spatial_entropy_windowed* (include/vet.h): the kernels and
// their launch logic.  Row r pools the samples of frames [r * stride, r * stride + window) into ONE histogram per lattice
// and takes the reference's normalised entropy of it (compute_spatial_entropy on one dict that holds every sample of the
// window, utilities/entropy_utils.py:147-211), then the mean over the lattices (k_finalize).
// Two stages, every frame's histogram built once whatever the overlap of the windows:
//   1  per frame and lattice, in the context's workspace:
//        weighted Fibonacci lattices   [T][n_k] f64 tile sums: k_weights_gather over the lattice's exact FP64 weight rows
//                                      (vet_spatial.hip: exact_frame_rows), `dtable`'s sums bit for bit
//        unweighted / binned lattices  [T][U] i32 tile of every sample, -1 absent (k_window_tiles)
//        present samples per frame [T] and the range status word (k_window_tiles)
//   2  k_window_entropy_w / k_window_entropy_c: the window's histogram in LDS and the reference's epilogue over it.
// A row is a pure function of the plan and of its frames' samples: the FP64 sums are re-added from the window's first frame
// in ascending frame order for every row (never a running sum with subtractions), the integer counts are exact under add
// and subtract, and every reduction runs in one wave in fixed lane order.
// The same unit holds the sliding-window TRANSITION entropy behind vet_transition_entropy_windowed*: stage 1 is k_window_tiles
// again (every sample quantised and looked up once), stage 2 is k_window_transition below.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_finalize.hpp"
#include "vet_transition.hpp"
#include "vet_window_hist.hpp"
#include "vet_row_hist.hpp"

#include <algorithm>

namespace vet {

// ------------------------------------------------------------------------------------------
// k_window_tiles — stage 1 of the integer-count lattices and the per-frame bookkeeping of every plan: one wave per frame;
// tiles[f][u] = nearest tile / bin of the sample (LUT gather), -1 absent; present[f] = samples of the frame; status[0] is
// raised by samples outside [0, 1] (ids: at or beyond the direction table) exactly as vet_spatial_entropy raises it.
// ------------------------------------------------------------------------------------------
struct WindowTilesParams {
    SampleSrc src;
    int U, T;
    const uint16_t* nearest;     // [n_dirs] direction -> tile / bin of this lattice, or null (bookkeeping only)
    int32_t* tiles;              // [T][U] or null
    int32_t* present;            // [T] or null
    int32_t* status;             // [2] or null
};

template <bool FROM_IDS>
__global__ __launch_bounds__(256) void k_window_tiles(const WindowTilesParams p) {
    const int lane = lane_id();
    const long f = (long)blockIdx.x * (blockDim.x >> 6) + wave_id();
    bool bad = false;
    if (f < p.T) {
        int np = 0;
        for (int u = lane; u < p.U; u += WAVE) {
            const long idx = f * (long)p.U + u;
            const int id = sample_dir<FROM_IDS>(p.src, idx, bad);
            if (p.tiles) p.tiles[idx] = id >= 0 ? (int)p.nearest[id] : -1;
            np += id >= 0 ? 1 : 0;
        }
        np = wave_sum(np);
        if (lane == 0 && p.present) p.present[f] = np;
    }
    if (p.status) {
        const unsigned long long anybad = __ballot(bad);
        if (anybad && lane == 0) atomicAdd(&p.status[0], (int)__popcll(anybad));
    }
}

// ------------------------------------------------------------------------------------------
// k_window_entropy_w — stage 2 of a weighted Fibonacci lattice.  One wave per row, NW rows per workgroup, no barriers.
// hist[f][t] is the dense tile_weights encoding of frame f (include/vet.h): -0.0 = key of the reference's dict with the
// value 0.0, +0.0 = no key.  Tile t of the row = the window's frames added in ascending frame order onto "no key" (-0.0):
// a frame without the key adds -0.0 (no change), a zero-valued key adds +0.0 (-0.0 + +0.0 = +0.0: key with the value 0.0),
// so one frame (window = 1) gives back k_spatial_dtable's own LDS value.  Lane l owns tiles l, l + 64, ...: the loads of a
// frame row are coalesced, four frames are in flight per tile, and a frame row is read from L2 by the window / stride rows
// that share it (window_row_w, vet_window_hist.hpp, shared with k_window_hist_w).  The epilogue is k_spatial_dtable's:
// row_entropy (vet_row_hist.hpp) over the keys, / hmax; NaN for a window without a sample (and status[1] += 1).
// LDS: f64 [NW][n] (a wave reads back only what its own lanes wrote).
// ------------------------------------------------------------------------------------------
struct WindowWParams {
    const double* hist;          // [T][n]
    const int32_t* present;      // [T]
    int n;
    double hmax;
    int window, stride;
    long R;
    double* ent;                 // [R]
    double* weights;             // [R][n] or null
    int32_t* samples;            // [R] or null
    int32_t* status;             // [2] or null
};

__global__ __launch_bounds__(256) void k_window_entropy_w(const WindowWParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int NW = blockDim.x >> 6, lane = lane_id(), wv = wave_id();
    const long r = (long)blockIdx.x * NW + wv;
    if (r >= p.R) return;
    double* h = (double*)smem + (size_t)wv * p.n;
    const long f0 = r * (long)p.stride;
    double tot;
    const int np = window_row_w(h, p.hist, p.present, p.n, p.window, f0, tot, [&](int t, double acc, bool key) {
        if (p.weights) __builtin_nontemporal_store(key ? (acc == 0.0 ? -0.0 : acc) : 0.0, p.weights + r * (long)p.n + t);
    });
    const double hh = row_entropy(p.n, tot, KeyedHist{h, WIN_NO_KEY_BITS});
    if (lane == 0) {
        p.ent[r] = np == 0 ? __builtin_nan("") : hh / p.hmax;
        if (p.samples) p.samples[r] = np;
        if (p.status && np == 0) atomicAdd(&p.status[1], 1);
    }
}

// ------------------------------------------------------------------------------------------
// k_window_entropy_c — stage 2 of an integer-count lattice (unweighted nearest tile, naive lat/lon bins).  One wave per
// workgroup owns rows [blockIdx * rpw, + rpw): the window's counts live in LDS; the first row adds its `window` frames, every
// later row (stride < window; the host gives rpw = 1 otherwise) subtracts the `stride` frames that leave and adds the
// `stride` frames that enter — integers, exact in any order.  The epilogue is count_row_entropy (vet_row_hist.hpp), shared with
// k_user_entropy_c: NaN and status[1] += 1 for an empty window.
// LDS: u32 [n].
// ------------------------------------------------------------------------------------------
struct WindowCParams {
    const int32_t* tiles;        // [T][U]
    int U, n;
    double hmax;
    int norm_n, full_norm;
    int window, stride, rpw;
    long R;
    double* ent;                 // [R]
    double* weights;             // [R][n] or null
    int32_t* samples;            // [R] or null
    int32_t* status;             // [2] or null
};

__global__ __launch_bounds__(64) void k_window_entropy_c(const WindowCParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* cnt = (unsigned*)smem;
    const int lane = lane_id();
    for (int t = lane; t < p.n; t += WAVE) cnt[t] = 0u;
    __syncthreads();
    const long r0 = (long)blockIdx.x * p.rpw, r1 = min(p.R, r0 + (long)p.rpw);
    for (long r = r0; r < r1; ++r) {
        const long f0 = r * (long)p.stride;
        if (r == r0) {
            window_count(cnt, p.n, p.tiles, p.U, f0, f0 + p.window, 1u);
        } else {
            window_count(cnt, p.n, p.tiles, p.U, f0 - p.stride, f0, ~0u);                              // - 1 (mod 2^32)
            window_count(cnt, p.n, p.tiles, p.U, f0 - p.stride + p.window, f0 + p.window, 1u);
        }
        __syncthreads();
        count_row_entropy(cnt, p, r);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// k_window_transition — stage 2 of the windowed transition entropy: compute_transition_entropy (entropy_utils.py:213-332) on
// the pooled (pair, user) samples of frame pairs [r * stride, r * stride + window), pair-major then user order, per row r.
// tiles[T][U] is k_window_tiles' output for this lattice, so the pooled samples of a row are a CONTIGUOUS slice of it:
// sample q in [0, window * U) has the source tile tiles[f0 * U + q] and the destination tile tiles[f0 * U + q + U],
// f0 = r * stride, and is pooled when both are >= 0.  With "user index" = q the row algorithm is k_transition_big's,
// device code shared (vet_transition.hpp: trans_big_clear / trans_big_count / trans_big_finish): per-tile words and the
// bucket hash in LDS, source tiles cut into passes where sum min(m, n) exceeds the hash.
// Every row is computed from scratch.  There is NO running add / subtract across overlapping rows: K and w of a source
// tile depend on which sample of the window is the tile's first and on the order of first appearance of its destinations,
// so a frame that leaves changes the roles of the samples that stay — the statistic is not decomposable over frames.
// Persistent workgroups take rows blockIdx, blockIdx + gridDim, ...  Workgroup and hash are sized by the pooled samples
// W = window * U alone (never by the stride, the row count or the device), so a row's bits are a pure function of the
// plan and its window + 1 frames:
//   W <= 256: 64 threads, 512 slots | W <= 1024: 256 threads, 2048 slots | W <= 2048: 256 threads, 4096 slots — the hash
//   holds every sample (2 W <= slots: one pass) and the packed pairs stay in LDS behind the hash;
//   else 1024 threads, 8192 slots, passes by k_transition_big's bound, packed pairs in a per-workgroup global slice.
// Integer atomics only; the FP64 cell sum per thread in tile order, wave_sum's butterfly, the waves in order.
// LDS: trans_big_lds_bytes(n, slots) | pc u32 [W4] (the three small shapes)
// ------------------------------------------------------------------------------------------
struct WindowTransParams {
    const int32_t* tiles;        // [T][U]
    int U, n;
    double hmax;
    int window, stride;
    long R;
    double* ent;                 // [R]
    int32_t* srccount;           // [R][n] or null
    int32_t* samples;            // [R] or null
    int32_t* status;             // [2] or null
    const double* log2_tab;      // [4097] log2(k)
    uint32_t* scratch;           // 1024-thread shape: per-workgroup slices of W4 words
};

template <int BD, int LG>
__global__ __launch_bounds__(BD) void k_window_transition(const WindowTransParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int HS = 1 << LG;
    constexpr bool SMALL = LG < 13;
    const TransBigLds L = trans_big_carve(smem, p.n, HS);
    const int tid = threadIdx.x;
    const int W = p.window * p.U;
    const size_t W4 = ((size_t)W + 3) & ~(size_t)3;
    unsigned* pc = SMALL ? (unsigned*)(smem + trans_big_lds_bytes(p.n, HS)) : p.scratch + (size_t)blockIdx.x * W4;
    const int cap = SMALL ? 0x7FFFFFFF : HS * 6 / 10 - p.n;
    const bool tab = W <= 4096;
    int parity = 0;
    for (long r = blockIdx.x; r < p.R; r += gridDim.x, parity ^= 1) {
        double* acc = L.acc2 + TRANS_ACC * parity;
        trans_big_clear<BD>(L, acc);
        __syncthreads();
        const int32_t* src = p.tiles + r * (long)p.stride * p.U;
        for (int q = tid; q < W; q += BD) pc[q] = trans_big_count(L, acc, (unsigned)q, src[q], src[q + p.U]);
        __syncthreads();
        trans_big_finish<BD, LG>(L, pc, W, p.n, cap, tab, p.log2_tab, p.hmax, acc, r, p.ent, p.srccount, p.samples, p.status);
    }
}

}  // namespace vet

namespace vh {

namespace {

// one launch of k_window_tiles<src.ids given> over frames [0, T), charged to k_spatial: tiles [T][U] through `nearest`, present [T]
// and status[0], each where given
int window_tiles_run(vet_ctx* c, const vet::SampleSrc& src, int U, int T, const uint16_t* nearest, int32_t* tiles, int32_t* present,
                     int32_t* d_status, hipStream_t s) {
    const int frames_per_wg = 4;
    const dim3 grid((unsigned)((T + frames_per_wg - 1) / frames_per_wg)), block(frames_per_wg * vet::WAVE);
    vet::WindowTilesParams q{};
    q.src = src; q.U = U; q.T = T;
    q.nearest = nearest; q.tiles = tiles; q.present = present; q.status = d_status;
    ProfScope ps(c, s, KID_SPATIAL);
    if (src.ids) hipLaunchKernelGGL(vet::k_window_tiles<true>, grid, block, 0, s, q);
    else hipLaunchKernelGGL(vet::k_window_tiles<false>, grid, block, 0, s, q);
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

int launch_windowed(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window,
                    int stride, double* d_entropy, double* d_weights, int32_t* d_samples, int32_t* d_status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const int K = (int)pl->lat.size();
    const long R = (long)vet_window_rows(T, window, stride);
    // ---- what stage 1 leaves per lattice, and whether this plan can run windowed at all
    WindowFrames wf;
    int rc = window_frames_layout(pl, U, T, pad16(K > 1 ? (size_t)K * R * sizeof(double) : 0), wf, s);
    if (rc) return rc;
    rc = ensure_ws(c, wf.bytes);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    const size_t* off = wf.off;
    int32_t* d_frame_present = (int32_t*)(ws + wf.present_off);
    double* ent_k = K > 1 ? (double*)ws : d_entropy;
    // ---- stage 1
    rc = window_frames_run(pl, d_mu, d_mv, d_ids, U, T, wf, d_status, s);
    if (rc) return rc;
    // ---- stage 2, charged to the k_finalize scope (include/vet.h)
    for (int k = 0; k < K; ++k) {
        const Lattice& L = pl->lat[k];
        ProfScope ps(c, s, KID_FINALIZE);
        if (counts_lattice(pl, k)) {
            vet::WindowCParams q{};
            q.tiles = (const int32_t*)(ws + off[k]); q.U = U; q.n = L.n; q.hmax = L.hmax;
            q.norm_n = L.norm_n; q.full_norm = (L.binned && pl->weighted) ? 1 : 0;
            q.window = window; q.stride = stride; q.R = R;
            // overlapping windows: a run of rows per wave, at least ~8 waves per CU in the launch
            q.rpw = stride < window ? (int)std::min<long>(64, std::max<long>(1, R / (8L * c->n_cu))) : 1;
            q.ent = ent_k + (size_t)k * R;
            q.weights = k == 0 ? d_weights : nullptr; q.samples = k == 0 ? d_samples : nullptr; q.status = k == 0 ? d_status : nullptr;
            const long grid = (R + q.rpw - 1) / q.rpw;
            hipLaunchKernelGGL(vet::k_window_entropy_c, dim3((unsigned)grid), dim3(vet::WAVE), (size_t)L.n * 4, s, q);
        } else {
            vet::WindowWParams q{};
            q.hist = (const double*)(ws + off[k]); q.present = d_frame_present; q.n = L.n; q.hmax = L.hmax;
            q.window = window; q.stride = stride; q.R = R;
            q.ent = ent_k + (size_t)k * R;
            q.weights = k == 0 ? d_weights : nullptr; q.samples = k == 0 ? d_samples : nullptr; q.status = k == 0 ? d_status : nullptr;
            int nw = 4;
            while (nw > 1 && (size_t)nw * L.n * 8 > 32 * 1024) nw /= 2;
            const size_t lds = (size_t)nw * L.n * 8;
            if (lds > c->lds_max) return fail(VET_ERR_UNSUPPORTED, "windowed: lattice of %d tiles does not fit the LDS", L.n);
            hipLaunchKernelGGL(vet::k_window_entropy_w, dim3((unsigned)((R + nw - 1) / nw)), dim3(nw * vet::WAVE), lds, s, q);
        }
        HIP_TRY(hipGetLastError());
    }
    if (K > 1) {
        ProfScope ps(c, s, KID_FINALIZE);
        hipLaunchKernelGGL(vet::k_finalize, dim3(grid_for(R, 256, c->n_cu)), dim3(256), 0, s, (const double*)ent_k, K, R, d_entropy);
        HIP_TRY(hipGetLastError());
    }
    return VET_OK;
}

// ---- windowed transition entropy
// Shape of k_window_transition for W pooled samples per row (the kernel's header): a function of W alone
struct WindowTransShape { int threads, lg; const void* fn; };
WindowTransShape window_trans_shape(long W) {
    if (W <= 256) return {64, 9, (const void*)vet::k_window_transition<64, 9>};
    if (W <= 1024) return {256, 11, (const void*)vet::k_window_transition<256, 11>};
    if (W <= 2048) return {256, 12, (const void*)vet::k_window_transition<256, 12>};
    return {vet::TRANS_BIG_THREADS, 13, (const void*)vet::k_window_transition<vet::TRANS_BIG_THREADS, 13>};
}
size_t window_trans_lds(const WindowTransShape& g, int n, long W) {
    return vet::trans_big_lds_bytes(n, 1 << g.lg) + (g.lg < 13 ? (size_t)((W + 3) & ~3L) * 4 : 0);
}

int check_window_trans_args(const vet_plan* pl, int U, int T, int window, int stride, const void* out) {
    int rc = check_run_args(pl, U, T, out);
    if (rc) return rc;
    if (T < 2) return fail(VET_ERR_INVALID, "windowed transition entropy needs at least two frames (got %d)", T);
    if (window < 1) return fail(VET_ERR_INVALID, "window must be at least 1 frame pair (got %d)", window);
    if (stride < 1) return fail(VET_ERR_INVALID, "stride must be at least 1 frame pair (got %d)", stride);
    if (window > T - 1)
        return fail(VET_ERR_INVALID, "window of %d frame pairs is longer than the video's %d frame pairs", window, T - 1);
    // the kernel's packing, before anything is allocated or launched
    if ((long)window * U >= (1L << 19))
        return fail(VET_ERR_UNSUPPORTED, "windowed transition: window * n_users = %ld pooled samples per row, the kernel packs "
                    "fewer than 2^19", (long)window * U);
    for (const auto& L : pl->lat)
        if (L.n > vet::TRANS_BIG_MAX_TILES)
            return fail(VET_ERR_UNSUPPORTED, "windowed transition: lattice of %d tiles (at most %d)", L.n, vet::TRANS_BIG_MAX_TILES);
    return VET_OK;
}

int launch_window_transition(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window,
                             int stride, double* d_entropy, int32_t* d_srccount, int32_t* d_samples, int32_t* d_status,
                             hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const int K = (int)pl->lat.size();
    const long R = (long)vet_window_rows(T - 1, window, stride), W = (long)window * U;
    const vet::SampleSrc src{d_mu, d_mv, d_ids, pl->W, pl->H, (long)pl->n_dirs};
    const WindowTransShape g = window_trans_shape(W);
    // persistent workgroups: as many as LDS and wave slots let run at once, at most one per row
    size_t lds_most = 0;
    for (const auto& L : pl->lat) lds_most = std::max(lds_most, window_trans_lds(g, L.n, W));
    if (lds_most > kWholeLds) return fail(VET_ERR_UNSUPPORTED, "windowed transition: %zu B of LDS (max %zu)", lds_most, kWholeLds);
    long per_cu = std::min<long>({(long)(kWholeLds / lds_most), 32 / (g.threads / vet::WAVE), 16});
    const long grid = std::max<long>(1, std::min<long>(R, (long)c->n_cu * per_cu));
    // workspace: per-lattice rows (K > 1) | one lattice's tiles [T][U], reused lattice after lattice on the stream | the
    // packed pairs of the 1024-thread shape
    WsLayout lay;
    const size_t ent_o = lay.take<double>(K > 1 ? (size_t)K * R : 0), tiles_o = lay.take<int32_t>((size_t)T * U),
                 pc_o = lay.take<uint32_t>(g.lg < 13 ? 0 : (size_t)grid * ((W + 3) & ~3L));
    int rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    double* ent_k = K > 1 ? (double*)(ws + ent_o) : d_entropy;
    int32_t* tiles = (int32_t*)(ws + tiles_o);
    for (int k = 0; k < K; ++k) {
        const Lattice& L = pl->lat[k];
        // stage 1, as in the spatial windowed call
        rc = window_tiles_run(c, src, U, T, L.d_nearest, tiles, nullptr, k == 0 ? d_status : nullptr, s);
        if (rc) return rc;
        vet::WindowTransParams q{};
        q.tiles = tiles; q.U = U; q.n = L.n; q.hmax = L.hmax;
        q.window = window; q.stride = stride; q.R = R;
        q.ent = ent_k + (size_t)k * R;
        q.srccount = k == 0 ? d_srccount : nullptr; q.samples = k == 0 ? d_samples : nullptr; q.status = k == 0 ? d_status : nullptr;
        q.log2_tab = c->d_log2;
        q.scratch = (uint32_t*)(ws + pc_o);
        ProfScope ps(c, s, KID_TRANSITION);
        void* args[] = {(void*)&q};
        HIP_TRY(hipLaunchKernel(g.fn, dim3((unsigned)grid), dim3(g.threads), args, window_trans_lds(g, L.n, W), s));
        HIP_TRY(hipGetLastError());
    }
    if (K > 1) {
        ProfScope ps(c, s, KID_FINALIZE);
        hipLaunchKernelGGL(vet::k_finalize, dim3(grid_for(R, 256, c->n_cu)), dim3(256), 0, s, (const double*)ent_k, K, R, d_entropy);
        HIP_TRY(hipGetLastError());
    }
    return VET_OK;
}

}  // namespace

// ---- stage 1 of the windowed spatial calls, shared with vet_window_divergence.hip (vet_host.hpp)
int window_frames_layout(vet_plan* pl, int U, int T, size_t head_bytes, WindowFrames& wf, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const int K = (int)pl->lat.size();
    if (K > 64) return fail(VET_ERR_UNSUPPORTED, "more than 64 lattices in one plan");
    WsLayout lay{head_bytes};
    wf.present_off = lay.take<int32_t>((size_t)T);
    for (int k = 0; k < K; ++k) {
        const Lattice& L = pl->lat[k];
        if (counts_lattice(pl, k)) {
            if ((size_t)L.n * 4 > c->lds_max)
                return fail(VET_ERR_UNSUPPORTED, "windowed: %d bins do not fit the LDS histogram of a window (at most %zu)", L.n,
                            c->lds_max / 4);
            wf.off[k] = lay.take<int32_t>((size_t)T * U);
        } else {
            int rc = ensure_exact_rows(pl, k, s);
            if (rc) return rc;
            if (exact_rows(pl, k).state != 1)
                return fail(VET_ERR_UNSUPPORTED, "windowed: the exact FP64 weight rows of lattice %d are not on the device "
                            "(too large for it); the windowed call has no other formulation", k);
            wf.off[k] = lay.take<double>((size_t)T * L.n);
        }
    }
    wf.bytes = lay.at;
    return VET_OK;
}

int window_frames_run(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T,
                      const WindowFrames& wf, int32_t* d_status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const vet::SampleSrc src{d_mu, d_mv, d_ids, pl->W, pl->H, (long)pl->n_dirs};
    const int K = (int)pl->lat.size();
    char* ws = (char*)c->ws;
    // the counting lattices' tiles; the first launch (one without tiles if there is no such lattice) books present and status
    bool booked = false;
    for (int k = 0; k < K || !booked; ++k) {
        if (k < K && !counts_lattice(pl, k)) continue;
        int rc = window_tiles_run(c, src, U, T, k < K ? pl->lat[k].d_nearest : nullptr, k < K ? (int32_t*)(ws + wf.off[k]) : nullptr,
                                  booked ? nullptr : (int32_t*)(ws + wf.present_off), booked ? nullptr : d_status, s);
        if (rc) return rc;
        booked = true;
    }
    for (int k = 0; k < K; ++k) {
        if (counts_lattice(pl, k)) continue;
        int rc = exact_frame_rows(pl, k, d_mu, d_mv, d_ids, U, T, (double*)(ws + wf.off[k]), s);
        if (rc) return rc;
    }
    return VET_OK;
}

int window_tiles_lattice(vet_plan* pl, int k, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int32_t* tiles,
                         int32_t* d_status, hipStream_t s) {
    const vet::SampleSrc src{d_mu, d_mv, d_ids, pl->W, pl->H, (long)pl->n_dirs};
    return window_tiles_run(pl->ctx, src, U, T, pl->lat[k].d_nearest, tiles, nullptr, d_status, s);
}

int check_window_args(const vet_plan* pl, int U, int T, int window, int stride, const void* out) {
    int rc = check_run_args(pl, U, T, out);
    if (rc) return rc;
    if (window < 1) return fail(VET_ERR_INVALID, "window must be at least 1 frame (got %d)", window);
    if (stride < 1) return fail(VET_ERR_INVALID, "stride must be at least 1 frame (got %d)", stride);
    if (window > T) return fail(VET_ERR_INVALID, "window of %d frames is longer than the video's %d frames", window, T);
    return VET_OK;
}

int window_set_attrs(vet_ctx* c) {
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_window_entropy_w, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_max));
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_window_entropy_c, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_max));
    for (long W : {1L, 257L, 1025L, 2049L})
        HIP_TRY(hipFuncSetAttribute(window_trans_shape(W).fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWholeLds));
    return VET_OK;
}

}  // namespace vh

using namespace vh;

extern "C" {

int64_t vet_window_rows(int n_frames, int window, int stride) {
    if (n_frames < 1 || window < 1 || stride < 1 || window > n_frames) return VET_ERR_INVALID;
    return ((int64_t)n_frames - window) / stride + 1;
}

int vet_spatial_entropy_windowed(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride,
                                 double* d_entropy, double* d_weights, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_args(pl, U, T, window, stride, d_entropy);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_spatial_entropy_windowed_ids", stream, &s);
    return rc ? rc : launch_windowed(pl, d_mu, d_mv, nullptr, U, T, window, stride, d_entropy, d_weights, d_samples, d_status, s);
}

int vet_spatial_entropy_windowed_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride,
                                     double* d_entropy, double* d_weights, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_args(pl, U, T, window, stride, d_entropy);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_windowed(pl, nullptr, nullptr, d_ids, U, T, window, stride, d_entropy, d_weights, d_samples, d_status, s);
}

int vet_transition_entropy_windowed(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride,
                                    double* d_entropy, int32_t* d_srccount, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_trans_args(pl, U, T, window, stride, d_entropy);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_transition_entropy_windowed_ids", stream, &s);
    return rc ? rc : launch_window_transition(pl, d_mu, d_mv, nullptr, U, T, window, stride, d_entropy, d_srccount, d_samples, d_status, s);
}

int vet_transition_entropy_windowed_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride,
                                        double* d_entropy, int32_t* d_srccount, int32_t* d_samples, int32_t* d_status,
                                        void* stream) {
    hipStream_t s;
    int rc = check_window_trans_args(pl, U, T, window, stride, d_entropy);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_window_transition(pl, nullptr, nullptr, d_ids, U, T, window, stride, d_entropy, d_srccount, d_samples, d_status, s);
}

}  // extern "C"
