// vet_user.hip — per-viewer spatial entropy behind vet_user_entropy* (include/vet.h): the kernels and their launch logic.
// Row (u, r) pools the present samples of ONE user over frames [r * stride, r * stride + window) into one histogram per
// lattice and takes the reference's normalised entropy of it (compute_spatial_entropy on one dict that holds those samples in
// ascending frame order, utilities/entropy_utils.py:147-211; naive plans: compute_naive_spatial_entropy), then the mean over
// the lattices (k_finalize).  The transposed question of vet_window.hip: a histogram per user over time, not per frame over
// the users.
// Two stages:
//   1  k_user_dirs: every sample quantised once, its direction id written TRANSPOSED, dirs[U][T] i32 (-1 absent), through a
//      64 x 64 LDS tile — the samples lie [T][U], and a per-user walk over that layout would touch one value per cache line;
//   2  per (user, row) and lattice, over the contiguous slice dirs[u][r * stride ..]:
//        weighted Fibonacci lattices   k_user_entropy_w: the exact FP64 weight rows of the row's frames added in ascending
//                                      frame order (add_exact_rows, waves_in_order), `dtable`'s epilogue in one wave
//        unweighted / binned lattices  k_user_entropy_c: u32 counts in LDS, a wave slides over a run of rows of one user,
//                                      k_window_entropy_c's epilogue
// A row is a pure function of the plan and of its own samples: the FP64 sums are taken from scratch for every row with a wave
// split that depends on `window` alone, the integer counts are exact under add and subtract, and every reduction runs in one
// wave in fixed lane order.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_finalize.hpp"
#include "vet_spatial_dtable.hpp"
#include "vet_user_dirs.hpp"

#include <algorithm>

namespace vet {

// ------------------------------------------------------------------------------------------
// k_user_entropy_w — stage 2 of a weighted Fibonacci lattice.  One workgroup per (user, row), blockIdx = u * R + r.  Wave w
// takes the w-th contiguous share of the row's frames in ascending order; a 64-frame chunk is one coalesced load of 64
// consecutive ids of dirs[u], alias[id], and add_exact_rows into the wave's own LDS histogram (initialised to "no key"): the
// frames of a chunk are added in lane = frame order, the waves' histograms in wave order (waves_in_order).  Every row is
// summed from scratch.  The epilogue is k_spatial_dtable's for one lattice: total and -sum q log2 q over the keys in lane
// order in wave 0, wave_sum's butterfly, / hmax; NaN (and status[1] += 1) for a row without a sample.
// blockDim (NW waves) is chosen by the host from `window` (and the lattice's LDS footprint) alone.
// LDS: dtable_lds_bytes(NW, n): hist f64 [NW][n], present counts i32 [NW].
// S: 64-entry chunks of the lattice's longest exact row (1, 2, 4; 0 = any number), as k_weights_gather.
// ------------------------------------------------------------------------------------------
struct UserWParams {
    const int32_t* dirs;         // [U][T]
    int T;
    const uint32_t* alias;       // [n_dirs] direction -> row | mirrored << 31
    ExactRows X;
    double hmax;
    int window, stride;
    long R;                      // rows per user
    double* ent;                 // [U][R]
    double* weights;             // [U][R][n] or null
    int32_t* samples;            // [U][R] or null
    int32_t* status;             // [2] or null
};

template <int S>
__global__ __launch_bounds__(256) void k_user_entropy_w(const UserWParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* hist = (double*)smem;                                  // [NW][n]
    const int NW = blockDim.x >> 6, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int n = p.X.n;
    int* cnt_w = (int*)(hist + (size_t)NW * n);                    // [NW] present samples per wave
    const long row = blockIdx.x, u = row / p.R, r = row - u * p.R;
    const int32_t* d = p.dirs + u * (long)p.T + r * (long)p.stride;
    double* h = hist + (size_t)wv * n;
    for (int t = lane; t < n; t += WAVE) ((unsigned long long*)h)[t] = NO_KEY_BITS;
    const int per = (p.window + NW - 1) / NW;
    const int j_begin = min(p.window, wv * per), j_end = min(p.window, j_begin + per);
    int np = 0;
    for (int j0 = j_begin; j0 < j_end; j0 += WAVE) {
        const int j = j0 + lane;
        const int id = j < j_end ? d[j] : -1;
        const uint32_t a = id >= 0 ? p.alias[id] : 0u;
        add_exact_rows<S>(h, p.X, (int)(a & 0x7FFFFFFFu), (int)(a >> 31), id >= 0, min(WAVE, j_end - j0));
        np += id >= 0 ? 1 : 0;
    }
    np = wave_sum(np);
    if (lane == 0) cnt_w[wv] = np;
    __syncthreads();
    // tile values, wave order, into wave 0's share (every slot is read and written by one thread only)
    for (int t = tid; t < n; t += blockDim.x) {
        const double v = waves_in_order(hist, NW, n, t);
        hist[t] = v;
        if (p.weights) __builtin_nontemporal_store(weights_out(v), p.weights + row * (long)n + t);
    }
    int n_present = 0;
    for (int w2 = 0; w2 < NW; ++w2) n_present += cnt_w[w2];
    __syncthreads();
    if (wv != 0) return;
    double tot = 0.0;
    for (int t = lane; t < n; t += WAVE) {
        const double v = hist[t];
        if ((unsigned long long)__double_as_longlong(v) != NO_KEY_BITS) tot += v;
    }
    tot = wave_sum(tot);
    double hh = 0.0;
    for (int t = lane; t < n; t += WAVE) {
        const double v = hist[t];
        if ((unsigned long long)__double_as_longlong(v) != NO_KEY_BITS) {
            const double q = v / tot;
            hh -= q * log2(q);
        }
    }
    hh = wave_sum(hh);
    if (lane == 0) {
        p.ent[row] = n_present == 0 ? __builtin_nan("") : hh / p.hmax;
        if (p.samples) p.samples[row] = n_present;
        if (p.status && n_present == 0) atomicAdd(&p.status[1], 1);
    }
}

// ------------------------------------------------------------------------------------------
// k_user_entropy_c — stage 2 of an integer-count lattice (unweighted nearest tile, naive lat/lon bins).  One wave per
// workgroup owns rows [c * rpw, + rpw) of user u, blockIdx = u * chunks + c: the row's counts live in LDS; the first row adds
// its `window` frames, every later row (stride < window; the host gives rpw = 1 otherwise) subtracts the `stride` frames
// that leave and adds the `stride` frames that enter — k_window_entropy_c's scheme on a contiguous slice of dirs[u], the
// tile taken from the lattice's nearest[id].  Integers, exact in any order.  The epilogue restates k_window_entropy_c's
// operation for operation: samples = histogram total, h -= (v / N) * (log2 v - log2 N) in lane order, the normaliser log2(n)
// if full_norm or N > norm_n, else log2(N) (entropy_utils.py:201-206; one sample gives the reference's 0 / 0), NaN and
// status[1] += 1 for an empty row.
// LDS: u32 [n].
// ------------------------------------------------------------------------------------------
struct UserCParams {
    const int32_t* dirs;         // [U][T]
    int T;
    const uint16_t* nearest;     // [n_dirs] direction -> tile / bin
    int n;
    double hmax;
    int norm_n, full_norm;
    int window, stride, rpw;
    long R, chunks;              // rows per user, workgroups per user
    double* ent;                 // [U][R]
    double* weights;             // [U][R][n] or null
    int32_t* samples;            // [U][R] or null
    int32_t* status;             // [2] or null
};

__global__ __launch_bounds__(64) void k_user_entropy_c(const UserCParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* cnt = (unsigned*)smem;
    const int lane = lane_id();
    for (int t = lane; t < p.n; t += WAVE) cnt[t] = 0u;
    __syncthreads();
    const long u = blockIdx.x / p.chunks, c = blockIdx.x - u * p.chunks;
    const int32_t* d = p.dirs + u * (long)p.T;
    const long r0 = c * p.rpw, r1 = min(p.R, r0 + (long)p.rpw);
    for (long r = r0; r < r1; ++r) {
        const long f0 = r * (long)p.stride, row = u * p.R + r;
        if (r == r0) {
            user_count(cnt, p.n, d, p.nearest, f0, f0 + p.window, 1u);
        } else {
            user_count(cnt, p.n, d, p.nearest, f0 - p.stride, f0, ~0u);                                // - 1 (mod 2^32)
            user_count(cnt, p.n, d, p.nearest, f0 - p.stride + p.window, f0 + p.window, 1u);
        }
        __syncthreads();
        int np = 0;
        for (int t = lane; t < p.n; t += WAVE) np += (int)cnt[t];
        np = wave_sum(np);
        const double tw = (double)np, lgn = np ? log2(tw) : 0.0, inv_tw = 1.0 / tw;
        double h = 0.0;
        for (int t = lane; t < p.n; t += WAVE) {
            const unsigned v = cnt[t];
            if (v) h -= ((double)v * inv_tw) * (log2((double)v) - lgn);
            if (p.weights) __builtin_nontemporal_store((double)v, p.weights + row * (long)p.n + t);
        }
        h = wave_sum(h);
        if (lane == 0) {
            double hmax = p.hmax;
            if (!(tw > (double)p.norm_n) && !p.full_norm) hmax = -tw * (1.0 / tw) * -lgn;
            double e = h / hmax;
            if (np == 0) {
                e = __builtin_nan("");
                if (p.status) atomicAdd(&p.status[1], 1);
            }
            p.ent[row] = e;
            if (p.samples) p.samples[row] = np;
        }
        __syncthreads();
    }
}

}  // namespace vet

namespace vh {

// (declared in vet_host.hpp: vet_user_divergence.hip builds the same histograms)
bool counts_lattice(const vet_plan* pl, int k) { return !pl->weighted || pl->lat[k].binned; }

// waves per (user, row) workgroup of k_user_entropy_w: one per 64 frames of the window up to 4, fewer where the lattice's
// FP64 histograms would not fit the LDS — a function of `window` and the plan, never of stride, rows, users
int user_nw(size_t lds_max, int n, int window) {
    int nw = window <= vet::WAVE ? 1 : window <= 2 * vet::WAVE ? 2 : 4;
    while (nw > 1 && vet::dtable_lds_bytes(nw, n) > lds_max) nw /= 2;
    return nw;
}

// whether this plan can run per user at all (before anything is launched); `what` names the call in the message
int check_user_plan(vet_plan* pl, const char* what, hipStream_t s) {
    const vet_ctx* c = pl->ctx;
    for (int k = 0; k < (int)pl->lat.size(); ++k) {
        const Lattice& L = pl->lat[k];
        if (counts_lattice(pl, k)) {
            if ((size_t)L.n * 4 > c->lds_max)
                return fail(VET_ERR_UNSUPPORTED, "%s: %d bins do not fit the LDS histogram of a row (at most %zu)", what, L.n,
                            c->lds_max / 4);
        } else {
            int rc = ensure_exact_rows(pl, k, s);
            if (rc) return rc;
            if (exact_rows(pl, k).state != 1)
                return fail(VET_ERR_UNSUPPORTED, "%s: the exact FP64 weight rows of lattice %d are not on the device "
                            "(too large for it); the call has no other formulation", what, k);
            if (vet::dtable_lds_bytes(1, L.n) > c->lds_max)
                return fail(VET_ERR_UNSUPPORTED, "%s: lattice of %d tiles does not fit the LDS", what, L.n);
        }
    }
    return VET_OK;
}

// check_window_args of vet_window.hip, restated for the per-viewer units
int check_user_args(const vet_plan* pl, int U, int T, int window, int stride, const void* out) {
    int rc = check_run_args(pl, U, T, out);
    if (rc) return rc;
    if (window < 1) return fail(VET_ERR_INVALID, "window must be at least 1 frame (got %d)", window);
    if (stride < 1) return fail(VET_ERR_INVALID, "stride must be at least 1 frame (got %d)", stride);
    if (window > T) return fail(VET_ERR_INVALID, "window of %d frames is longer than the video's %d frames", window, T);
    return VET_OK;
}

namespace {

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

const void* user_w_kernel(int stride) {
    const int chunks = stride / vet::WAVE;
    return chunks <= 1 ? (const void*)vet::k_user_entropy_w<1> : chunks <= 2 ? (const void*)vet::k_user_entropy_w<2>
         : chunks <= 4 ? (const void*)vet::k_user_entropy_w<4> : (const void*)vet::k_user_entropy_w<0>;
}

template <bool FROM_IDS>
int launch_user(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window, int stride,
                double* d_entropy, double* d_weights, int32_t* d_samples, int32_t* d_status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const int K = (int)pl->lat.size();
    const long R = (long)vet_window_rows(T, window, stride), rows = R * (long)U;
    if (rows >= (1L << 31)) return fail(VET_ERR_UNSUPPORTED, "per-user entropy: %ld rows in one call (fewer than 2^31)", rows);
    // ---- whether this plan can run per user at all (before anything is launched)
    int rc = check_user_plan(pl, "per-user entropy", s);
    if (rc) return rc;
    // workspace: per-lattice rows (K > 1) | dirs [U][T]
    const size_t ent_b = pad16(K > 1 ? (size_t)K * rows * sizeof(double) : 0);
    rc = ensure_ws(c, ent_b + pad16((size_t)U * T * sizeof(int32_t)));
    if (rc) return rc;
    char* ws = (char*)c->ws;
    double* ent_k = K > 1 ? (double*)ws : d_entropy;
    int32_t* dirs = (int32_t*)(ws + ent_b);
    {   // ---- stage 1, charged to k_spatial
        vet::UserDirsParams q{};
        q.src = vet::SampleSrc{d_mu, d_mv, d_ids, pl->W, pl->H, (long)pl->n_dirs};
        q.U = U; q.T = T; q.dirs = dirs; q.status = d_status;
        const unsigned gy = (unsigned)((T + vet::UT - 1) / vet::UT);
        if (gy > 65535u) return fail(VET_ERR_UNSUPPORTED, "per-user entropy: %d frames in one call (at most %d)", T, 65535 * vet::UT);
        ProfScope ps(c, s, KID_SPATIAL);
        hipLaunchKernelGGL(vet::k_user_dirs<FROM_IDS>, dim3((unsigned)((U + vet::UT - 1) / vet::UT), gy), dim3(256), 0, s, q);
        HIP_TRY(hipGetLastError());
    }
    // ---- stage 2
    for (int k = 0; k < K; ++k) {
        const Lattice& L = pl->lat[k];
        double* weights = k == 0 ? d_weights : nullptr;
        int32_t *samples = k == 0 ? d_samples : nullptr, *status = k == 0 ? d_status : nullptr;
        if (counts_lattice(pl, k)) {
            vet::UserCParams q{};
            q.dirs = dirs; q.T = T; q.nearest = L.d_nearest; q.n = L.n; q.hmax = L.hmax;
            q.norm_n = L.norm_n; q.full_norm = (L.binned && pl->weighted) ? 1 : 0;
            q.window = window; q.stride = stride; q.R = R;
            // overlapping rows: a run of rows per wave, at least ~8 waves per CU in the launch
            q.rpw = stride < window ? (int)std::min<long>(64, std::max<long>(1, rows / (8L * c->n_cu))) : 1;
            q.chunks = (R + q.rpw - 1) / q.rpw;
            q.ent = ent_k + (size_t)k * rows; q.weights = weights; q.samples = samples; q.status = status;
            const long grid = q.chunks * U;
            if (grid >= (1L << 31)) return fail(VET_ERR_UNSUPPORTED, "per-user entropy: %ld workgroups in one launch", grid);
            ProfScope ps(c, s, KID_FINALIZE);
            hipLaunchKernelGGL(vet::k_user_entropy_c, dim3((unsigned)grid), dim3(vet::WAVE), (size_t)L.n * 4, s, q);
        } else {
            const WeightsCore::Exact& X = exact_rows(pl, k);
            vet::UserWParams q{};
            q.dirs = dirs; q.T = T; q.alias = pl->d_alias;
            q.X = vet::ExactRows{(const uint16_t*)X.idx.get(), (const double*)X.w.get(), (const uint32_t*)X.len.get(), X.stride, L.n};
            q.hmax = L.hmax; q.window = window; q.stride = stride; q.R = R;
            q.ent = ent_k + (size_t)k * rows; q.weights = weights; q.samples = samples; q.status = status;
            const int nw = user_nw(c->lds_max, L.n, window);
            void* args[] = {(void*)&q};
            ProfScope ps(c, s, KID_WEIGHTS);
            HIP_TRY(hipLaunchKernel(user_w_kernel(X.stride), dim3((unsigned)rows), dim3(nw * vet::WAVE), args,
                                    vet::dtable_lds_bytes(nw, L.n), s));
        }
        HIP_TRY(hipGetLastError());
    }
    if (K > 1) {
        ProfScope ps(c, s, KID_FINALIZE);
        hipLaunchKernelGGL(vet::k_finalize, dim3(grid_for(rows, 256, c->n_cu)), dim3(256), 0, s, (const double*)ent_k, K, rows, d_entropy);
        HIP_TRY(hipGetLastError());
    }
    return VET_OK;
}

}  // namespace

int user_set_attrs(vet_ctx* c) {
    for (int stride : {64, 128, 256, 512})
        HIP_TRY(hipFuncSetAttribute(user_w_kernel(stride), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_max));
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_user_entropy_c, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_max));
    return VET_OK;
}

}  // namespace vh

using namespace vh;

extern "C" {

int vet_user_entropy(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride,
                     double* d_entropy, double* d_weights, int32_t* d_samples, int32_t* d_status, void* stream) {
    int rc = check_user_args(pl, U, T, window, stride, d_entropy);
    if (rc) return rc;
    if (!pl->grid) return fail(VET_ERR_INVALID, "plan has no pixel grid; use vet_user_entropy_ids");
    if (!d_mu || !d_mv) return fail(VET_ERR_INVALID, "d_mu / d_mv is NULL");
    return launch_user<false>(pl, d_mu, d_mv, nullptr, U, T, window, stride, d_entropy, d_weights, d_samples, d_status,
                              stream ? (hipStream_t)stream : pl->ctx->stream);
}

int vet_user_entropy_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, double* d_entropy,
                         double* d_weights, int32_t* d_samples, int32_t* d_status, void* stream) {
    int rc = check_user_args(pl, U, T, window, stride, d_entropy);
    if (rc) return rc;
    if (!d_ids) return fail(VET_ERR_INVALID, "d_ids is NULL");
    return launch_user<true>(pl, nullptr, nullptr, d_ids, U, T, window, stride, d_entropy, d_weights, d_samples, d_status,
                             stream ? (hipStream_t)stream : pl->ctx->stream);
}

}  // extern "C"
