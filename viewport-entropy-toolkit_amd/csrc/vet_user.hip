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
//                                      frame order (user_walk_w, vet_user_dirs.hpp), `dtable`'s epilogue in one wave
//        unweighted / binned lattices  k_user_entropy_c: u32 counts in LDS, a wave slides over a run of rows of one user,
//                                      k_window_entropy_c's epilogue
// The walks and the wave-level epilogues are shared with vet_user_divergence.hip and vet_crowd.hip (vet_user_dirs.hpp,
// vet_row_hist.hpp): a viewer's histogram there is this unit's by construction.
// A row is a pure function of the plan and of its own samples: the FP64 sums are taken from scratch for every row with a wave
// split that depends on `window` alone, the integer counts are exact under add and subtract, and every reduction runs in one
// wave in fixed lane order.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_finalize.hpp"
#include "vet_spatial_dtable.hpp"
#include "vet_user_dirs.hpp"
#include "vet_row_hist.hpp"

#include <algorithm>

namespace vet {

// ------------------------------------------------------------------------------------------
// k_user_entropy_w — stage 2 of a weighted Fibonacci lattice.  One workgroup per (user, row), blockIdx = u * R + r.  The row's
// histogram is user_walk_w's (vet_user_dirs.hpp: the exact rows of the row's frames added in ascending frame order, the waves
// in order), the tile values leaving as weights on the way.  The epilogue is k_spatial_dtable's for one lattice, in wave 0:
// row_total and row_entropy (vet_row_hist.hpp) over the keys, / hmax; NaN (and status[1] += 1) for a row without a sample.
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
    const int n = p.X.n;
    const long row = blockIdx.x, u = row / p.R, r = row - u * p.R;
    const int n_present = user_walk_w<S>(hist, p.dirs + u * (long)p.T + r * (long)p.stride, p.alias, p.X, p.window, [&](int t, double v) {
        if (p.weights) __builtin_nontemporal_store(weights_out(v), p.weights + row * (long)n + t);
    });
    if (wave_id() != 0) return;
    const KeyedHist keys{hist, NO_KEY_BITS};
    const double tot = row_total(n, keys);
    const double hh = row_entropy(n, tot, keys);
    if (lane_id() == 0) {
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
// tile taken from the lattice's nearest[id].  Integers, exact in any order.  The epilogue is count_row_entropy
// (vet_row_hist.hpp), the one k_window_entropy_c runs.
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
        count_row_entropy(cnt, p, row);
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

int check_user_dirs_frames(int T, const char* what) {
    if ((T + vet::UT - 1) / vet::UT > 65535)
        return fail(VET_ERR_UNSUPPORTED, "%s: %d frames in one call (at most %d)", what, T, 65535 * vet::UT);
    return VET_OK;
}

int user_dirs_run(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int32_t* dirs,
                  int32_t* d_status, const char* what, hipStream_t s) {
    int rc = check_user_dirs_frames(T, what);
    if (rc) return rc;
    vet::UserDirsParams q{};
    q.src = vet::SampleSrc{d_mu, d_mv, d_ids, pl->W, pl->H, (long)pl->n_dirs};
    q.U = U; q.T = T; q.dirs = dirs; q.status = d_status;
    const dim3 grid((unsigned)((U + vet::UT - 1) / vet::UT), (unsigned)((T + vet::UT - 1) / vet::UT));
    ProfScope ps(pl->ctx, s, KID_SPATIAL);
    if (d_ids) hipLaunchKernelGGL(vet::k_user_dirs<true>, grid, dim3(256), 0, s, q);
    else hipLaunchKernelGGL(vet::k_user_dirs<false>, grid, dim3(256), 0, s, q);
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

namespace {

const void* user_w_kernel(int stride) { return VET_KERNEL_BY_S(vet::k_user_entropy_w, row_chunk_class(stride)); }

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
    WsLayout lay;
    const size_t ent_o = lay.take<double>(K > 1 ? (size_t)K * rows : 0), dirs_o = lay.take<int32_t>((size_t)U * T);
    rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    double* ent_k = K > 1 ? (double*)(ws + ent_o) : d_entropy;
    int32_t* dirs = (int32_t*)(ws + dirs_o);
    // ---- stage 1
    rc = user_dirs_run(pl, d_mu, d_mv, d_ids, U, T, dirs, d_status, "per-user entropy", s);
    if (rc) return rc;
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
            vet::UserWParams q{};
            q.dirs = dirs; q.T = T; q.alias = pl->d_alias; q.X = exact_rows_arg(pl, k);
            q.hmax = L.hmax; q.window = window; q.stride = stride; q.R = R;
            q.ent = ent_k + (size_t)k * rows; q.weights = weights; q.samples = samples; q.status = status;
            const int nw = user_nw(c->lds_max, L.n, window);
            void* args[] = {(void*)&q};
            ProfScope ps(c, s, KID_WEIGHTS);
            HIP_TRY(hipLaunchKernel(user_w_kernel(q.X.stride), dim3((unsigned)rows), dim3(nw * vet::WAVE), args,
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
    hipStream_t s;
    int rc = check_window_args(pl, U, T, window, stride, d_entropy);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_user_entropy_ids", stream, &s);
    return rc ? rc : launch_user(pl, d_mu, d_mv, nullptr, U, T, window, stride, d_entropy, d_weights, d_samples, d_status, s);
}

int vet_user_entropy_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, double* d_entropy,
                         double* d_weights, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_args(pl, U, T, window, stride, d_entropy);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_user(pl, nullptr, nullptr, d_ids, U, T, window, stride, d_entropy, d_weights, d_samples, d_status, s);
}

}  // extern "C"
