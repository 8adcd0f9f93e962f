// vet_user_transition.hip — per-viewer transition entropy behind vet_user_transition_entropy* (include/vet.h): the kernels and
// their launch logic.  A video of T frames has T - 1 frame pairs; row (u, r) pools the transitions of ONE user over pairs
// [r * stride, r * stride + window) and takes compute_transition_entropy (utilities/entropy_utils.py:213-332) of them — both
// dicts hold one entry per pair in which the user is present in both frames, in ascending pair order — per lattice, then the
// mean over the lattices (k_finalize).  The transposed question of vet_window.hip's k_window_transition: a user's pairs over
// time, not the audience's pairs of a window.
// Two stages:
//   1  k_user_dirs (vet_user_dirs.hpp): every sample quantised once, its direction id written transposed, dirs[U][T] i32
//      (-1 absent); one transposition serves every lattice, stage 2 looks up nearest[id];
//   2  per (user, row) and lattice, over the contiguous slice dirs[u][r * stride .. r * stride + window]: pair q of the row
//      has the source nearest[dirs[u][f0 + q]] and the destination nearest[dirs[u][f0 + q + 1]], f0 = r * stride.
//        window <= 64   k_user_transition_wave: a row lives in one wave's registers, lane = pair; no LDS, no atomics
//        window  > 64   k_user_transition<BD, LG>: k_window_transition's body (trans_big_* of vet_transition.hpp)
//      vet_test_user_transition_hash sends the short windows through the second kernel too.
// A row is a pure function of the plan, `window` and its own window + 1 frames of its own user: which kernel runs, the wave's
// segments, the workgroup shape and the hash are chosen by `window` alone, every row is computed from scratch and every FP64
// sum runs in an order fixed by the row's own samples.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_finalize.hpp"
#include "vet_transition.hpp"
#include "vet_user_dirs.hpp"

#include <algorithm>

namespace vet {

struct UserTransParams {
    const int32_t* dirs;         // [U][T]
    int T;
    const uint16_t* nearest;     // [n_dirs] direction -> tile of this lattice
    int n;
    double hmax;
    int window, stride;
    long R, rows;                // rows per user, U * R
    double* ent;                 // [U][R]
    int32_t* srccount;           // [U][R][n] or null
    int32_t* samples;            // [U][R] or null
    int32_t* status;             // [2] or null
    const double* log2_tab;      // [4097] log2(k)
    uint32_t* scratch;           // k_user_transition, 1024-thread shape: per-workgroup slices of W4 words
    int spw;                     // k_user_transition_wave: rows (segments) per wave, floor(64 / window)
    long waves_per_user, groups; // k_user_transition_wave: ceil(R / spw), U * waves_per_user
};

// ------------------------------------------------------------------------------------------
// k_user_transition_wave — stage 2 for window <= 64.  One wave per workgroup; a wave holds spw = floor(64 / window) consecutive
// rows of one user as segments of `window` lanes, lane base + j = pair j of its row (tail segments and the lanes behind the
// last segment are predicated).  Persistent: waves take groups blockIdx, blockIdx + gridDim, ...
// The reduced form of the header comment of vet_transition.hpp with "user index" = the pair's rank in the row, in three walks
// of `window` steps; in step i every lane reads a word of lane base + i (ds_bpermute: no LDS is allocated):
//   1  keys: the lane finds its source tile's first pair (the first i with its source), m = pairs with its source, and among
//      the tile's NON-first pairs with its own (source, destination) their count and whether one is earlier than itself — no
//      earlier one: the lane is its bucket's first sample;
//   2  source | (bucket count if bucket-first else 0): K = 1 + bucket-first lanes with the lane's source, w = the bucket count
//      of the LAST of them (ascending order: the latest first appearance), w = 1 when m = 1;
//   3  cells: the tile's first pair holds (K w / N) (log2 w - log2 m), trans_big_finish's term and table arithmetic (all
//      arguments <= 64); they are subtracted from 0 in ascending lane order of the segment, so the sum does not depend on
//      where the segment lies in the wave.  N = the segment's pairs present in both frames (a ballot).
// The row's first lane writes the outputs as trans_big_finish does (normaliser log2(n) if N > n else log2(N), N = 1: 0 / 0;
// N = 0: NaN and status[1] += 1).  srccount: the wave zero-fills its rows, then (behind a barrier) the first pair of every
// source tile writes m.  A word is thus stored twice, by two lanes of ONE wave: the workgroup is one wave, its stores to one
// address stay in issue order, and the barrier between the fill and the counts waits for the fill (vmcnt).  More than one
// wave per workgroup, or a fill moved elsewhere, would need a different scheme.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_user_transition_wave(const UserTransParams p) {
    const int lane = lane_id();
    const int seg = lane / p.window;
    const bool in_seg = seg < p.spw;
    const int base = in_seg ? seg * p.window : 0, j = lane - seg * p.window;
    const unsigned long long seg_mask = (p.window == WAVE ? ~0ull : (1ull << p.window) - 1ull) << base;
    for (long g = blockIdx.x; g < p.groups; g += gridDim.x) {
        const long u = g / p.waves_per_user, r0 = (g - u * p.waves_per_user) * p.spw, r = r0 + seg;
        const bool live = in_seg && r < p.R;
        const long row = u * p.R + r;
        unsigned key = EMPTY_KEY;
        if (live) {
            const int32_t* d = p.dirs + u * (long)p.T + r * (long)p.stride + j;
            const int ia = d[0], ib = d[1];
            if (ia >= 0 && ib >= 0) key = ((unsigned)p.nearest[ia] << 16) | (unsigned)p.nearest[ib];   // present in both frames
        }
        const bool valid = key != EMPTY_KEY;
        const unsigned src = key >> 16;                    // 0xFFFF for a lane without a pair: no tile has it
        const int N = (int)__popcll(__ballot(valid) & seg_mask);
        // ---- walk 1
        int first_i = -1;
        unsigned m = 0u, bucket = 0u;
        bool earlier = false;
        for (int i = 0; i < p.window; ++i) {
            const unsigned k = (unsigned)__shfl((int)key, base + i, WAVE);
            if (k != EMPTY_KEY && (k >> 16) == src) {
                if (first_i < 0) first_i = i;
                ++m;
                if (k == key && i != first_i) { ++bucket; earlier |= i < j; }
            }
        }
        const bool tile_first = valid && first_i == j;
        const bool bucket_first = valid && !tile_first && !earlier;
        // ---- walk 2
        const unsigned word = (src << 8) | (bucket_first ? bucket : 0u);
        unsigned K = 1u, w = 1u;
        for (int i = 0; i < p.window; ++i) {
            const unsigned v = (unsigned)__shfl((int)word, base + i, WAVE);
            if ((v & 0xFFu) && (v >> 8) == src) { ++K; w = v & 0xFFu; }
        }
        // ---- walk 3
        double cell = 0.0;
        if (tile_first) cell = ((double)((unsigned long long)K * w) * (1.0 / (double)N)) * (p.log2_tab[w] - p.log2_tab[m]);
        double h = 0.0;
        for (int i = 0; i < p.window; ++i) h -= __shfl(cell, base + i, WAVE);
        if (live && j == 0) {
            double hmax = p.hmax;
            if (!(N > p.n)) {
                const double tp = 1.0 / (double)N;          // entropy_utils.py:322-327
                hmax = (double)N * -tp * -p.log2_tab[N];
            }
            double e = h / hmax;
            if (N == 0) {
                e = __builtin_nan("");
                if (p.status) atomicAdd(&p.status[1], 1);
            }
            p.ent[row] = e;
            if (p.samples) p.samples[row] = N;
        }
        if (p.srccount) {
            const long r1 = min(p.R, r0 + (long)p.spw);
            int32_t* out = p.srccount + (u * p.R + r0) * (long)p.n;
            for (long t = lane; t < (r1 - r0) * (long)p.n; t += WAVE) out[t] = 0;
            __syncthreads();
            if (tile_first) p.srccount[row * (long)p.n + src] = (int)m;      // after the fill: the kernel's header
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_user_transition — stage 2 for window > 64 (and, under vet_test_user_transition_hash, for every window): k_window_transition's
// body over the slice dirs[u][r * stride ..] — sample q of the row is pair q, the destination lies at offset 1, and "user
// index" = q in k_transition_big's row algorithm (vet_transition.hpp: trans_big_clear / trans_big_count / trans_big_finish).
// Persistent workgroups take rows blockIdx, blockIdx + gridDim, ... of the U * R rows.  Workgroup and hash by `window` alone:
//   window <= 256: 64 threads, 512 slots | <= 1024: 256 threads, 2048 slots | <= 2048: 256 threads, 4096 slots — the hash holds
//   every pair (one pass) and the packed pairs stay in LDS behind the hash;
//   else 1024 threads, 8192 slots, passes by cap = 0.6 * 8192 - n, packed pairs in a per-workgroup global slice.
// LDS: trans_big_lds_bytes(n, slots) | pc u32 [W4] (the three small shapes)
// ------------------------------------------------------------------------------------------
template <int BD, int LG>
__global__ __launch_bounds__(BD) void k_user_transition(const UserTransParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int HS = 1 << LG;
    constexpr bool SMALL = LG < 13;
    const TransBigLds L = trans_big_carve(smem, p.n, HS);
    const int tid = threadIdx.x;
    const int W = p.window;
    const size_t W4 = ((size_t)W + 3) & ~(size_t)3;
    unsigned* pc = SMALL ? (unsigned*)(smem + trans_big_lds_bytes(p.n, HS)) : p.scratch + (size_t)blockIdx.x * W4;
    const int cap = SMALL ? 0x7FFFFFFF : HS * 6 / 10 - p.n;
    const bool tab = W <= 4096;
    int parity = 0;
    for (long row = blockIdx.x; row < p.rows; row += gridDim.x, parity ^= 1) {
        double* acc = L.acc2 + TRANS_ACC * parity;
        trans_big_clear<BD>(L, acc);
        __syncthreads();
        const long u = row / p.R, r = row - u * p.R;
        const int32_t* d = p.dirs + u * (long)p.T + r * (long)p.stride;
        for (int q = tid; q < W; q += BD) {
            const int ia = d[q], ib = d[q + 1];
            int pa = -1, cb = -1;
            if (ia >= 0 && ib >= 0) { pa = p.nearest[ia]; cb = p.nearest[ib]; }       // present in both frames of the pair
            pc[q] = trans_big_count(L, acc, (unsigned)q, pa, cb);
        }
        __syncthreads();
        trans_big_finish<BD, LG>(L, pc, W, p.n, cap, tab, p.log2_tab, p.hmax, acc, row, p.ent, p.srccount, p.samples, p.status);
    }
}

}  // namespace vet

namespace vh {

namespace {

// Shape of k_user_transition for rows of `window` pairs (the kernel's header): a function of the window alone
struct UserTransShape { int threads, lg; const void* fn; };
UserTransShape user_trans_shape(long window) {
    if (window <= 256) return {64, 9, (const void*)vet::k_user_transition<64, 9>};
    if (window <= 1024) return {256, 11, (const void*)vet::k_user_transition<256, 11>};
    if (window <= 2048) return {256, 12, (const void*)vet::k_user_transition<256, 12>};
    return {vet::TRANS_BIG_THREADS, 13, (const void*)vet::k_user_transition<vet::TRANS_BIG_THREADS, 13>};
}
size_t user_trans_lds(const UserTransShape& g, int n, long window) {
    return vet::trans_big_lds_bytes(n, 1 << g.lg) + (g.lg < 13 ? (size_t)((window + 3) & ~3L) * 4 : 0);
}

// the largest LDS footprint of k_user_transition over the plan's lattices
size_t user_trans_lds_most(const vet_plan* pl, long window) {
    const UserTransShape g = user_trans_shape(window);
    size_t most = 0;
    for (const auto& L : pl->lat) most = std::max(most, user_trans_lds(g, L.n, window));
    return most;
}

int launch_user_transition(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window,
                           int stride, double* d_entropy, int32_t* d_srccount, int32_t* d_samples, int32_t* d_status,
                           hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const int K = (int)pl->lat.size();
    const long R = (long)vet_window_rows(T - 1, window, stride), rows = R * (long)U;
    const bool wave = window <= vet::WAVE && !c->tune.user_transition_hash;
    UserTransShape g{};
    long grid = 0;
    size_t pc_words = 0;                                                  // a multiple of 4 per workgroup
    if (wave) {
        const long spw = vet::WAVE / window, groups = (R + spw - 1) / spw * U;
        grid = std::max<long>(1, std::min<long>(groups, (long)c->n_cu * 32));
    } else {
        // persistent workgroups: as many as LDS and wave slots let run at once, at most one per row
        g = user_trans_shape(window);
        const size_t lds_most = user_trans_lds_most(pl, window);          // <= kWholeLds: check_user_transition_args
        const long per_cu = std::min<long>({(long)(kWholeLds / lds_most), 32 / (g.threads / vet::WAVE), 16});
        grid = std::max<long>(1, std::min<long>(rows, (long)c->n_cu * per_cu));
        pc_words = g.lg < 13 ? 0 : (size_t)grid * (((size_t)window + 3) & ~(size_t)3);
    }
    // workspace: per-lattice rows (K > 1) | dirs [U][T] | the packed pairs of the 1024-thread shape
    WsLayout lay;
    const size_t ent_o = lay.take<double>(K > 1 ? (size_t)K * rows : 0), dirs_o = lay.take<int32_t>((size_t)U * T);
    const size_t pc_o = lay.take<uint32_t>(pc_words);
    int rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    double* ent_k = K > 1 ? (double*)(ws + ent_o) : d_entropy;
    int32_t* dirs = (int32_t*)(ws + dirs_o);
    // ---- stage 1 (the frame count was refused by check_user_transition_args)
    rc = user_dirs_run(pl, d_mu, d_mv, d_ids, U, T, dirs, d_status, "per-user transition", s);
    if (rc) return rc;
    // ---- stage 2, charged to k_transition
    for (int k = 0; k < K; ++k) {
        const Lattice& L = pl->lat[k];
        vet::UserTransParams q{};
        q.dirs = dirs; q.T = T; q.nearest = L.d_nearest; q.n = L.n; q.hmax = L.hmax;
        q.window = window; q.stride = stride; q.R = R; q.rows = rows;
        q.ent = ent_k + (size_t)k * rows;
        q.srccount = k == 0 ? d_srccount : nullptr; q.samples = k == 0 ? d_samples : nullptr; q.status = k == 0 ? d_status : nullptr;
        q.log2_tab = c->d_log2;
        q.scratch = (uint32_t*)(ws + pc_o);
        ProfScope ps(c, s, KID_TRANSITION);
        if (wave) {
            q.spw = vet::WAVE / window;
            q.waves_per_user = (R + q.spw - 1) / q.spw;
            q.groups = q.waves_per_user * U;
            hipLaunchKernelGGL(vet::k_user_transition_wave, dim3((unsigned)grid), dim3(vet::WAVE), 0, s, q);
        } else {
            void* args[] = {(void*)&q};
            HIP_TRY(hipLaunchKernel(g.fn, dim3((unsigned)grid), dim3(g.threads), args, user_trans_lds(g, L.n, window), s));
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

// Everything the entry points refuse, before anything is staged, allocated or launched (the _host entry calls it first).  The
// limits hold for both stage-2 kernels, so a refusal never depends on the window: rows pack pair << 13 | hash slot and
// tiles < 4096 (trans_big_finish).
int check_user_transition_args(const vet_plan* pl, int U, int T, int window, int stride, const void* out) {
    int rc = check_run_args(pl, U, T, out);
    if (rc) return rc;
    if (T < 2) return fail(VET_ERR_INVALID, "per-user transition entropy needs at least two frames (got %d)", T);
    if (window < 1) return fail(VET_ERR_INVALID, "window must be at least 1 frame pair (got %d)", window);
    if (stride < 1) return fail(VET_ERR_INVALID, "stride must be at least 1 frame pair (got %d)", stride);
    if (window > T - 1)
        return fail(VET_ERR_INVALID, "window of %d frame pairs is longer than the video's %d frame pairs", window, T - 1);
    if (window >= (1 << 19))
        return fail(VET_ERR_UNSUPPORTED, "per-user transition: window of %d pairs per row, the kernel packs fewer than 2^19", window);
    for (const auto& L : pl->lat)
        if (L.n > vet::TRANS_BIG_MAX_TILES)
            return fail(VET_ERR_UNSUPPORTED, "per-user transition: lattice of %d tiles (at most %d)", L.n, vet::TRANS_BIG_MAX_TILES);
    const long rows = (long)vet_window_rows(T - 1, window, stride) * U;
    if (rows >= (1L << 31)) return fail(VET_ERR_UNSUPPORTED, "per-user transition: %ld rows in one call (fewer than 2^31)", rows);
    rc = check_user_dirs_frames(T, "per-user transition");
    if (rc) return rc;
    // the hash kernel's LDS at this window (not reached with lattices of up to TRANS_BIG_MAX_TILES tiles; kept so that the
    // launch below has nothing left to refuse)
    const size_t lds_most = user_trans_lds_most(pl, window);
    if (lds_most > kWholeLds) return fail(VET_ERR_UNSUPPORTED, "per-user transition: %zu B of LDS (max %zu)", lds_most, kWholeLds);
    return VET_OK;
}

int user_transition_set_attrs(vet_ctx* c) {
    (void)c;
    for (long window : {1L, 257L, 1025L, 2049L})
        HIP_TRY(hipFuncSetAttribute(user_trans_shape(window).fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWholeLds));
    return VET_OK;
}

}  // namespace vh

using namespace vh;

extern "C" {

int vet_user_transition_entropy(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride,
                                double* d_entropy, int32_t* d_srccount, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_user_transition_args(pl, U, T, window, stride, d_entropy);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_user_transition_entropy_ids", stream, &s);
    return rc ? rc : launch_user_transition(pl, d_mu, d_mv, nullptr, U, T, window, stride, d_entropy, d_srccount, d_samples, d_status, s);
}

int vet_user_transition_entropy_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, double* d_entropy,
                                    int32_t* d_srccount, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_user_transition_args(pl, U, T, window, stride, d_entropy);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_user_transition(pl, nullptr, nullptr, d_ids, U, T, window, stride, d_entropy, d_srccount, d_samples, d_status, s);
}

}  // extern "C"
