// vet_markov.hip — windowed Markov transition statistics behind vet_transition_markov* (include/vet.h): the kernels and their
// launch logic.  A video of T frames has T - lag pairs, pair f = (frame f, frame f + lag); row r pools the (pair, user) samples of
// pairs [r * stride, r * stride + window) present in both frames.  Per lattice, with n_pc the samples per (source, destination)
// tile pair, n_p = sum_c n_pc, m_c = sum_p n_pc, N = sum n_pc and f(k) = k log2 k:
//   rate        H(c | p) = (A - B) / N, A = sum_p f(n_p) and B = sum_pc f(n_pc) over the sources with >= 2 distinct destinations
//   stationary  H(p) = log2 N - sum_p f(n_p) / N          dest  H(c) = log2 N - sum_c f(m_c) / N
//   mutual      dest - rate                               stay  sum_p n_pp / N
// then the mean over the lattices (k_finalize over [K][5 R]).  Only integer pair counts enter: no first-appearance order, nothing
// of the reference's compute_transition_entropy.
// Stage 1 is the windowed transition call's (vet_window.hip: k_window_tiles, tiles [T][U] per lattice), so a row's candidate
// samples are the contiguous slice q in [0, W), W = window * U: source tiles[f0 * U + q], destination tiles[(f0 + lag) * U + q].
// Stage 2, the shape chosen from W alone:
//   W <= 32768   k_markov_rows<P>, P the power of two >= W (1024 .. 32768): one workgroup per row, persistent over the rows; the
//                keys p * n + c sorted in LDS (mk_sort: a bitonic network), run lengths = n_pc, LDS histograms n_p and m_c;
//   W >  32768   k_markov_count: one workgroup per (row, chunk of 32768 samples), the same sort and run lengths, one global integer
//                atomicAdd per run into the row's dense u32 [n][n] matrix (the workspace, or the caller's matrix for lattice 0),
//                rows in chunks under the workspace budget; then k_markov_cells, one workgroup per row, walks the matrix in index
//                order.
// Counts are integers, exact in any order; the FP64 sums are taken per thread in ascending position (cell, tile) order, then
// wave_sum's butterfly, then the four waves in order, so a row's bits depend on the plan, window, lag and the row's frames only.
// log2 k: the context's table for k <= 4096, FP64 log2 beyond — one rule for every shape.  No FP atomics.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_finalize.hpp"

#include <algorithm>

namespace vet {

constexpr int MK_THREADS = 256;        // mk_sort's workgroup
constexpr int MK_MAX_TILES = 2048;     // keys p * n + c stay below 2^22; n_p and m_c take 16 KB of LDS (include/vet.h states the limit)
constexpr int MK_CHUNK = 32768;        // keys of one LDS sort: 128 KB of the 160 KB
constexpr int MK_MIN_P = 1024;
constexpr int MK_STATS = 5;

__device__ __forceinline__ double mk_log2(unsigned k, const double* tab) { return k <= 4096u ? tab[k] : log2((double)k); }
__device__ __forceinline__ double mk_f(unsigned k, const double* tab) { return (double)k * mk_log2(k, tab); }   // f(0) = f(1) = +0.0

// The key of candidate sample (a, b): a * n + b, EMPTY_KEY when either frame has no sample (or a tile outside the lattice)
__device__ __forceinline__ unsigned mk_key(int a, int b, int n) {
    return ((unsigned)a < (unsigned)n && (unsigned)b < (unsigned)n) ? (unsigned)a * (unsigned)n + (unsigned)b : EMPTY_KEY;
}

// keys[0 .. P) in LDS ascending, P a power of two >= 1024; every thread of the 256-thread workgroup calls it; begins and ends with a
// barrier like lds_bitonic_sort (vet_rank.hpp), whose network this is.  The unit's own walk of it: a thread takes the P / 2
// compare-exchange pairs t, t + 256, ... of a stage (i = t with a zero bit inserted at j, partner i | j) instead of all P positions
// of which every other one idles, four pairs at a time with their eight LDS reads in flight ahead of the stores (the pairs of a
// stage are disjoint).  Measured against lds_bitonic_sort in this unit: profiles/markov/markov_timing.json (sort_walk).
__device__ __forceinline__ void mk_sort(unsigned* x, int P) {
    const int tid = threadIdx.x, half = P >> 1;
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t0 = tid; t0 < half; t0 += 4 * MK_THREADS) {
                int i[4];
                unsigned a[4], b[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int t = t0 + u * MK_THREADS;
                    i[u] = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    if (t < half) { a[u] = x[i[u]]; b[u] = x[i[u] | j]; }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (t0 + u * MK_THREADS < half && (a[u] > b[u]) == ((i[u] & k) == 0)) { x[i[u]] = b[u]; x[i[u] | j] = a[u]; }
            }
        }
    __syncthreads();
}

// The runs of the ascending keys[0 .. P) (EMPTY_KEY behind every key): the thread that holds a run's first position finds its end
// by a galloping then binary search — a crowd on one tile pair costs log P, not its length — and calls fn(start, key, end).
// Every thread walks its positions tid, tid + 256, ... in ascending order.
template <class Fn>
__device__ __forceinline__ void mk_runs(const unsigned* keys, int P, Fn fn) {
    for (int i = threadIdx.x; i < P; i += MK_THREADS) {
        const unsigned key = keys[i];
        if (key == EMPTY_KEY) break;                            // sorted: nothing behind it
        if (i && keys[i - 1] == key) continue;
        int lo = i + 1, step = 1;                               // keys[lo - 1] == key
        while (lo + step <= P && keys[lo + step - 1] == key) { lo += step; step <<= 1; }
        int hi = min(P, lo + step - 1);                         // the run ends in [lo, hi]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys[mid] == key) lo = mid + 1; else hi = mid;
        }
        fn(i, key, lo);
    }
}

// The five sums of a row, and the end of every stage 2 shape: wave_sum's butterfly, the four waves added in order by thread 0, the
// statistics from them.  part: LDS f64 [4][4], cnt: LDS u32 [4][2].
struct MarkovSums {
    double A = 0.0, B = 0.0, Sp = 0.0, Sc = 0.0;
    unsigned stay = 0u, N = 0u;
};
struct MarkovOut {
    long R;
    double* stats;               // [5][R] of this lattice
    int32_t* samples;            // [R] or null
    int32_t* status;             // [2] or null
    const double* log2_tab;      // [4097] log2(k)
};

__device__ __forceinline__ void mk_finish(MarkovSums v, double (*part)[4], unsigned (*cnt)[2], const MarkovOut& o, long r) {
    const int lane = lane_id(), wv = wave_id();
    v.A = wave_sum(v.A); v.B = wave_sum(v.B); v.Sp = wave_sum(v.Sp); v.Sc = wave_sum(v.Sc);
    v.stay = (unsigned)wave_sum((int)v.stay); v.N = (unsigned)wave_sum((int)v.N);
    if (lane == 0) {
        part[wv][0] = v.A; part[wv][1] = v.B; part[wv][2] = v.Sp; part[wv][3] = v.Sc;
        cnt[wv][0] = v.stay; cnt[wv][1] = v.N;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double A = 0.0, B = 0.0, Sp = 0.0, Sc = 0.0;
        unsigned stay = 0u, N = 0u;
        for (int w = 0; w < MK_THREADS / WAVE; ++w) {
            A += part[w][0]; B += part[w][1]; Sp += part[w][2]; Sc += part[w][3];
            stay += cnt[w][0]; N += cnt[w][1];
        }
        double out[MK_STATS];
        if (N == 0u) {
            for (int i = 0; i < MK_STATS; ++i) out[i] = __builtin_nan("");
            if (o.status) atomicAdd(&o.status[1], 1);
        } else {
            const double dN = (double)N, lN = mk_log2(N, o.log2_tab);
            out[0] = (A - B) / dN;
            out[1] = lN - Sp / dN;
            out[2] = lN - Sc / dN;
            out[3] = out[2] - out[0];
            out[4] = (double)stay / dN;
        }
        for (int i = 0; i < MK_STATS; ++i) o.stats[(long)i * o.R + r] = out[i];
        if (o.samples) o.samples[r] = (int32_t)N;
    }
}

// ------------------------------------------------------------------------------------------
// k_markov_rows<P> — stage 2 for W = window * U <= P <= 32768 candidate samples per row.  256 threads; persistent workgroups
// take rows blockIdx, blockIdx + gridDim, ...  Per row:
//   a  n_p and m_c zeroed; every candidate's key to LDS (EMPTY_KEY up to P), the pooled ones counted into n_p and m_c (LDS
//      integer atomics);
//   b  mk_sort;
//   c  mk_runs: a run is one (p, c) pair, its length n_pc.  The keys in front of and behind the run tell whether it is its
//      source's first run and its last: first and last = the source's only destination, the run enters neither A nor B.  A
//      source's first run adds f(n_p) to Sp (and to A unless it is the only one); p == c adds n_pc to stay; with a matrix the run
//      start stores n_pc into the zeroed output;
//   d  f(m_c) over the tiles tid, tid + 256, ...; mk_finish.
// Shapes (a function of W alone): P = 1024 for W <= 1024, then 2048, 4096, 8192, 16384, 32768.
// LDS: keys u32 [P] | n_p u32 [n] | m_c u32 [n] (dynamic: 4 P + 8 n bytes, at most 144 KB) + 160 B static.
// ------------------------------------------------------------------------------------------
struct MarkovRowsParams {
    const int32_t* tiles;        // [T][U]
    int U, n;
    int window, stride, lag;
    MarkovOut out;
    int32_t* matrix;             // [R][n][n], zeroed, or null
};

template <int P>
__global__ __launch_bounds__(MK_THREADS) void k_markov_rows(const MarkovRowsParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double s_part[MK_THREADS / WAVE][4];
    __shared__ unsigned s_cnt[MK_THREADS / WAVE][2];
    unsigned* keys = (unsigned*)smem;
    unsigned* np = keys + P;
    unsigned* mc = np + p.n;
    const int tid = threadIdx.x, n = p.n;
    const int W = p.window * p.U;
    const long nn = (long)n * n;
    for (long r = blockIdx.x; r < p.out.R; r += gridDim.x) {
        for (int t = tid; t < n; t += MK_THREADS) { np[t] = 0u; mc[t] = 0u; }
        __syncthreads();
        const int32_t* src = p.tiles + r * (long)p.stride * p.U;
        const int32_t* dst = src + (long)p.lag * p.U;
        for (int q = tid; q < P; q += MK_THREADS) {
            unsigned key = EMPTY_KEY;
            if (q < W) {
                const int a = src[q], b = dst[q];
                key = mk_key(a, b, n);
                if (key != EMPTY_KEY) { atomicAdd(&np[a], 1u); atomicAdd(&mc[b], 1u); }
            }
            keys[q] = key;
        }
        mk_sort(keys, P);
        MarkovSums v;
        mk_runs(keys, P, [&](int i, unsigned key, int end) {
            const unsigned a = key / (unsigned)n, base = a * (unsigned)n, len = (unsigned)(end - i);
            const bool first = i == 0 || keys[i - 1] < base;
            const bool last = end == P || keys[end] >= base + (unsigned)n;      // EMPTY_KEY included
            if (first) {
                const double fp = mk_f(np[a], p.out.log2_tab);
                v.Sp += fp;
                if (!last) v.A += fp;
            }
            if (!(first && last)) v.B += mk_f(len, p.out.log2_tab);
            if (key - base == a) v.stay += len;
            v.N += len;
            if (p.matrix) p.matrix[r * nn + key] = (int32_t)len;
        });
        for (int t = tid; t < n; t += MK_THREADS) v.Sc += mk_f(mc[t], p.out.log2_tab);
        mk_finish(v, s_part, s_cnt, p.out, r);
    }
}

// ------------------------------------------------------------------------------------------
// k_markov_count — stage 2a for W > 32768.  Workgroup (x, y): candidates [x * 32768, min(W, x * 32768 + 32768)) of row r0 + y;
// their keys sorted in LDS (P = the power of two >= their number, at least 1024), mk_runs, one global integer atomicAdd per run
// into mat[y][key].  Integers: exact whatever the order of the chunks.
// LDS: keys u32 [32768] (dynamic).
// ------------------------------------------------------------------------------------------
struct MarkovCountParams {
    const int32_t* tiles;        // [T][U]
    int U, n;
    long W;
    int stride, lag;
    long r0;
    unsigned* mat;               // [rows of the pass][n][n], zeroed
};

__global__ __launch_bounds__(MK_THREADS) void k_markov_count(const MarkovCountParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* keys = (unsigned*)smem;
    const int tid = threadIdx.x;
    const long q0 = (long)blockIdx.x * MK_CHUNK;
    const int m = (int)min((long)MK_CHUNK, p.W - q0);
    int P = MK_MIN_P;
    while (P < m) P <<= 1;
    const int32_t* src = p.tiles + (p.r0 + blockIdx.y) * (long)p.stride * p.U + q0;
    const int32_t* dst = src + (long)p.lag * p.U;
    for (int q = tid; q < P; q += MK_THREADS) keys[q] = q < m ? mk_key(src[q], dst[q], p.n) : EMPTY_KEY;
    mk_sort(keys, P);
    unsigned* mat = p.mat + (long)blockIdx.y * p.n * p.n;
    mk_runs(keys, P, [&](int i, unsigned key, int end) { atomicAdd(&mat[key], (unsigned)(end - i)); });
}

// ------------------------------------------------------------------------------------------
// k_markov_cells — stage 2b for W > 32768.  Workgroup x = row r0 + x: its dense matrix walked twice in index order, every thread
// the cells tid, tid + 256, ... ascending.  Walk 1: n_p, m_c and the distinct destinations d_p of every source (LDS integer
// atomics, non-zero cells only).  Walk 2: f(n_pc) to B where d_p >= 2, the diagonal to stay.  Then the tiles tid, tid + 256, ...:
// f(n_p) to Sp (and to A where d_p >= 2), f(m_c) to Sc; mk_finish.
// LDS: n_p | m_c | d_p, u32 [n] each (dynamic: 12 n bytes) + 160 B static.
// ------------------------------------------------------------------------------------------
struct MarkovCellsParams {
    const unsigned* mat;         // [rows of the pass][n][n]
    int n;
    long r0;
    MarkovOut out;
};

__global__ __launch_bounds__(MK_THREADS) void k_markov_cells(const MarkovCellsParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double s_part[MK_THREADS / WAVE][4];
    __shared__ unsigned s_cnt[MK_THREADS / WAVE][2];
    const int tid = threadIdx.x, n = p.n;
    unsigned* np = (unsigned*)smem;
    unsigned* mc = np + n;
    unsigned* nd = mc + n;
    const long cells = (long)n * n;
    const unsigned* mat = p.mat + (long)blockIdx.x * cells;
    const int da = MK_THREADS / n, db = MK_THREADS % n;         // a step of 256 cells in (source, destination)
    for (int t = tid; t < n; t += MK_THREADS) { np[t] = 0u; mc[t] = 0u; nd[t] = 0u; }
    __syncthreads();
    int a = tid / n, b = tid % n;
    for (long i = tid; i < cells; i += MK_THREADS) {
        const unsigned v = mat[i];
        if (v) { atomicAdd(&np[a], v); atomicAdd(&mc[b], v); atomicAdd(&nd[a], 1u); }
        a += da; b += db;
        if (b >= n) { b -= n; ++a; }
    }
    __syncthreads();
    MarkovSums s;
    a = tid / n; b = tid % n;
    for (long i = tid; i < cells; i += MK_THREADS) {
        const unsigned v = mat[i];
        if (v) {
            if (nd[a] >= 2u) s.B += mk_f(v, p.out.log2_tab);
            if (a == b) s.stay += v;
        }
        a += da; b += db;
        if (b >= n) { b -= n; ++a; }
    }
    for (int t = tid; t < n; t += MK_THREADS) {
        const double fp = mk_f(np[t], p.out.log2_tab);
        s.Sp += fp;
        if (nd[t] >= 2u) s.A += fp;
        s.Sc += mk_f(mc[t], p.out.log2_tab);
        s.N += np[t];
    }
    mk_finish(s, s_part, s_cnt, p.out, p.r0 + blockIdx.x);
}

}  // namespace vet

namespace vh {

// What vet_transition_markov* refuse about their arguments, before anything is staged, allocated or launched.
int check_markov_args(const vet_plan* pl, int U, int T, int window, int stride, int lag, const void* stats, const void* matrix) {
    int rc = check_run_args(pl, U, T, stats);
    if (rc) return rc;
    if (lag < 1) return fail(VET_ERR_INVALID, "lag must be at least 1 frame (got %d)", lag);
    if (lag > T - 1) return fail(VET_ERR_INVALID, "lag of %d frames leaves no pair in a video of %d frames", lag, T);
    if (window < 1) return fail(VET_ERR_INVALID, "window must be at least 1 frame pair (got %d)", window);
    if (stride < 1) return fail(VET_ERR_INVALID, "stride must be at least 1 frame pair (got %d)", stride);
    if (window > T - lag)
        return fail(VET_ERR_INVALID, "window of %d frame pairs is longer than the video's %d frame pairs at lag %d", window, T - lag, lag);
    if ((int64_t)window * U > (int64_t)0x7FFFFFFF)
        return fail(VET_ERR_UNSUPPORTED, "transition markov: window * n_users = %lld candidate samples per row (at most 2^31 - 1)",
                    (long long)window * U);
    for (const auto& L : pl->lat)
        if (L.n > vet::MK_MAX_TILES)
            return fail(VET_ERR_UNSUPPORTED, "transition markov: lattice of %d tiles (at most %d)", L.n, vet::MK_MAX_TILES);
    const int64_t R = vet_window_rows(T - lag, window, stride), n0 = pl->lat[0].n;
    if (matrix && R * n0 * n0 > (int64_t)0x7FFFFFFF)
        return fail(VET_ERR_UNSUPPORTED, "transition markov: a matrix output of %lld cells (at most 2^31 - 1 per call)",
                    (long long)(R * n0 * n0));
    return VET_OK;
}

namespace {

constexpr size_t kMarkovMatrixBudget = (size_t)256 << 20;   // bytes of row matrices a pass of the chunked shape may take

// Shape of k_markov_rows for W candidate samples per row (the kernel's header): a function of W alone
struct MarkovShape { int P; const void* fn; };
MarkovShape markov_shape(long W) {
    if (W <= 1024) return {1024, (const void*)vet::k_markov_rows<1024>};
    if (W <= 2048) return {2048, (const void*)vet::k_markov_rows<2048>};
    if (W <= 4096) return {4096, (const void*)vet::k_markov_rows<4096>};
    if (W <= 8192) return {8192, (const void*)vet::k_markov_rows<8192>};
    if (W <= 16384) return {16384, (const void*)vet::k_markov_rows<16384>};
    return {32768, (const void*)vet::k_markov_rows<32768>};
}

int launch_markov(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window, int stride,
                  int lag, double* d_stats, int32_t* d_matrix, int32_t* d_samples, int32_t* d_status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const int K = (int)pl->lat.size();
    const long R = (long)vet_window_rows(T - lag, window, stride), W = (long)window * U;
    const bool in_lds = W <= vet::MK_CHUNK;
    const MarkovShape g = markov_shape(W);
    int n_most = 0;
    for (const auto& L : pl->lat) n_most = std::max(n_most, L.n);
    // the chunked shape: rows per pass under the matrix budget (one grid row each)
    long CR = c->tune.markov_chunk_rows > 0 ? c->tune.markov_chunk_rows : (long)(kMarkovMatrixBudget / ((size_t)n_most * n_most * 4));
    CR = std::max(1L, std::min({CR, R, 65535L}));
    // workspace: per-lattice statistics (K > 1) | one lattice's tiles [T][U], reused lattice after lattice on the stream | the
    // row matrices of a pass of the chunked shape
    WsLayout lay;
    const size_t ent_o = lay.take<double>(K > 1 ? (size_t)K * vet::MK_STATS * R : 0), tiles_o = lay.take<int32_t>((size_t)T * U),
                 mat_o = lay.take<uint32_t>(in_lds ? 0 : (size_t)CR * n_most * n_most);
    int rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    double* ent_k = K > 1 ? (double*)(ws + ent_o) : d_stats;
    int32_t* tiles = (int32_t*)(ws + tiles_o);
    for (int k = 0; k < K; ++k) {
        const int n = pl->lat[k].n;
        const size_t cells = (size_t)n * n;
        // stage 1, the windowed transition call's
        rc = window_tiles_lattice(pl, k, d_mu, d_mv, d_ids, U, T, tiles, k == 0 ? d_status : nullptr, s);
        if (rc) return rc;
        const vet::MarkovOut out{R, ent_k + (size_t)k * vet::MK_STATS * R, k == 0 ? d_samples : nullptr, k == 0 ? d_status : nullptr,
                                 c->d_log2};
        int32_t* matrix = k == 0 ? d_matrix : nullptr;
        if (in_lds) {
            vet::MarkovRowsParams q{};
            q.tiles = tiles; q.U = U; q.n = n; q.window = window; q.stride = stride; q.lag = lag;
            q.out = out; q.matrix = matrix;
            // persistent workgroups: as many as LDS and wave slots let run at once, at most one per row
            const size_t lds = (size_t)g.P * 4 + (size_t)n * 8;
            const long per_cu = std::min<long>((long)(kWholeLds / lds), 32 / (vet::MK_THREADS / vet::WAVE));
            const long grid = std::max<long>(1, std::min<long>(R, (long)c->n_cu * per_cu));
            ProfScope ps(c, s, KID_TRANSITION);
            if (matrix) HIP_TRY(hipMemsetAsync(matrix, 0, (size_t)R * cells * 4, s));
            void* args[] = {(void*)&q};
            HIP_TRY(hipLaunchKernel(g.fn, dim3((unsigned)grid), dim3(vet::MK_THREADS), args, lds, s));
            HIP_TRY(hipGetLastError());
            continue;
        }
        const unsigned chunks = (unsigned)((W + vet::MK_CHUNK - 1) / vet::MK_CHUNK);
        for (long r0 = 0; r0 < R; r0 += CR) {
            const long cr = std::min(CR, R - r0);
            uint32_t* mat = matrix ? (uint32_t*)matrix + (size_t)r0 * cells : (uint32_t*)(ws + mat_o);
            {
                vet::MarkovCountParams q{};
                q.tiles = tiles; q.U = U; q.n = n; q.W = W; q.stride = stride; q.lag = lag; q.r0 = r0; q.mat = mat;
                ProfScope ps(c, s, KID_TRANSITION);
                HIP_TRY(hipMemsetAsync(mat, 0, (size_t)cr * cells * 4, s));
                hipLaunchKernelGGL(vet::k_markov_count, dim3(chunks, (unsigned)cr), dim3(vet::MK_THREADS), (size_t)vet::MK_CHUNK * 4, s, q);
                HIP_TRY(hipGetLastError());
            }
            {   // charged to k_wtab: an id no steady-state call uses, so that the two kernels can be told apart
                vet::MarkovCellsParams q{};
                q.mat = mat; q.n = n; q.r0 = r0; q.out = out;
                ProfScope ps(c, s, KID_WTAB);
                hipLaunchKernelGGL(vet::k_markov_cells, dim3((unsigned)cr), dim3(vet::MK_THREADS), (size_t)n * 12, s, q);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    if (K > 1) {
        const long rows = (long)vet::MK_STATS * R;
        ProfScope ps(c, s, KID_FINALIZE);
        hipLaunchKernelGGL(vet::k_finalize, dim3(grid_for(rows, 256, c->n_cu)), dim3(256), 0, s, (const double*)ent_k, K, rows, d_stats);
        HIP_TRY(hipGetLastError());
    }
    return VET_OK;
}

}  // namespace

int markov_set_attrs(vet_ctx*) {
    for (long W : {1L, 1025L, 2049L, 4097L, 8193L, 16385L})
        HIP_TRY(hipFuncSetAttribute(markov_shape(W).fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWholeLds));
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_markov_count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWholeLds));
    return VET_OK;
}

}  // namespace vh

using namespace vh;

extern "C" {

int vet_transition_markov(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, int lag,
                          double* d_stats, int32_t* d_matrix, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_markov_args(pl, U, T, window, stride, lag, d_stats, d_matrix);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_transition_markov_ids", stream, &s);
    return rc ? rc : launch_markov(pl, d_mu, d_mv, nullptr, U, T, window, stride, lag, d_stats, d_matrix, d_samples, d_status, s);
}

int vet_transition_markov_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, int lag, double* d_stats,
                              int32_t* d_matrix, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_markov_args(pl, U, T, window, stride, lag, d_stats, d_matrix);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_markov(pl, nullptr, nullptr, d_ids, U, T, window, stride, lag, d_stats, d_matrix, d_samples, d_status, s);
}

}  // extern "C"
