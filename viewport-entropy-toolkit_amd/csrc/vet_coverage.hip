// vet_coverage.hip — attention coverage behind vet_coverage* (include/vet.h): the kernels and their launch logic.  Rows are
// vet_spatial_entropy_windowed's (row r pools frames [r * stride, r * stride + window) into one histogram per lattice); only
// lattice 0 takes part.  With h_r >= 0 row r's histogram (the windowed call's d_weights by absolute value):
//   order_r      the tiles by weight descending, equal weights by tile index ascending (all n tiles);
//   C_j          the running sum of the weights in rank order, ONE accumulator; W_r = C_n;
//   tiles[r][i]  the smallest k with C_k >= fractions[i] * W_r (0 where W_r = 0);
//   hit[r][l][i] the share of row r + l's mass on row r's first tiles[r][i] tiles, l = 0 .. L.
// Stages, rows in chunks so that the workspace stays bounded whatever R is (vet_window_divergence.hip's scheme):
//   1  vet_spatial_entropy_windowed's stage 1, unchanged (vet_window.hip: window_frames_run);
//   2  per chunk of rows [r0, r0 + CR): lattice 0's row histograms [r0, min(R, r0 + CR + L)) — the chunk's rows and the halo of L
//      rows their lags reach (vet_window_divergence.hip: window_hist_run);
//   3  k_coverage_rank, one workgroup per row of the chunk: the row sorted in LDS, the sequential running sum, the Q thresholds;
//      leaves tiles, order and, in the workspace, every tile's rank (u16) and W_r;
//   4  k_coverage_hits, one wave per (row, lag): the masked sums of row r + l over row r's ranks.
// tiles[r], order_r and hit[r][0] are pure functions of the plan, the window, row r's frames and (per column) its own fraction;
// hit[r][l] depends on row r + l's frames besides: the sort is a total order, one lane owns the running sum, a wave's lanes take
// the tiles t = lane, lane + 64, ... in ascending order and end in wave_sum's butterfly, whatever the chunk or the launch.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_rank.hpp"
#include "vet_row_hist.hpp"

#include <algorithm>

namespace vet {

constexpr int COV_MAX_TILES = 2048;    // records of the LDS sort: 16 B x 2048 = 32 KB (include/vet.h states the limit)
constexpr int COV_MAX_Q = 8;           // fractions of a call
constexpr int COV_LB = 16;             // lags of a workgroup of k_coverage_hits (four waves, four lags each)

// One tile of a row in the sort: the weight's bit pattern (non-negative doubles order as their unsigned bits) and the tile.
// a > b  <=>  a comes later in rank order: the ascending bitonic sort leaves weight descending, tile ascending.  Padding records
// (weight 0, tile >= n) sort behind every tile of the row.  16 bytes, 16-byte aligned and all of them in use, so that the sort's
// compare-exchange moves a record with ONE 128-bit LDS access: consecutive lanes on consecutive records are conflict-free (as
// 64-bit accesses 16 bytes apart they would meet four to a bank).
struct alignas(16) CovRec {
    unsigned long long w, tile;
    __device__ __forceinline__ bool operator>(const CovRec& o) const { return w < o.w || (w == o.w && tile > o.tile); }
};
static_assert(sizeof(CovRec) == 16, "record size");

// ------------------------------------------------------------------------------------------
// k_coverage_rank — stage 3.  Workgroup x = row r0 + x of the chunk, 256 threads.
//   a  the row's n weights go to LDS as records, padded to P (a power of two, >= 8) — lds_bitonic_sort;
//   b  thread 0 adds the weights in rank order, eight LDS reads ahead of the eight dependent FP64 adds, and writes C_j over the
//      weight of record j; it stops behind the last positive weight (m of them: zeros change nothing);
//   c  every thread looks at its records j < m: tiles[i] = j + 1 where C_{j+1} >= thr_i > C_j, thr_i = fractions[i] * W (one
//      multiply; C is non-decreasing, so at most one j answers; thr_i <= 0, from W = 0 or an underflow, leaves 0 = C_0's place);
//   d  tiles, order (where wanted), the rank of every tile and W leave.
// LDS: 16 * P bytes, dynamic.
// ------------------------------------------------------------------------------------------
struct CoverageRankParams {
    RowStats in;                 // the chunk's histograms, rows [h0, ..)
    int n, P, Q;
    long h0, r0;
    double q[COV_MAX_Q];         // fractions
    int32_t* tiles;              // [R][Q]
    int32_t* order;              // [R][n] or null
    uint16_t* rank;              // [rows of the chunk][n]
    double* mass;                // [rows of the chunk] W_r
};

__global__ __launch_bounds__(256) void k_coverage_rank(const CoverageRankParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    CovRec* rec = (CovRec*)smem;
    __shared__ int s_tiles[COV_MAX_Q];
    __shared__ int s_m;
    __shared__ double s_W;
    const int tid = threadIdx.x;
    const long slot = blockIdx.x, r = p.r0 + slot;
    const double* h = p.in.hist + (r - p.h0) * (long)p.n;
    for (int t = tid; t < p.P; t += 256) {
        CovRec c;
        c.w = t < p.n ? ((unsigned long long)__double_as_longlong(h[t]) & 0x7fffffffffffffffull) : 0ull;
        c.tile = (unsigned long long)t;
        rec[t] = c;
    }
    if (tid < COV_MAX_Q) s_tiles[tid] = 0;
    lds_bitonic_sort(rec, p.P);
    if (tid == 0) {
        double C = 0.0;
        int m = 0;
        for (int j = 0; j < p.n; j += 8) {                          // j + 7 < P: P is a multiple of 8 and >= n
            double w[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k] = __longlong_as_double((long long)rec[j + k].w);
            if (!(w[0] > 0.0)) break;                               // sorted: nothing positive follows
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                C += w[k];
                rec[j + k].w = (unsigned long long)__double_as_longlong(C);
                if (w[k] > 0.0) m = j + k + 1;
            }
        }
        s_W = C;
        s_m = m;
    }
    __syncthreads();
    const double W = s_W;
    const int m = s_m;
    for (int j = tid; j < m; j += 256) {
        const double cur = __longlong_as_double((long long)rec[j].w);
        const double prev = j ? __longlong_as_double((long long)rec[j - 1].w) : 0.0;
        for (int i = 0; i < p.Q; ++i) {
            const double thr = p.q[i] * W;
            if (cur >= thr && prev < thr) s_tiles[i] = j + 1;
        }
    }
    __syncthreads();
    if (tid < p.Q) __builtin_nontemporal_store(s_tiles[tid], p.tiles + r * (long)p.Q + tid);
    for (int j = tid; j < p.n; j += 256) {
        const unsigned t = (unsigned)rec[j].tile;                   // the first n records are the row's n tiles
        if (t < (unsigned)p.n) {
            if (p.order) __builtin_nontemporal_store((int32_t)t, p.order + r * (long)p.n + j);
            p.rank[slot * (long)p.n + t] = (uint16_t)j;
        }
    }
    if (tid == 0) p.mass[slot] = W;
}

// ------------------------------------------------------------------------------------------
// k_coverage_hits<NQ> — stage 4.  Workgroup (x, y): row r = r0 + x of the chunk, lags [y * COV_LB, y * COV_LB + COV_LB); the
// row's ranks are staged in LDS once; wave w takes the lags l0 + w, l0 + w + 4, ...  For a lag the wave's lanes walk row r + l's
// histogram coalesced (tiles lane, lane + 64, ..., four loads in flight) and add h[t] to accumulator i where rank[t] <
// tiles[r][i] (+0.0 otherwise: no bit changes); wave_sum; hit = sum / W'_{r+l}, W' = window_hist_run's tot.  NaN where
// r + l >= R, W_r = 0 or W'_{r+l} = 0.  NQ = 4 or 8 accumulators (Q <= NQ).  Non-temporal stores.
// LDS: 2 * n bytes, dynamic.
// ------------------------------------------------------------------------------------------
struct CoverageHitsParams {
    RowStats in;
    int n, Q;
    long h0, r0, R, L;
    const int32_t* tiles;        // [R][Q]
    const uint16_t* rank;        // [rows of the chunk][n]
    const double* mass;          // [rows of the chunk]
    double* hit;                 // [R][L + 1][Q]
};

template <int NQ>
__global__ __launch_bounds__(256) void k_coverage_hits(const CoverageHitsParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* rk = (uint16_t*)smem;
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const long slot = blockIdx.x, r = p.r0 + slot, l0 = (long)blockIdx.y * COV_LB;
    for (int t = tid; t < p.n; t += 256) rk[t] = p.rank[slot * (long)p.n + t];
    __syncthreads();
    int k[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) k[i] = i < p.Q ? p.tiles[r * (long)p.Q + i] : 0;
    const double Wr = p.mass[slot];
    const long l_end = l0 + COV_LB < p.L + 1 ? l0 + COV_LB : p.L + 1;
    for (long l = l0 + wv; l < l_end; l += 4) {
        const long rb = r + l;
        double acc[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) acc[i] = 0.0;
        const double Wb = (rb < p.R && Wr > 0.0) ? p.in.tot[rb - p.h0] : 0.0;
        const bool ok = Wb > 0.0;
        if (ok) {
            const double* hb = p.in.hist + (rb - p.h0) * (long)p.n;
            for (int t0 = lane; t0 < p.n; t0 += 4 * WAVE) {
                double v[4];
                int rank[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int t = t0 + u * WAVE;
                    v[u] = t < p.n ? hb[t] : 0.0;
                    rank[u] = t < p.n ? (int)rk[t] : 0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int i = 0; i < NQ; ++i) acc[i] += rank[u] < k[i] ? v[u] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < NQ; ++i) acc[i] = wave_sum(acc[i]);
        }
        double mine = 0.0;
#pragma unroll
        for (int i = 0; i < NQ; ++i) mine = lane == i ? acc[i] : mine;
        if (lane < p.Q)
            __builtin_nontemporal_store(ok ? mine / Wb : __builtin_nan(""), p.hit + (r * (p.L + 1) + l) * (long)p.Q + lane);
    }
}

}  // namespace vet

namespace vh {

// What vet_coverage* refuse about their own arguments, before anything is staged, allocated or launched — after
// check_window_args; R = the rows of the call.
int check_coverage_args(const vet_plan* pl, long R, int max_lag, const double* fractions, int Q, const void* hit) {
    if (!hit) return fail(VET_ERR_INVALID, "the hit output is NULL");
    if (!fractions) return fail(VET_ERR_INVALID, "fractions is NULL");
    if (Q < 1 || Q > vet::COV_MAX_Q) return fail(VET_ERR_INVALID, "need 1 to %d fractions (got %d)", vet::COV_MAX_Q, Q);
    for (int i = 0; i < Q; ++i) {
        if (!(fractions[i] > 0.0 && fractions[i] <= 1.0))
            return fail(VET_ERR_INVALID, "fractions[%d] = %g is outside (0, 1]", i, fractions[i]);
        if (i && !(fractions[i] > fractions[i - 1])) return fail(VET_ERR_INVALID, "fractions must be strictly increasing");
    }
    if (max_lag < 0 || max_lag > R - 1)
        return fail(VET_ERR_INVALID, "max_lag must be between 0 and rows - 1 = %ld (got %d)", R - 1, max_lag);
    if (pl->lat[0].n > vet::COV_MAX_TILES)
        return fail(VET_ERR_UNSUPPORTED, "coverage: lattice 0 has %d tiles, the LDS sort holds at most %d", pl->lat[0].n,
                    vet::COV_MAX_TILES);
    if ((long)max_lag / vet::COV_LB + 1 > 65535)
        return fail(VET_ERR_UNSUPPORTED, "coverage: max_lag %d (at most %d)", max_lag, 65535 * vet::COV_LB - 1);
    if (R >= (1L << 31) - 256) return fail(VET_ERR_UNSUPPORTED, "coverage: %ld rows in one call (fewer than 2^31 - 256)", R);
    return VET_OK;
}

namespace {

constexpr size_t kCoverageHistBudget = (size_t)256 << 20;   // bytes of row histograms a chunk may take in the workspace

int check_coverage_entry(const vet_plan* pl, int U, int T, int window, int stride, int max_lag, const double* fractions, int Q,
                         const void* tiles, const void* hit) {
    int rc = check_window_args(pl, U, T, window, stride, tiles);
    if (rc) return rc;
    return check_coverage_args(pl, (long)vet_window_rows(T, window, stride), max_lag, fractions, Q, hit);
}

int launch_coverage(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window, int stride,
                    int max_lag, const double* fractions, int Q, int32_t* d_tiles, double* d_hit, int32_t* d_order,
                    int32_t* d_samples, int32_t* d_status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const long R = (long)vet_window_rows(T, window, stride), L = max_lag;
    const int n = pl->lat[0].n;
    int P = 8;
    while (P < n) P <<= 1;
    const unsigned gy = (unsigned)(L / vet::COV_LB + 1);
    WindowFrames wf;
    int rc = window_frames_layout(pl, U, T, 0, wf, s);
    if (rc) return rc;
    // rows per chunk: the histogram budget pays for the chunk's rows and the halo of L rows
    const long budget_rows = (long)(kCoverageHistBudget / ((size_t)n * sizeof(double)));
    long CR = c->tune.coverage_chunk_rows > 0 ? c->tune.coverage_chunk_rows : budget_rows - L;
    CR = std::max(1L, std::min(CR, R));
    const long HR = std::min(R, CR + L);
    // workspace: stage 1's arrays | hist [HR][n] | tot [HR] | flag [HR] | rank [CR][n] | mass [CR]
    WsLayout lay{wf.bytes};
    const size_t hist_o = lay.take<double>((size_t)HR * n), tot_o = lay.take<double>((size_t)HR), flag_o = lay.take<int32_t>((size_t)HR);
    const size_t rank_o = lay.take<uint16_t>((size_t)CR * n), mass_o = lay.take<double>((size_t)CR);
    rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    const vet::RowStats st{(double*)(ws + hist_o), (double*)(ws + tot_o), (int32_t*)(ws + flag_o)};
    // ---- stage 1 (charged as vet_spatial_entropy_windowed's)
    rc = window_frames_run(pl, d_mu, d_mv, d_ids, U, T, wf, d_status, s);
    if (rc) return rc;
    for (long r0 = 0; r0 < R; r0 += CR) {
        const long r_end = std::min(R, r0 + CR), h_end = std::min(R, r_end + L);
        const long r_new = r0 == 0 ? 0 : std::min(R, r0 + L);      // rows below were written by the chunk before
        // ---- stage 2, charged to k_finalize
        rc = window_hist_run(pl, 0, U, wf, window, stride, r0, h_end, r_new, st.hist, st.tot, st.flag, d_samples, d_status, s);
        if (rc) return rc;
        {   // ---- stage 3, charged to k_transition
            vet::CoverageRankParams q{};
            q.in = st; q.n = n; q.P = P; q.Q = Q; q.h0 = r0; q.r0 = r0;
            for (int i = 0; i < Q; ++i) q.q[i] = fractions[i];
            q.tiles = d_tiles; q.order = d_order; q.rank = (uint16_t*)(ws + rank_o); q.mass = (double*)(ws + mass_o);
            ProfScope ps(c, s, KID_TRANSITION);
            hipLaunchKernelGGL(vet::k_coverage_rank, dim3((unsigned)(r_end - r0)), dim3(256), (size_t)P * sizeof(vet::CovRec), s, q);
            HIP_TRY(hipGetLastError());
        }
        {   // ---- stage 4, charged to k_wtab: an id no steady-state call uses
            vet::CoverageHitsParams q{};
            q.in = st; q.n = n; q.Q = Q; q.h0 = r0; q.r0 = r0; q.R = R; q.L = L;
            q.tiles = d_tiles; q.rank = (const uint16_t*)(ws + rank_o); q.mass = (const double*)(ws + mass_o); q.hit = d_hit;
            ProfScope ps(c, s, KID_WTAB);
            const dim3 grid((unsigned)(r_end - r0), gy);
            if (Q <= 4) hipLaunchKernelGGL(vet::k_coverage_hits<4>, grid, dim3(256), (size_t)n * sizeof(uint16_t), s, q);
            else hipLaunchKernelGGL(vet::k_coverage_hits<8>, grid, dim3(256), (size_t)n * sizeof(uint16_t), s, q);
            HIP_TRY(hipGetLastError());
        }
    }
    return VET_OK;
}

}  // namespace

}  // namespace vh

using namespace vh;

extern "C" {

int vet_coverage(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, int max_lag,
                 const double* fractions, int Q, int32_t* d_tiles, double* d_hit, int32_t* d_order, int32_t* d_samples,
                 int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_coverage_entry(pl, U, T, window, stride, max_lag, fractions, Q, d_tiles, d_hit);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_coverage_ids", stream, &s);
    return rc ? rc : launch_coverage(pl, d_mu, d_mv, nullptr, U, T, window, stride, max_lag, fractions, Q, d_tiles, d_hit, d_order,
                                     d_samples, d_status, s);
}

int vet_coverage_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, int max_lag, const double* fractions,
                     int Q, int32_t* d_tiles, double* d_hit, int32_t* d_order, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_coverage_entry(pl, U, T, window, stride, max_lag, fractions, Q, d_tiles, d_hit);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_coverage(pl, nullptr, nullptr, d_ids, U, T, window, stride, max_lag, fractions, Q, d_tiles, d_hit, d_order,
                                     d_samples, d_status, s);
}

}  // extern "C"
