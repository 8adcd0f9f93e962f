// vet_crowd.hip — viewer-to-crowd divergence behind vet_crowd_divergence* (include/vet.h): the kernels and their launch logic.
// For every row r (frames [r * stride, r * stride + window)) and viewer u, how typical the viewer is of the audience: with h_u
// the viewer's row histogram (vet_user_entropy's d_weights, total W_u) and P_r the row's pooled histogram
// (vet_spatial_entropy_windowed's d_weights, total W_r),
//     D_k(u, r) = sum_{t in keys of h_u} q_t log2(q_t / p_t),   q_t = h_ut / W_u,   p_t = P_rt / W_r            (bits)
// the Kullback-Leibler divergence of the viewer from the crowd, 0 <= D <= log2(W_r / W_u), and per row the decomposition
//     pooled = S(P_r),   within = sum_u (W_u / W_r) S(h_u),   between = sum_u (W_u / W_r) D_k(u, r),   pooled = within + between,
// S(h) = -sum_keys (h_t / W) log2(h_t / W) being the reference's `entropy` before the normaliser (compute_spatial_entropy,
// utilities/entropy_utils.py:194-198; naive plans: compute_naive_spatial_entropy); then the mean over the lattices.
// Stages, rows in chunks so that the workspace stays bounded whatever R is:
//   1  k_user_dirs (vet_user_dirs.hpp, unchanged): direction ids transposed once, dirs[U][T];
//   2  vet_spatial_entropy_windowed's stage 1, unchanged (vet_window.hip: window_frames_run): every frame's histogram once;
//   3  per lattice and chunk of rows, k_window_hist_w/_c (vet_window_divergence.hip: window_hist_run): P[rows][n] f64, W_r and
//      the row's flag (no sample, or the row's own S is NaN under the reference's q * log2 q); k_crowd_logp: log2 p_t per row and
//      tile, once;
//   4  k_crowd_w (weighted Fibonacci lattices) / k_crowd_c (unweighted and binned lattices): one workgroup per (row, viewer),
//      the viewer fastest so that neighbouring workgroups read the same row's table from L2.  The viewer's histogram is built
//      in LDS by k_user_entropy_w's / k_user_entropy_c's walk and never leaves it; wave 0 takes W_u, S(h_u) and D against the
//      row's log2 p table read straight from global (lanes along t: coalesced), every reduction in lane order followed by
//      wave_sum's butterfly;
//   5  k_crowd_rows: one wave per row, each lane sums its viewers in ascending order, then wave_sum.
// Several lattices: lattice 0 stores its value / K, later lattices add theirs, in lattice order; a NaN of any lattice stays.
// What wave 0's epilogue costs per key tile of the viewer: k_user_entropy_w's own (one LDS read, the division by W_u, one FP64
// log2) plus one 8-byte global read of log2 p_t, a subtraction and a multiply-add: D = sum q (log2 q - log2 p_t) shares the log2.
// A value is a pure function of the plan, the window and the frames of its row: the walk is vet_user_entropy's (pure), the P row
// vet_spatial_entropy_windowed's (pure), and nothing here depends on stride, the number of rows, the chunk or the entry point.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_spatial_dtable.hpp"
#include "vet_user_dirs.hpp"
#include "vet_row_hist.hpp"

#include <algorithm>

namespace vet {

// what stage 3 leaves per row of the chunk (read-only here): RowStats — P_r [CR][n], W_r [CR] and the row's flag [CR] — and
struct CrowdRows : RowStats {
    const double* logp;          // [CR][n]  log2(P_rt / W_r) where P_rt > 0 (k_crowd_logp), +0.0 elsewhere
};

// what stage 4 leaves per (row of the chunk, viewer) for stage 5
constexpr int CROWD_OK = 0, CROWD_ABSENT = 1, CROWD_NAN = 2;
struct CrowdStats {
    double* div;                 // [CR][U]  D_k(u, r), NaN where it is not a number
    double* tot;                 // [CR][U]  W_u
    double* own;                 // [CR][U]  S(h_u)
    int32_t* flag;               // [CR][U]  CROWD_OK, CROWD_ABSENT (no sample in the row), CROWD_NAN (the viewer's own S is NaN)
};

struct CrowdOut {
    CrowdStats st;
    double* out;                 // [U][R]
    int32_t* samples;            // [U][R] or null
    int32_t* status;             // [2] or null
    long R, r0;                  // rows per user, first row of the chunk
    int U;
    int first;                   // lattice 0: store; later lattices: add
    double K;                    // lattices of the plan
};

// Wave 0's epilogue of k_crowd_w / k_crowd_c for slot = rc * U + u.  value(t, v): whether tile t is a key of the viewer's
// histogram, and its value (vet_row_hist.hpp).  W_u = row_total, then S(h_u) and D in one pass in lane order: q = v / W_u,
// S -= q log2 q (row_entropy's statement; the reference's term: NaN for q = 0), D += q (log2 q - log2 p_t) with log2 p_t
// read from the row's table: the one log2 of the tile serves both sums.
template <class V>
__device__ __forceinline__ void crowd_epilogue(const CrowdRows& in, const CrowdOut& o, long slot, int n, int n_present, V value) {
    const int lane = lane_id();
    const long rc = slot / o.U, u = slot - rc * o.U, r = o.r0 + rc;
    const double* LP = in.logp + rc * (long)n;
    const double tot = row_total(n, value);
    double hh = 0.0, dd = 0.0;
    for (int t = lane; t < n; t += WAVE) {
        double v;
        if (value(t, v)) {
            const double q = v / tot, lq = log2(q);
            hh -= q * lq;
            dd += q * (lq - LP[t]);
        }
    }
    hh = wave_sum(hh);
    dd = wave_sum(dd);
    if (lane == 0) {
        const int fl = n_present == 0 ? CROWD_ABSENT : isnan(hh) ? CROWD_NAN : CROWD_OK;
        const double d = (fl != CROWD_OK || in.flag[rc]) ? __builtin_nan("") : dd;
        o.st.div[slot] = d;
        o.st.tot[slot] = tot;
        o.st.own[slot] = hh;
        o.st.flag[slot] = fl;
        double* dst = o.out + u * o.R + r;
        *dst = o.first ? d / o.K : *dst + d / o.K;
        if (o.samples) o.samples[u * o.R + r] = n_present;
        if (o.status && n_present == 0) atomicAdd(&o.status[1], 1);
    }
}

// ------------------------------------------------------------------------------------------
// k_crowd_w — stage 4 of a weighted Fibonacci lattice for rows [r0, r0 + CR).  One workgroup per (row, viewer),
// blockIdx = (r - r0) * U + u.  user_walk_w (vet_user_dirs.hpp: k_user_entropy_w's walk, same NW from the host) leaves the tile
// values in LDS; then wave 0 runs crowd_epilogue.  Nothing of the histogram is written to memory.
// LDS: dtable_lds_bytes(NW, n).
// ------------------------------------------------------------------------------------------
struct CrowdWParams {
    const int32_t* dirs;         // [U][T]
    int T;
    const uint32_t* alias;       // [n_dirs] direction -> row | mirrored << 31
    ExactRows X;
    int window, stride;
    CrowdRows in;
    CrowdOut o;
};

template <int S>
__global__ __launch_bounds__(256) void k_crowd_w(const CrowdWParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* hist = (double*)smem;                                  // [NW][n]
    const long slot = blockIdx.x, rc = slot / p.o.U, u = slot - rc * p.o.U, r = p.o.r0 + rc;
    const int n_present = user_walk_w<S>(hist, p.dirs + u * (long)p.T + r * (long)p.stride, p.alias, p.X, p.window, [](int, double) {});
    if (wave_id() != 0) return;
    crowd_epilogue(p.in, p.o, slot, p.X.n, n_present, KeyedHist{hist, NO_KEY_BITS});
}

// ------------------------------------------------------------------------------------------
// k_crowd_c — stage 4 of an integer-count lattice (unweighted nearest tile, naive lat/lon bins) for rows [r0, r0 + CR).  One wave
// per (row, viewer), blockIdx = (r - r0) * U + u: user_row_count (vet_user_dirs.hpp) over the row's frames, every row counted
// afresh, then crowd_epilogue on the exact integers (a key is a tile with a count; W_u = the row's samples).
// LDS: u32 [n].
// ------------------------------------------------------------------------------------------
struct CrowdCParams {
    const int32_t* dirs;         // [U][T]
    int T;
    const uint16_t* nearest;     // [n_dirs] direction -> tile / bin
    int n;
    int window, stride;
    CrowdRows in;
    CrowdOut o;
};

__global__ __launch_bounds__(64) void k_crowd_c(const CrowdCParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* cnt = (unsigned*)smem;
    const long slot = blockIdx.x, rc = slot / p.o.U, u = slot - rc * p.o.U, r = p.o.r0 + rc;
    const int np = user_row_count(cnt, p.n, p.dirs + u * (long)p.T, p.nearest, r * (long)p.stride, p.window, [](int, unsigned) {});
    crowd_epilogue(p.in, p.o, slot, p.n, np, [&](int t, double& v) {
        const unsigned c = cnt[t];
        v = (double)c;
        return c != 0u;
    });
}

// ------------------------------------------------------------------------------------------
// k_crowd_logp — between stages 3 and 4: logp[rc][t] = log2(P[rc][t] / W_r) for the tiles of the chunk's rows with weight, +0.0
// elsewhere; one thread per (row, tile).  Taken once per row and tile here, not once per (row, viewer, key tile) in stage 4.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_crowd_logp(const double* hist, const double* tot, double* logp, int n, long cells) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells) return;
    const double v = hist[i];
    logp[i] = v > 0.0 ? log2(v / tot[i / n]) : 0.0;
}

// ------------------------------------------------------------------------------------------
// k_crowd_rows — stage 5 for rows [r0, r0 + CR).  One wave per row, NW rows per workgroup, no barriers, no LDS.
// pooled = S(P_r): -sum q log2 q over the tiles with weight in lane order, wave_sum.  within / between: lane l takes the viewers
// l, l + 64, ... in ascending order, skips those without a sample and adds (W_u / W_r) S(h_u) and (W_u / W_r) D(u, r); wave_sum.
// A viewer whose own S is NaN makes within and between NaN through the sum itself; the row's flag makes all three NaN.
// Output rows[3][R] = pooled, within, between: lattice 0 stores its value / K, later lattices add.
// ------------------------------------------------------------------------------------------
struct CrowdRowsParams {
    CrowdRows in;
    CrowdStats st;               // read
    int U, n;
    long R, r0, cr;              // rows of the call, first row and rows of the chunk
    int first;
    double K;
    double* rows;                // [3][R]
};

__global__ __launch_bounds__(256) void k_crowd_rows(const CrowdRowsParams p) {
    const int NW = blockDim.x >> 6, lane = lane_id(), wv = wave_id();
    const long rc = (long)blockIdx.x * NW + wv;
    if (rc >= p.cr) return;
    const double* P = p.in.hist + rc * (long)p.n;
    const double Wr = p.in.tot[rc];
    double pooled = 0.0;
    for (int t = lane; t < p.n; t += WAVE) {
        const double v = P[t];
        if (v > 0.0) {
            const double q = v / Wr;
            pooled -= q * log2(q);
        }
    }
    pooled = wave_sum(pooled);
    double within = 0.0, between = 0.0;
    for (int u = lane; u < p.U; u += WAVE) {
        const long slot = rc * p.U + u;
        if (p.st.flag[slot] != CROWD_ABSENT) {
            const double m = p.st.tot[slot] / Wr;
            within += m * p.st.own[slot];
            between += m * p.st.div[slot];
        }
    }
    within = wave_sum(within);
    between = wave_sum(between);
    if (lane < 3) {
        double v = lane == 0 ? pooled : lane == 1 ? within : between;
        if (p.in.flag[rc]) v = __builtin_nan("");
        double* dst = p.rows + lane * p.R + p.r0 + rc;
        *dst = p.first ? v / p.K : *dst + v / p.K;
    }
}

}  // namespace vet

namespace vh {

namespace {

// bytes a chunk of rows may take in the workspace: the P rows and the per-(row, viewer) statistics
constexpr size_t kCrowdBudget = (size_t)256 << 20;

const void* crowd_w_kernel(int stride) { return VET_KERNEL_BY_S(vet::k_crowd_w, row_chunk_class(stride)); }

int launch_crowd(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window, int stride,
                 double* d_div, double* d_rows, int32_t* d_samples, int32_t* d_status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const int K = (int)pl->lat.size();
    const long R = (long)vet_window_rows(T, window, stride);
    // ---- what the call refuses, before anything is launched or allocated
    if (R * (long)U >= (1L << 31))
        return fail(VET_ERR_UNSUPPORTED, "crowd divergence: %ld rows x users in one call (fewer than 2^31)", R * (long)U);
    int rc = check_user_dirs_frames(T, "crowd divergence");
    if (rc) return rc;
    rc = check_user_plan(pl, "crowd divergence", s);
    if (rc) return rc;
    WindowFrames wf;
    rc = window_frames_layout(pl, U, T, 0, wf, s);
    if (rc) return rc;
    int n_max = 0;
    for (int k = 0; k < K; ++k) n_max = std::max(n_max, pl->lat[k].n);
    // rows per chunk: the budget pays for a row's P, its log2 table and its U statistics slots
    const size_t slot_b = 3 * sizeof(double) + sizeof(int32_t);
    long CR = c->tune.crowd_divergence_chunk_rows > 0
                  ? c->tune.crowd_divergence_chunk_rows
                  : (long)(kCrowdBudget / (2 * (size_t)n_max * sizeof(double) + (size_t)U * slot_b));
    CR = std::max(1L, std::min({CR, R, ((1L << 31) - 1) / U}));
    // workspace: stage 2's arrays | dirs [U][T] | P [CR][n_max] | log2 p [CR][n_max] | W_r [CR] | row flag [CR] |
    //            D, W_u, S_u [CR][U] | flag [CR][U]
    WsLayout lay{wf.bytes};
    const size_t dirs_o = lay.take<int32_t>((size_t)U * T), P_o = lay.take<double>((size_t)CR * n_max),
                 logp_o = lay.take<double>((size_t)CR * n_max), Wr_o = lay.take<double>((size_t)CR),
                 rflag_o = lay.take<int32_t>((size_t)CR), div_o = lay.take<double>((size_t)CR * U),
                 tot_o = lay.take<double>((size_t)CR * U), own_o = lay.take<double>((size_t)CR * U),
                 uflag_o = lay.take<int32_t>((size_t)CR * U);
    rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    int32_t* dirs = (int32_t*)(ws + dirs_o);
    double *P = (double*)(ws + P_o), *logp = (double*)(ws + logp_o), *Wr = (double*)(ws + Wr_o);
    int32_t* rflag = (int32_t*)(ws + rflag_o);
    const vet::CrowdStats st{(double*)(ws + div_o), (double*)(ws + tot_o), (double*)(ws + own_o), (int32_t*)(ws + uflag_o)};
    const vet::CrowdRows in{{P, Wr, rflag}, logp};
    // ---- stage 1
    rc = user_dirs_run(pl, d_mu, d_mv, d_ids, U, T, dirs, d_status, "crowd divergence", s);
    if (rc) return rc;
    // ---- stage 2 (charged as vet_spatial_entropy_windowed's); a null status: stage 1 has counted the bad samples
    rc = window_frames_run(pl, d_mu, d_mv, d_ids, U, T, wf, nullptr, s);
    if (rc) return rc;
    for (long r0 = 0; r0 < R; r0 += CR) {
        const long cr = std::min(CR, R - r0);
        for (int k = 0; k < K; ++k) {
            const Lattice& L = pl->lat[k];
            // ---- stage 3, charged to k_finalize
            rc = window_hist_run(pl, k, U, wf, window, stride, r0, r0 + cr, r0, P, Wr, rflag, nullptr, nullptr, s);
            if (rc) return rc;
            {
                const long cells = cr * (long)L.n;
                ProfScope ps(c, s, KID_FINALIZE);
                hipLaunchKernelGGL(vet::k_crowd_logp, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, (const double*)P,
                                   (const double*)Wr, logp, L.n, cells);
                HIP_TRY(hipGetLastError());
            }
            vet::CrowdOut o{};
            o.st = st; o.out = d_div; o.samples = k == 0 ? d_samples : nullptr; o.status = k == 0 ? d_status : nullptr;
            o.R = R; o.r0 = r0; o.U = U; o.first = k == 0; o.K = (double)K;
            {   // ---- stage 4, charged to k_transition: the one profile id the call does not use otherwise, so that the
                // (row, viewer) stage can be told from stage 2's gather
                ProfScope ps(c, s, KID_TRANSITION);
                if (counts_lattice(pl, k)) {
                    vet::CrowdCParams q{};
                    q.dirs = dirs; q.T = T; q.nearest = L.d_nearest; q.n = L.n; q.window = window; q.stride = stride;
                    q.in = in; q.o = o;
                    hipLaunchKernelGGL(vet::k_crowd_c, dim3((unsigned)(cr * U)), dim3(vet::WAVE), (size_t)L.n * 4, s, q);
                } else {
                    vet::CrowdWParams q{};
                    q.dirs = dirs; q.T = T; q.alias = pl->d_alias; q.X = exact_rows_arg(pl, k);
                    q.window = window; q.stride = stride; q.in = in; q.o = o;
                    const int nw = user_nw(c->lds_max, L.n, window);
                    void* args[] = {(void*)&q};
                    HIP_TRY(hipLaunchKernel(crowd_w_kernel(q.X.stride), dim3((unsigned)(cr * U)), dim3(nw * vet::WAVE), args,
                                            vet::dtable_lds_bytes(nw, L.n), s));
                }
                HIP_TRY(hipGetLastError());
            }
            if (d_rows) {   // ---- stage 5, charged to k_finalize
                vet::CrowdRowsParams q{};
                q.in = in; q.st = st; q.U = U; q.n = L.n; q.R = R; q.r0 = r0; q.cr = cr; q.first = k == 0; q.K = (double)K;
                q.rows = d_rows;
                ProfScope ps(c, s, KID_FINALIZE);
                hipLaunchKernelGGL(vet::k_crowd_rows, dim3((unsigned)((cr + 3) / 4)), dim3(4 * vet::WAVE), 0, s, q);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    return VET_OK;
}

}  // namespace

int crowd_set_attrs(vet_ctx* c) {
    for (int stride : {64, 128, 256, 512})
        HIP_TRY(hipFuncSetAttribute(crowd_w_kernel(stride), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_max));
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_crowd_c, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_max));
    return VET_OK;
}

}  // namespace vh

using namespace vh;

extern "C" {

int vet_crowd_divergence(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, double* d_div,
                         double* d_rows, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_args(pl, U, T, window, stride, d_div);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_crowd_divergence_ids", stream, &s);
    return rc ? rc : launch_crowd(pl, d_mu, d_mv, nullptr, U, T, window, stride, d_div, d_rows, d_samples, d_status, s);
}

int vet_crowd_divergence_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, double* d_div,
                             double* d_rows, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_args(pl, U, T, window, stride, d_div);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_crowd(pl, nullptr, nullptr, d_ids, U, T, window, stride, d_div, d_rows, d_samples, d_status, s);
}

}  // extern "C"
