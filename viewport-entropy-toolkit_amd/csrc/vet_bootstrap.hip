// vet_bootstrap.hip — bootstrap confidence bands over viewers behind vet_bootstrap_entropy* (include/vet.h): the kernels and their
// launch logic.  Viewers are the independent unit: replicate b resamples the audience with replacement (c[b][u] = how often the
// draw picked viewer u, sum_u c[b][u] = U; the same resample for every row and lattice: a viewer's trajectory stays together) and
// row r of the replicate is the reference's compute_spatial_entropy (naive plans: compute_naive_spatial_entropy) on ONE dict that
// holds the row's present samples of every drawn viewer, a viewer drawn c times entered c times.  Its histogram is
//     H_b = sum_u c[b][u] * h_u,   h_u = viewer u's own row histogram (vet_user_entropy's d_weights),
// so the B replicate histograms of a row are the [B x U] . [U x n] FP64 matrix product of the counts with the viewers' histograms:
// the one dense contraction of the engine, on the FP64 matrix unit (v_mfma_f64_16x16x4_f64).
// Stages, rows in chunks so that the workspace stays bounded whatever R is:
//   1  k_user_dirs (vet_user_dirs.hpp, unchanged): direction ids transposed once, dirs[U][T];
//   2  k_bootstrap_counts: c[B][U] u16 from the draw of include/vet.h, integer atomics (exact in any order);
//   3  per lattice and chunk of rows, k_user_hist_w/_c (vet_user_divergence.hip: user_hist_run, unchanged): hist [rows][U][n] f64,
//      tot and flag; weighted lattices then k_bootstrap_zero_keys: for the flagged (row, viewer) slots only, the tiles that are keys
//      of the viewer with the value 0.0 (power_factor underflow), as a bit mask — k_user_hist_w writes +0.0 for those and for
//      "no key" alike;
//   4  k_bootstrap_gemm: one workgroup per (row, block of 16 replicates): the product into LDS, then the entropy epilogue of the
//      row calls (row_total / row_entropy, vet_row_hist.hpp) per replicate; lattice 0 stores value / K, later lattices add;
//   5  k_bootstrap_summary: one workgroup per row sorts the finite replicates in LDS and takes mean, sd and the two quantiles.
// A replicate's bits depend on the plan, the window, the row's frames, U, seed and b only: the histograms are vet_user_entropy's
// (pure), a replicate's tile sums run over the viewers in ascending blocks of four into one accumulator whatever B, the row chunk
// or the launch, and the order inside one 16x16x4 MFMA is the hardware's, fixed.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_user_dirs.hpp"
#include "vet_row_hist.hpp"
#include "vet_rank.hpp"

#include <algorithm>

namespace vet {

constexpr int BOOT_RB = 16;           // replicates per workgroup of k_bootstrap_gemm: the M of the 16x16x4 MFMA
constexpr int BOOT_NT = 4;            // column blocks a wave of k_bootstrap_gemm holds accumulators for at a time
constexpr int BOOT_MAX_B = 4096;      // replicates of a call: k_bootstrap_summary sorts them in LDS

// ------------------------------------------------------------------------------------------
// k_bootstrap_counts — stage 2.  One thread per draw (b, j): the SplitMix64 finaliser of seed + (b U + j + 1) * golden ratio, the
// viewer = high 32 bits * U >> 32, and c[b][viewer] += 1.  The u16 counts are packed two to a dword (a count is at most
// U <= 65535: no carry into the neighbour); the array is zeroed by the host before the launch.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bootstrap_counts(unsigned* c32, int U, long draws, unsigned long long seed) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;    // b * U + j
    if (i >= draws) return;
    unsigned long long z = seed + (unsigned long long)(i + 1) * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    const unsigned long long viewer = ((z >> 32) * (unsigned long long)U) >> 32;
    const long e = (i / U) * U + (long)viewer;
    atomicAdd(&c32[e >> 1], 1u << (16 * (int)(e & 1)));
}

// ------------------------------------------------------------------------------------------
// k_bootstrap_zero_keys — stage 3 of a weighted Fibonacci lattice, behind k_user_hist_w.  One wave per (row, viewer) slot of the
// chunk; a slot whose flag is 0 (the common case) leaves at once.  A flagged slot walks the exact rows of the viewer's present
// frames of the row and marks every entry's tile whose histogram value is 0.0: the keys of the viewer's dict whose value is 0.0.
// zmask [slot][zw] u32 (written for flagged slots only), zflag[slot] = whether any bit is set (written for every slot).
// LDS: u32 [zw].
// ------------------------------------------------------------------------------------------
struct BootZeroParams {
    const int32_t* dirs;         // [U][T]
    int T, U;
    const uint32_t* alias;       // [n_dirs] direction -> row | mirrored << 31
    ExactRows X;
    int window, stride;
    long r0;                     // first row of the chunk
    const double* hist;          // [CR][U][n]
    const int32_t* flag;         // [CR][U]
    uint32_t* zmask;             // [CR][U][zw]
    int32_t* zflag;              // [CR][U]
    int zw;                      // ceil(n / 32)
};

__global__ __launch_bounds__(64) void k_bootstrap_zero_keys(const BootZeroParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* m = (unsigned*)smem;
    const int lane = lane_id(), n = p.X.n;
    const long slot = blockIdx.x, rc = slot / p.U, u = slot - rc * p.U, r = p.r0 + rc;
    if (!p.flag[slot]) {
        if (lane == 0) p.zflag[slot] = 0;
        return;
    }
    for (int w = lane; w < p.zw; w += WAVE) m[w] = 0u;
    __syncthreads();
    const int32_t* d = p.dirs + u * (long)p.T + r * (long)p.stride;
    const double* h = p.hist + slot * (long)n;
    for (int j = 0; j < p.window; ++j) {
        const int id = d[j];
        if (id < 0) continue;
        const uint32_t a = p.alias[id];
        const int row = (int)(a & 0x7FFFFFFFu), mir = (int)(a >> 31), ln = (int)p.X.len[row];
        const size_t base = (size_t)row * (size_t)p.X.stride;
        for (int e = lane; e < ln; e += WAVE) {
            int t = (int)p.X.idx[base + e];
            if (mir) t = n - 1 - t;
            if (h[t] == 0.0) atomicOr(&m[t >> 5], 1u << (t & 31));
        }
    }
    __syncthreads();
    unsigned any = 0u;
    for (int w = lane; w < p.zw; w += WAVE) {
        const unsigned v = m[w];
        p.zmask[slot * (long)p.zw + w] = v;
        any |= v;
    }
    const bool some = __ballot(any != 0u) != 0ull;
    if (lane == 0) p.zflag[slot] = some ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// k_bootstrap_gemm — stage 4.  Workgroup (x, y): row y of the chunk, replicates [16 x, 16 x + 16); 256 threads = 4 waves.
// Product: wave w takes the 16-tile column blocks w, w + 4, ... (four of them at a time); for each it runs the whole K loop over
// the viewers in ascending blocks of four into ONE accumulator with v_mfma_f64_16x16x4_f64 (no split-K, no atomics):
//     A[i = lane & 15][k = lane >> 4] = (double)c[b0 + i][u0 + k]        B[k = lane >> 4][j = lane & 15] = hist[u0 + k][t0 + j]
//     D: col = lane & 15, row = (lane >> 4) + 4 * reg   (the f64 form's own map, not the f32 one)
// with the edges predicated to 0.0 (U not a multiple of 4, n not a multiple of 16, B not a multiple of 16), and leaves the 16 x n
// block in LDS.  Counts and histogram values are read straight from global memory: a row's U x n histograms are shared by the
// B / 16 workgroups of the row through L2, the 16 x U counts by the row's column blocks through L1.
// Epilogue: wave w takes replicates 4 w .. 4 w + 3: a tile is a key iff its sum is > 0.0 (values are >= 0), W = row_total,
// S = row_entropy (q = 0 by underflow gives the reference's NaN by itself), the normaliser k_user_entropy_w's (weighted: hmax) or
// count_row_entropy's (counts: log2(n) if full_norm or W > norm_n, else log2(W)), NaN where W is not > 0 (nobody drawn has a
// sample, or every key is 0.0).  Zero-key rule: only where the row has a slot with zflag set, the replicate is NaN iff a marked
// tile of a drawn viewer sums to 0.0.  Output rep[row][b]: `first` stores value / K, later lattices add; lattice 0 may also
// leave the block as weights[row][b][n] (plain values, +0.0 = no weight).
// LDS: f64 [16][n] dynamic.
// ------------------------------------------------------------------------------------------
typedef double boot_v4d __attribute__((ext_vector_type(4)));

struct BootGemmParams {
    const double* hist;          // [CR][U][n]
    const int32_t* zflag;        // [CR][U], null for counting lattices
    const uint32_t* zmask;       // [CR][U][zw]
    const uint16_t* counts;      // [B][U]
    int U, n, B, zw;
    double hmax;
    int norm_n, full_norm, counting;
    int first;                   // lattice 0: store; later lattices: add
    double K;                    // lattices of the plan
    double* rep;                 // [CR][B], the chunk's first row
    double* weights;             // [CR][B][n], the chunk's first row, or null
};

__global__ __launch_bounds__(256) void k_bootstrap_gemm(const BootGemmParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* S = (double*)smem;                                     // [16][n]
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int n = p.n, U = p.U;
    const long rc = blockIdx.y;
    const int b0 = (int)blockIdx.x * BOOT_RB;
    const double* H = p.hist + rc * (long)U * n;
    {
        const int i = lane & 15, kk = lane >> 4;
        const bool row_ok = b0 + i < p.B;
        const uint16_t* crow = p.counts + (long)(row_ok ? b0 + i : 0) * U;
        const int ntb = (n + 15) >> 4;
        // BOOT_NT of the wave's column blocks at a time (w, w + 4, w + 8, w + 12; then 16 further on): one load of the A operand
        // serves four MFMAs, and four independent accumulators hide the MFMA's own latency.  Two K blocks per trip: the ten loads
        // are issued before the first MFMA; a K block beyond U adds 0.0 * 0.0.  Every accumulator still sees its K blocks in
        // ascending order, whatever the grouping.
        for (int tb0 = wv; tb0 < ntb; tb0 += 4 * BOOT_NT) {
            int t[BOOT_NT];
            bool col_ok[BOOT_NT];
            boot_v4d acc[BOOT_NT];
#pragma unroll
            for (int j = 0; j < BOOT_NT; ++j) {
                t[j] = (tb0 + 4 * j) * 16 + i;
                col_ok[j] = t[j] < n;
                acc[j] = boot_v4d{0.0, 0.0, 0.0, 0.0};
            }
            for (int u0 = 0; u0 < U; u0 += 8) {
                double a[2], b[2][BOOT_NT];
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const int u = u0 + 4 * s2 + kk;
                    const bool ok = u < U;
                    a[s2] = (ok && row_ok) ? (double)crow[u] : 0.0;
#pragma unroll
                    for (int j = 0; j < BOOT_NT; ++j) b[s2][j] = (ok && col_ok[j]) ? H[(long)u * n + t[j]] : 0.0;
                }
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                    for (int j = 0; j < BOOT_NT; ++j)
                        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s2], b[s2][j], acc[j], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < BOOT_NT; ++j)
                if (col_ok[j]) {
                    S[(kk + 0) * (long)n + t[j]] = acc[j][0];
                    S[(kk + 4) * (long)n + t[j]] = acc[j][1];
                    S[(kk + 8) * (long)n + t[j]] = acc[j][2];
                    S[(kk + 12) * (long)n + t[j]] = acc[j][3];
                }
        }
    }
    // whether any slot of the row carries zero-valued keys (weighted lattices; every thread takes part in the barrier)
    int any_z = 0;
    if (p.zflag)
        for (int u = tid; u < U; u += 256) any_z |= p.zflag[rc * (long)U + u];
    any_z = __syncthreads_or(any_z);                               // also: the block is complete in LDS
    if (p.weights) {
        const int live = min(BOOT_RB, p.B - b0);
        double* out = p.weights + (rc * (long)p.B + b0) * (long)n;
        for (long i = tid; i < (long)live * n; i += 256) __builtin_nontemporal_store(S[i], out + i);
    }
    for (int q = 0; q < 4; ++q) {
        const int ii = wv * 4 + q, b = b0 + ii;
        if (b >= p.B) break;
        const double* Sr = S + (long)ii * n;
        const auto keys = [&](int t, double& v) {
            v = Sr[t];
            return v > 0.0;
        };
        const double tot = row_total(n, keys);
        const double hh = row_entropy(n, tot, keys);
        bool bad = false;
        if (any_z) {
            const uint16_t* crow = p.counts + (long)b * U;
            for (int u0 = 0; u0 < U; u0 += WAVE) {
                const int u = u0 + lane;
                const bool f = u < U && p.zflag[rc * (long)U + u] != 0 && crow[u] != 0;
                unsigned long long who = __ballot(f);
                while (who) {
                    const int j = __ffsll((long long)who) - 1;
                    who &= who - 1ull;
                    const uint32_t* zm = p.zmask + (rc * (long)U + u0 + j) * (long)p.zw;
                    for (int w = lane; w < p.zw; w += WAVE) {
                        unsigned bits = zm[w];
                        while (bits) {
                            const int t = w * 32 + __ffs((int)bits) - 1;
                            bits &= bits - 1u;
                            bad |= Sr[t] == 0.0;
                        }
                    }
                }
            }
            bad = __ballot(bad) != 0ull;
        }
        if (lane == 0) {
            double hmax = p.hmax;
            if (p.counting && !(tot > (double)p.norm_n) && !p.full_norm) hmax = -tot * (1.0 / tot) * -log2(tot);
            double e = hh / hmax;
            if (!(tot > 0.0) || bad) e = __builtin_nan("");
            double* dst = p.rep + rc * (long)p.B + b;
            *dst = p.first ? e / p.K : *dst + e / p.K;
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_bootstrap_summary — stage 5.  One workgroup per row: rep[r][0 .. B) to LDS, everything that is not finite replaced by +inf
// (so are the slots up to the next power of two), a bitonic sort (vet_rank.hpp), then wave 0 over the m finite values in ascending order:
// mean and the two-pass sd (ddof = 1) in lane order + wave_sum, and the quantiles q by linear interpolation between the order
// statistics at position q (m - 1): x[i] + (x[i + 1] - x[i]) g.  m = 0: NaN for all four; m = 1: sd NaN.
// LDS: f64 [4096] static.
// ------------------------------------------------------------------------------------------
struct BootSummaryParams {
    const double* rep;           // [R][B]
    int B;
    long R;
    double q_lo, q_hi;
    double* summary;             // [4][R] mean, sd, lo, hi
    int32_t* valid;              // [R] or null
};

__global__ __launch_bounds__(256) void k_bootstrap_summary(const BootSummaryParams p) {
    __shared__ double x[BOOT_MAX_B];
    __shared__ int m_s;
    const int tid = threadIdx.x, lane = lane_id();
    const long r = blockIdx.x;
    int P = 1;
    while (P < p.B) P <<= 1;
    if (tid == 0) m_s = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < P; i += 256) {
        double v = __builtin_inf();
        if (i < p.B) {
            const double w = p.rep[r * p.B + i];
            if (isfinite(w)) { v = w; ++mine; }
        }
        x[i] = v;
    }
    if (mine) atomicAdd(&m_s, mine);
    lds_bitonic_sort(x, P);
    if (wave_id() != 0) return;
    const int m = m_s;
    double s = 0.0;
    for (int i = lane; i < m; i += WAVE) s += x[i];
    s = wave_sum(s);
    const double mean = s / (double)m;
    double ss = 0.0;
    for (int i = lane; i < m; i += WAVE) {
        const double d = x[i] - mean;
        ss += d * d;
    }
    ss = wave_sum(ss);
    if (lane == 0) {
        const double nan = __builtin_nan("");
        p.summary[0 * p.R + r] = m ? mean : nan;
        p.summary[1 * p.R + r] = m >= 2 ? sqrt(ss / (double)(m - 1)) : nan;
        p.summary[2 * p.R + r] = m ? lerp_quantile(x, m, p.q_lo) : nan;
        p.summary[3 * p.R + r] = m ? lerp_quantile(x, m, p.q_hi) : nan;
        if (p.valid) p.valid[r] = m;
    }
}

}  // namespace vet

namespace vh {

namespace {

constexpr size_t kBootHistBudget = (size_t)256 << 20;     // bytes of histograms a chunk of rows may take in the workspace

size_t gemm_lds_bytes(int n) { return (size_t)vet::BOOT_RB * n * sizeof(double); }

// c[B][U] u16 at `counts` (16-byte aligned, room for an even number of entries), on s; charged to k_finalize
int bootstrap_counts_run(vet_ctx* c, int U, int B, uint64_t seed, uint16_t* counts, hipStream_t s) {
    const long draws = (long)B * U;
    HIP_TRY(hipMemsetAsync(counts, 0, (size_t)((draws + 1) & ~1L) * sizeof(uint16_t), s));
    ProfScope ps(c, s, KID_FINALIZE);
    hipLaunchKernelGGL(vet::k_bootstrap_counts, dim3((unsigned)((draws + 255) / 256)), dim3(256), 0, s, (unsigned*)counts, U, draws,
                       (unsigned long long)seed);
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

int launch_bootstrap(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window, int stride,
                     int B, uint64_t seed, double confidence, double* d_summary, double* d_replicates, double* d_weights,
                     int32_t* d_valid, int32_t* d_status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const int K = (int)pl->lat.size();
    const long R = (long)vet_window_rows(T, window, stride);
    // ---- what the call refuses, before anything is launched or allocated
    int rc = check_bootstrap_args(pl, U, B, confidence);
    if (rc) return rc;
    if (R * (long)U >= (1L << 31))
        return fail(VET_ERR_UNSUPPORTED, "bootstrap: %ld rows x users in one call (fewer than 2^31)", R * (long)U);
    rc = check_user_dirs_frames(T, "bootstrap");
    if (rc) return rc;
    rc = check_user_plan(pl, "bootstrap", s);
    if (rc) return rc;
    int n_max = 0;
    for (int k = 0; k < K; ++k) n_max = std::max(n_max, pl->lat[k].n);
    const int zw_max = (n_max + 31) / 32;
    // rows per chunk: the histogram budget, the y extent of the product's launch and the x extent of the histogram launch
    long CR = c->tune.bootstrap_chunk_rows > 0 ? c->tune.bootstrap_chunk_rows
                                               : (long)(kBootHistBudget / ((size_t)U * n_max * sizeof(double)));
    CR = std::max(1L, std::min({CR, R, 65535L, ((1L << 31) - 1) / U}));
    // workspace: dirs [U][T] | counts [B][U] u16 | hist [CR][U][n_max] | tot [CR][U] | flag [CR][U] | zmask [CR][U][zw] |
    //            zflag [CR][U] | rep [R][B] where the caller does not take the replicates
    WsLayout lay;
    const size_t dirs_o = lay.take<int32_t>((size_t)U * T), cnt_o = lay.take<uint16_t>((size_t)B * U + 1),
                 hist_o = lay.take<double>((size_t)CR * U * n_max), tot_o = lay.take<double>((size_t)CR * U),
                 flag_o = lay.take<int32_t>((size_t)CR * U), zmask_o = lay.take<uint32_t>((size_t)CR * U * zw_max),
                 zflag_o = lay.take<int32_t>((size_t)CR * U), rep_o = lay.take<double>(d_replicates ? 0 : (size_t)R * B);
    rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    int32_t* dirs = (int32_t*)(ws + dirs_o);
    uint16_t* counts = (uint16_t*)(ws + cnt_o);
    double *hist = (double*)(ws + hist_o), *tot = (double*)(ws + tot_o);
    int32_t *flag = (int32_t*)(ws + flag_o), *zflag = (int32_t*)(ws + zflag_o);
    uint32_t* zmask = (uint32_t*)(ws + zmask_o);
    double* rep = d_replicates ? d_replicates : (double*)(ws + rep_o);
    // ---- stage 1 and 2
    rc = user_dirs_run(pl, d_mu, d_mv, d_ids, U, T, dirs, d_status, "bootstrap", s);
    if (rc) return rc;
    rc = bootstrap_counts_run(c, U, B, seed, counts, s);
    if (rc) return rc;
    const unsigned bblocks = (unsigned)((B + vet::BOOT_RB - 1) / vet::BOOT_RB);
    for (long r0 = 0; r0 < R; r0 += CR) {
        const long cr = std::min(CR, R - r0);
        for (int k = 0; k < K; ++k) {
            const Lattice& L = pl->lat[k];
            const bool counting = counts_lattice(pl, k);
            // ---- stage 3; the bootstrap has no per-viewer outputs: no samples, and status[1] stays as it is
            rc = user_hist_run(pl, k, dirs, U, T, window, stride, R, r0, cr, hist, tot, flag, nullptr, nullptr, s);
            if (rc) return rc;
            const int zw = (L.n + 31) / 32;
            if (!counting) {
                rc = zero_keys_run(pl, k, dirs, U, T, window, stride, r0, cr, hist, flag, zmask, zflag, s);
                if (rc) return rc;
            }
            {   // ---- stage 4, charged to k_transition: the one profile id the call does not use otherwise, so that the product
                // can be told from the histogram walk
                vet::BootGemmParams q{};
                q.hist = hist; q.zflag = counting ? nullptr : zflag; q.zmask = zmask; q.counts = counts;
                q.U = U; q.n = L.n; q.B = B; q.zw = zw; q.hmax = L.hmax;
                q.norm_n = L.norm_n; q.full_norm = (L.binned && pl->weighted) ? 1 : 0; q.counting = counting ? 1 : 0;
                q.first = k == 0; q.K = (double)K;
                q.rep = rep + (size_t)r0 * B;
                q.weights = (k == 0 && d_weights) ? d_weights + (size_t)r0 * B * L.n : nullptr;
                ProfScope ps(c, s, KID_TRANSITION);
                hipLaunchKernelGGL(vet::k_bootstrap_gemm, dim3(bblocks, (unsigned)cr), dim3(256), gemm_lds_bytes(L.n), s, q);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    {   // ---- stage 5, charged to k_finalize
        vet::BootSummaryParams q{};
        q.rep = rep; q.B = B; q.R = R;
        q.q_lo = (1.0 - confidence) / 2.0; q.q_hi = 1.0 - (1.0 - confidence) / 2.0;
        q.summary = d_summary; q.valid = d_valid;
        ProfScope ps(c, s, KID_FINALIZE);
        hipLaunchKernelGGL(vet::k_bootstrap_summary, dim3((unsigned)R), dim3(256), 0, s, q);
        HIP_TRY(hipGetLastError());
    }
    return VET_OK;
}

}  // namespace

int zero_keys_run(vet_plan* pl, int k, const int32_t* dirs, int U, int T, int window, int stride, long r0, long cr, const double* hist,
                  const int32_t* flag, uint32_t* zmask, int32_t* zflag, hipStream_t s) {
    vet::BootZeroParams q{};
    q.dirs = dirs; q.T = T; q.U = U; q.alias = pl->d_alias; q.X = exact_rows_arg(pl, k);
    q.window = window; q.stride = stride; q.r0 = r0; q.hist = hist; q.flag = flag; q.zmask = zmask; q.zflag = zflag;
    q.zw = (pl->lat[k].n + 31) / 32;
    ProfScope ps(pl->ctx, s, KID_FINALIZE);
    hipLaunchKernelGGL(vet::k_bootstrap_zero_keys, dim3((unsigned)(cr * U)), dim3(vet::WAVE), (size_t)q.zw * 4, s, q);
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

int check_bootstrap_args(const vet_plan* pl, int U, int replicates, double confidence) {
    if (replicates < 1 || replicates > vet::BOOT_MAX_B)
        return fail(VET_ERR_INVALID, "replicates must be between 1 and %d (got %d)", vet::BOOT_MAX_B, replicates);
    if (!(confidence > 0.0 && confidence < 1.0))
        return fail(VET_ERR_INVALID, "confidence must be inside (0, 1) (got %g)", confidence);
    if (U > 65535) return fail(VET_ERR_UNSUPPORTED, "bootstrap: %d users (the resample counts are 16-bit: at most 65535)", U);
    for (const Lattice& L : pl->lat)
        if (gemm_lds_bytes(L.n) > kWholeLds)
            return fail(VET_ERR_UNSUPPORTED, "bootstrap: 16 replicate histograms of %d tiles do not fit the LDS (at most %zu tiles)",
                        L.n, kWholeLds / gemm_lds_bytes(1));
    return VET_OK;
}

int bootstrap_set_attrs(vet_ctx* c) {
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_bootstrap_gemm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWholeLds));
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_bootstrap_zero_keys, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_max));
    return VET_OK;
}

}  // namespace vh

using namespace vh;

extern "C" {

int vet_bootstrap_entropy(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, int replicates,
                          uint64_t seed, double confidence, double* d_summary, double* d_replicates, double* d_weights,
                          int32_t* d_valid, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_args(pl, U, T, window, stride, d_summary);
    if (!rc) rc = check_bootstrap_args(pl, U, replicates, confidence);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_bootstrap_entropy_ids", stream, &s);
    return rc ? rc : launch_bootstrap(pl, d_mu, d_mv, nullptr, U, T, window, stride, replicates, seed, confidence, d_summary,
                                      d_replicates, d_weights, d_valid, d_status, s);
}

int vet_bootstrap_entropy_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, int replicates, uint64_t seed,
                              double confidence, double* d_summary, double* d_replicates, double* d_weights, int32_t* d_valid,
                              int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_args(pl, U, T, window, stride, d_summary);
    if (!rc) rc = check_bootstrap_args(pl, U, replicates, confidence);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_bootstrap(pl, nullptr, nullptr, d_ids, U, T, window, stride, replicates, seed, confidence, d_summary,
                                      d_replicates, d_weights, d_valid, d_status, s);
}

int vet_bootstrap_counts_host(vet_plan* pl, int U, int replicates, uint64_t seed, uint16_t* h_counts) {
    if (!pl || !h_counts) return fail(VET_ERR_INVALID, "plan or h_counts is NULL");
    if (U < 1) return fail(VET_ERR_INVALID, "n_users must be at least 1 (got %d)", U);
    int rc = check_bootstrap_args(pl, U, replicates, 0.5);
    if (rc) return rc;
    vet_ctx* c = pl->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const size_t entries = (size_t)replicates * U;
    rc = ensure_ws(c, pad16((entries + 1) * sizeof(uint16_t)));
    if (rc) return rc;
    rc = bootstrap_counts_run(c, U, replicates, seed, (uint16_t*)c->ws, c->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h_counts, c->ws, entries * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VET_OK;
}

}  // extern "C"
