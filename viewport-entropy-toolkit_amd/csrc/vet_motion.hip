// vet_motion.hip — head-motion statistics behind vet_head_motion* (include/vet.h): the kernels and their launch logic.  A video of T
// frames has P = T - lag pairs, pair f = (frame f, frame f + lag); a (pair, viewer) present in both frames is a sample, its angle a
// the reference's vector_angle_distance of the two Vectors in radians (k_angular_distances' arithmetic on the plan's unit table),
// +0.0 exactly where the two Vectors are the same.  Lattice-independent: only the direction table is read.
// Stage 1, k_motion_angles: one FP64 angle per (pair, viewer), NaN = absent; [P][U] for the pooled layout, [U][P] behind
// k_user_dirs for the per-viewer layout, so that in both layouts a row is a contiguous slice of W values (W = window * U, or window).
// Stage 2, the shape chosen from W alone (and the test bound vet_test_motion_lds_values):
//   W <= 64      k_motion_wave: one wave per row, four rows per workgroup, persistent over the rows; sums by wave_sum, the bit
//                patterns sorted across the lanes by shuffles;
//   W <= 16384   k_motion_rows: one workgroup per row, persistent over the rows; two walks over the slice (sums, then squared
//                deviations), the bit patterns sorted in LDS (lds_bitonic_sort; non-negative doubles order as their u64 bits), the
//                quantiles read off the sorted array;
//   W >  16384   the row is cut into chunks of 16384 values, one workgroup each (k_motion_chunk), rows in passes under the workspace
//                budget.  Pass 0 takes the sums, counts, the maximum and the edge histogram; k_motion_select combines the partial
//                sums in order.  The order statistics come from a most-significant-digit-first radix selection of the u64 bit
//                patterns: eight passes of eight bits, each a walk over the row that counts — for every distinct prefix the wanted
//                ranks still share, at most 16 — the next digit of the values under that prefix (LDS integer histograms, then integer
//                atomicAdd into the workspace); k_motion_select then narrows each rank to its digit.  After the eighth pass a rank's
//                prefix is the value itself: exact, ties included, nothing is sorted or sampled.  Pass 1 also takes the squared
//                deviations.
// FP sums, one rule for both shapes: the slice is cut into blocks of 1024 values from its start; in a block thread t adds its
// positions t, t + 256, t + 512, t + 768 in that order, wave_sum's butterfly, the four waves in order; the blocks are added in
// ascending order.  Counts, the maximum (an integer maximum of bit patterns) and the histograms are exact in any order.  No FP atomics.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_angle.hpp"
#include "vet_rank.hpp"

#include <algorithm>
#include <cmath>

namespace vet {

constexpr int MO_THREADS = 256;
constexpr int MO_BLOCK = 1024;          // values of one block of the summation rule: four per thread
constexpr int MO_LDS_VALUES = 16384;    // one-workgroup rows: 128 KB of sorted bit patterns; also the chunk of the longer rows
constexpr int MO_BLOCKS = MO_LDS_VALUES / MO_BLOCK;
constexpr int MO_MAX_Q = 8;
constexpr int MO_TARGETS = 2 * MO_MAX_Q;   // two order statistics per fraction
constexpr int MO_MAX_BINS = 64;
constexpr int MO_PASSES = 8;            // digits of eight bits
constexpr unsigned long long MO_ABSENT = ~0ull;

// ------------------------------------------------------------------------------------------
// k_motion_angles — stage 1.  MODE 0: (mu, mv) quantised by sample_dir, 1: ids, both [T][U] -> angles [P][U]; 2: dirs [U][T]
// (k_user_dirs) -> angles [U][P].  One thread per output in a grid-stride loop: consecutive threads read consecutive samples of
// both frames and write consecutive angles.  The two unit vectors are gathered from the table (L2-resident at the reference grid);
// ids that differ compare the raw Vectors only when the cosine is near 1 (motion_angle, vet_angle.hpp).  status[0] counts a sample outside [0, 1] once: as the
// earlier frame of its pair, or as the later frame where it is the earlier frame of none.
// ------------------------------------------------------------------------------------------
struct MotionAnglesParams {
    SampleSrc src;
    const int32_t* dirs;         // [U][T], MODE 2
    const double* unit;          // [n_dirs][3]
    const double* raw;           // [n_dirs][3]
    int U, T, lag;
    long P;
    double* angles;
    int32_t* status;             // [2] or null
};

template <int MODE>
__global__ __launch_bounds__(MO_THREADS) void k_motion_angles(const MotionAnglesParams p) {
    const long total = p.P * (long)p.U;
    bool bad = false;
    for (long i = blockIdx.x * (long)MO_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * MO_THREADS) {
        int ia, ib;
        if (MODE == 2) {
            const long u = i / p.P, f = i - u * p.P;
            const int32_t* d = p.dirs + u * (long)p.T + f;
            ia = d[0]; ib = d[p.lag];
        } else {
            bool bad_b = false;
            const long j = i + (long)p.lag * p.U;
            ia = sample_dir<MODE == 1>(p.src, i, bad);
            ib = sample_dir<MODE == 1>(p.src, j, bad_b);
            if (j >= total) bad |= bad_b;
        }
        p.angles[i] = motion_angle(ia, ib, p.unit, p.raw);
    }
    if (MODE != 2 && p.status) {
        const unsigned long long anybad = __ballot(bad);
        if (anybad && lane_id() == 0) atomicAdd(&p.status[0], (int)__popcll(anybad));
    }
}

// ------------------------------------------------------------------------------------------
// stage 2, shared by both shapes
// ------------------------------------------------------------------------------------------
struct MotionRows {
    const double* angles;
    long R, P, W;                // rows per viewer (or of the call), pairs, values per row
    int U, stride, per_user;
    long rows;                   // R, or U * R
    int Q, B;
    double q[MO_MAX_Q];
    double edges[MO_MAX_BINS + 1];
    double* stats;               // [4][rows]
    double* quant;               // [rows][Q] or null
    int32_t* hist;               // [rows][B] or null
    int32_t* still;              // [rows] or null
    int32_t* samples;            // [rows] or null
    int32_t* status;             // [2] or null
};

__device__ __forceinline__ const double* mo_row(const MotionRows& g, long row) {
    if (g.per_user) {
        const long u = row / g.R;
        return g.angles + u * g.P + (row - u * g.R) * g.stride;
    }
    return g.angles + row * (long)g.stride * g.U;
}

// lerp_quantile's rule between two order statistics, as one explicit fma so that both shapes give the same bits
__device__ __forceinline__ void mo_rank_of(double q, int N, double& pos, int& i) {
    pos = q * (double)(N - 1);
    i = min((int)floor(pos), N - 1);
}
__device__ __forceinline__ double mo_lerp(double xi, double xj, double pos, int i) {
    return fma(xj - xi, pos - (double)i, xi);
}

__device__ __forceinline__ void mo_write_empty(const MotionRows& g, long row) {
    const double nan = __builtin_nan("");
    for (int k = 0; k < 4; ++k) g.stats[(long)k * g.rows + row] = nan;
    if (g.quant) for (int j = 0; j < g.Q; ++j) g.quant[row * g.Q + j] = nan;
    if (g.still) g.still[row] = 0;
    if (g.samples) g.samples[row] = 0;
    if (g.status) atomicAdd(&g.status[1], 1);
}
__device__ __forceinline__ void mo_write_head(const MotionRows& g, long row, double total, int N, int still, double mx) {
    g.stats[row] = total / (double)N;
    g.stats[2 * g.rows + row] = mx;
    g.stats[3 * g.rows + row] = total;
    if (g.still) g.still[row] = still;
    if (g.samples) g.samples[row] = N;
}
__device__ __forceinline__ double mo_sd(double ss, int N) { return sqrt(ss / (double)(N - 1)); }   // N = 1: 0 / 0 = NaN as numpy

// ------------------------------------------------------------------------------------------
// k_motion_wave — stage 2 for W <= 64 (short per-viewer rows, tiny audiences): one wave per row, four rows per workgroup, persistent
// over the rows; no barrier in the loop.  Lane t holds position t.  The block rule with one block and one busy wave: wave_sum's
// butterfly over the lanes is the row's sum (the other three waves of the rule would add +0.0).  Counts by ballots; the histogram one ballot per bin; the bit patterns sorted across the lanes by a
// bitonic network of 21 shuffle steps; a fraction's two order statistics read by shuffles.
// LDS: the edges only.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MO_THREADS) void k_motion_wave(const MotionRows g) {
    __shared__ double s_edges[MO_MAX_BINS + 1];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int W = (int)g.W;
    for (int i = tid; i <= g.B; i += MO_THREADS) s_edges[i] = g.edges[i];
    __syncthreads();
    for (long row = (long)blockIdx.x * (MO_THREADS / WAVE) + wv; row < g.rows; row += (long)gridDim.x * (MO_THREADS / WAVE)) {
        const double* src = mo_row(g, row);
        const double a = lane < W ? src[lane] : __builtin_nan("");
        const bool present = a == a;
        const int N = (int)__popcll(__ballot(present));
        const int still = (int)__popcll(__ballot(present && a == 0.0));
        if (g.hist) {
            const int bin = present ? mo_bin(s_edges, g.B, a) : -1;
            int mine = 0;
            for (int b = 0; b < g.B; ++b) {
                const int cnt = (int)__popcll(__ballot(bin == b));
                if (lane == b) mine = cnt;
            }
            if (lane < g.B) g.hist[row * g.B + lane] = mine;
        }
        if (N == 0) {                                            // uniform over the wave
            if (lane == 0) mo_write_empty(g, row);
            continue;
        }
        double t = 0.0;
        if (present) t += a;
        const double total = wave_sum(t), mx = wave_max(present ? a : 0.0);
        const double mean = total / (double)N;
        double t2 = 0.0;
        if (present) { const double d = a - mean; t2 = fma(d, d, t2); }
        const double ss = wave_sum(t2);
        if (lane == 0) {
            mo_write_head(g, row, total, N, still, mx);
            g.stats[g.rows + row] = mo_sd(ss, N);
        }
        if (g.quant) {
            unsigned long long key = present ? (unsigned long long)__double_as_longlong(a) : MO_ABSENT;
#pragma unroll
            for (int k = 2; k <= WAVE; k <<= 1)
#pragma unroll
                for (int j = k >> 1; j > 0; j >>= 1) {
                    const unsigned long long other = (unsigned long long)__shfl_xor((long long)key, j, WAVE);
                    const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
                    key = take_min ? min(key, other) : max(key, other);
                }
            for (int j = 0; j < g.Q; ++j) {
                double pos; int i;
                mo_rank_of(g.q[j], N, pos, i);
                const double xi = __longlong_as_double(__shfl((long long)key, i, WAVE));
                const double xj = __longlong_as_double(__shfl((long long)key, min(i + 1, N - 1), WAVE));
                if (lane == 0) g.quant[row * g.Q + j] = i >= N - 1 ? xi : mo_lerp(xi, xj, pos, i);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_motion_rows — stage 2 for 64 < W <= 16384.  256 threads; persistent workgroups take rows blockIdx, blockIdx + gridDim, ...
//   a  walk 1, block by block: the sums of a, N, still, the maximum, the edge histogram (LDS integer atomics), the bit patterns to
//      LDS when quantiles are wanted (absent = all ones, and up to Psort);
//   b  thread 0: the blocks in order -> total, mean;
//   c  walk 2: the squared deviations from the mean (fma(d, d, acc) per position), the same block rule -> sd;
//   d  lds_bitonic_sort of the bit patterns; thread j reads fraction j's two order statistics.
// LDS: u64 [Psort] dynamic (quantiles only), Psort the power of two >= W from 256, + about 1.6 KB static.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MO_THREADS) void k_motion_rows(const MotionRows g, const int Psort) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double s_w[MO_BLOCKS][4];
    __shared__ double s_edges[MO_MAX_BINS + 1];
    __shared__ int s_hist[MO_MAX_BINS];
    __shared__ int s_cnt[MO_THREADS / WAVE][2];
    __shared__ double s_mx[MO_THREADS / WAVE];
    __shared__ double s_mean;
    __shared__ int s_N;
    unsigned long long* keys = (unsigned long long*)smem;
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int W = (int)g.W, nblk = (W + MO_BLOCK - 1) / MO_BLOCK;
    const bool sort = g.quant != nullptr;
    for (int i = tid; i <= g.B; i += MO_THREADS) s_edges[i] = g.edges[i];
    for (long row = blockIdx.x; row < g.rows; row += gridDim.x) {
        const double* src = mo_row(g, row);
        if (tid < MO_MAX_BINS) s_hist[tid] = 0;
        __syncthreads();
        int n = 0, st = 0;
        double mx = 0.0;
        for (int b = 0; b < nblk; ++b) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = b * MO_BLOCK + k * MO_THREADS + tid;
                if (q < W) {
                    const double a = src[q];
                    const bool present = a == a;
                    if (present) {
                        t += a; ++n; st += a == 0.0 ? 1 : 0; mx = fmax(mx, a);
                        const int bin = mo_bin(s_edges, g.hist ? g.B : 0, a);
                        if (bin >= 0) atomicAdd(&s_hist[bin], 1);
                    }
                    if (sort) keys[q] = present ? (unsigned long long)__double_as_longlong(a) : MO_ABSENT;
                }
            }
            t = wave_sum(t);
            if (lane == 0) s_w[b][wv] = t;
        }
        if (sort) for (int q = W + tid; q < Psort; q += MO_THREADS) keys[q] = MO_ABSENT;
        n = wave_sum(n); st = wave_sum(st); mx = wave_max(mx);
        if (lane == 0) { s_cnt[wv][0] = n; s_cnt[wv][1] = st; s_mx[wv] = mx; }
        __syncthreads();
        if (tid == 0) {
            int N = 0, still = 0;
            double m = 0.0, total = 0.0;
            for (int w = 0; w < MO_THREADS / WAVE; ++w) { N += s_cnt[w][0]; still += s_cnt[w][1]; m = fmax(m, s_mx[w]); }
            for (int b = 0; b < nblk; ++b) total += mo_block_total(s_w[b]);
            s_N = N;
            s_mean = total / (double)N;
            if (N == 0) mo_write_empty(g, row); else mo_write_head(g, row, total, N, still, m);
        }
        __syncthreads();
        const int N = s_N;
        const double mean = s_mean;
        if (g.hist && tid < g.B) g.hist[row * g.B + tid] = s_hist[tid];
        if (N > 0) {                                             // uniform over the workgroup
            for (int b = 0; b < nblk; ++b) {
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int q = b * MO_BLOCK + k * MO_THREADS + tid;
                    if (q < W) {
                        const double a = src[q];
                        if (a == a) { const double d = a - mean; t = fma(d, d, t); }
                    }
                }
                t = wave_sum(t);
                if (lane == 0) s_w[b][wv] = t;
            }
            __syncthreads();
            if (tid == 0) {
                double ss = 0.0;
                for (int b = 0; b < nblk; ++b) ss += mo_block_total(s_w[b]);
                g.stats[g.rows + row] = mo_sd(ss, N);
            }
            if (sort) {
                lds_bitonic_sort(keys, Psort);
                if (tid < g.Q) {
                    double pos; int i;
                    mo_rank_of(g.q[tid], N, pos, i);
                    const double xi = __longlong_as_double((long long)keys[i]);
                    const double xj = __longlong_as_double((long long)keys[min(i + 1, N - 1)]);
                    g.quant[row * g.Q + tid] = i >= N - 1 ? xi : mo_lerp(xi, xj, pos, i);
                }
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// The chunked shape.  Per row of a pass the workspace holds the blocks' partial sums, the radix histograms [16][256] u32 and a
// MotionSel.  k_motion_chunk<pass>: workgroup (x, y) = chunk x of row r0 + y, `chunk` values (a multiple of 1024, at most 16384).
//   pass 0   walk 1 of k_motion_rows per block -> psum; N, still (integer atomicAdd), the maximum (atomicMax of the bit pattern),
//            the edge histogram (LDS, then integer atomicAdd into the zeroed output); the top digit of every value -> group 0
//   pass p   the values whose top 8 p bits equal a group's prefix count their next digit in the group's histogram; pass 1 also
//            takes walk 2 per block -> pss
// A wave whose lanes all hit one counter adds once.  k_motion_select<pass>, one wave per row: pass 0 combines psum in block order
// (mean, max, total, samples, still) and sets the wanted ranks; every pass narrows each rank to its digit (a serial scan of 256
// counts per rank), zeroes the histograms it read and regroups the ranks by prefix; pass 1 combines pss -> sd; the last pass
// interpolates the quantiles from the two values of each fraction.
// ------------------------------------------------------------------------------------------
struct MotionSel {
    unsigned long long prefix[MO_TARGETS];   // the top bits a rank's value is known to have
    unsigned long long gprefix[MO_TARGETS];  // the distinct prefixes
    unsigned rank[MO_TARGETS];               // the rank among the values under the prefix
    int group[MO_TARGETS];
    unsigned long long maxbits;
    double mean;
    int G, N, still, pad;
};

struct MotionChunkParams {
    MotionRows g;
    long r0;
    int chunk, nblk_row;         // values per chunk, blocks per row
    double* psum;                // [rows of the pass][nblk_row]
    double* pss;
    unsigned* rhist;             // [rows of the pass][16][256]
    MotionSel* sel;              // [rows of the pass]
};

__global__ __launch_bounds__(MO_THREADS) void k_motion_chunk(const MotionChunkParams p, const int pass) {
    __shared__ unsigned s_rh[MO_TARGETS * 256];
    __shared__ unsigned long long s_gp[MO_TARGETS];
    __shared__ double s_w[MO_BLOCKS][4];
    __shared__ double s_edges[MO_MAX_BINS + 1];
    __shared__ int s_hist[MO_MAX_BINS];
    const MotionRows& g = p.g;
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const long y = blockIdx.y, row = p.r0 + y;
    MotionSel* sel = p.sel + y;
    const int G = pass == 0 ? 1 : sel->G;
    if (pass > 1 && G == 0) return;
    const long q0 = (long)blockIdx.x * p.chunk;
    const int m = (int)min((long)p.chunk, g.W - q0), nblk = (m + MO_BLOCK - 1) / MO_BLOCK;
    const double* src = mo_row(g, row) + q0;
    const double mean = pass == 1 ? sel->mean : 0.0;
    const int shift = 56 - 8 * pass;
    for (int i = tid; i < G * 256; i += MO_THREADS) s_rh[i] = 0u;
    if (tid < MO_TARGETS) s_gp[tid] = pass == 0 ? 0ull : sel->gprefix[tid];
    if (pass == 0) {
        for (int i = tid; i <= g.B; i += MO_THREADS) s_edges[i] = g.edges[i];
        if (tid < MO_MAX_BINS) s_hist[tid] = 0;
    }
    __syncthreads();
    int n = 0, st = 0;
    unsigned long long mx = 0ull;
    for (int b = 0; b < nblk; ++b) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = b * MO_BLOCK + k * MO_THREADS + tid;
            int key = -1;
            if (q < m) {
                const double a = src[q];
                if (a == a) {
                    const unsigned long long bits = (unsigned long long)__double_as_longlong(a);
                    if (pass == 0) {
                        t += a; ++n; st += a == 0.0 ? 1 : 0; mx = max(mx, bits);
                        const int bin = mo_bin(s_edges, g.hist ? g.B : 0, a);
                        if (bin >= 0) atomicAdd(&s_hist[bin], 1);
                        key = (int)(bits >> 56);
                    } else {
                        if (pass == 1) { const double d = a - mean; t = fma(d, d, t); }
                        const unsigned long long pre = bits >> (shift + 8);
                        for (int gi = 0; gi < G; ++gi)
                            if (s_gp[gi] == pre) { key = gi * 256 + (int)((bits >> shift) & 255u); break; }
                    }
                }
            }
            const unsigned long long act = __ballot(key >= 0);
            if (act) {
                const int lead = __ffsll((long long)act) - 1;
                const int k0 = __shfl(key, lead, WAVE);
                if (__ballot(key == k0) == act) {
                    if (lane == lead) atomicAdd(&s_rh[k0], (unsigned)__popcll(act));
                } else if (key >= 0) {
                    atomicAdd(&s_rh[key], 1u);
                }
            }
        }
        if (pass <= 1) {
            t = wave_sum(t);
            if (lane == 0) s_w[b][wv] = t;
        }
    }
    if (pass == 0) {
        n = wave_sum(n); st = wave_sum(st);
        if (lane == 0 && n) { atomicAdd(&sel->N, n); atomicAdd(&sel->still, st); }
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned long long)__shfl_xor((long long)mx, o, WAVE));
        if (lane == 0 && mx) atomicMax(&sel->maxbits, mx);
    }
    __syncthreads();
    if (pass <= 1 && tid < nblk) {
        double* out = (pass == 0 ? p.psum : p.pss) + y * (long)p.nblk_row + blockIdx.x * (long)(p.chunk / MO_BLOCK);
        out[tid] = mo_block_total(s_w[tid]);
    }
    if (pass == 0 && g.hist && tid < g.B && s_hist[tid]) atomicAdd(&g.hist[row * g.B + tid], s_hist[tid]);
    unsigned* rh = p.rhist + y * (long)(MO_TARGETS * 256);
    for (int i = tid; i < G * 256; i += MO_THREADS) {
        const unsigned v = s_rh[i];
        if (v) atomicAdd(&rh[i], v);
    }
}

struct MotionSelectParams {
    MotionRows g;
    long r0;
    int nblk_row;
    const double* psum;
    const double* pss;
    unsigned* rhist;
    MotionSel* sel;
};

__global__ __launch_bounds__(WAVE) void k_motion_select(const MotionSelectParams p, const int pass) {
    const MotionRows& g = p.g;
    const int tid = threadIdx.x;
    const long y = blockIdx.x, row = p.r0 + y;
    MotionSel* sel = p.sel + y;
    unsigned* rh = p.rhist + y * (long)(MO_TARGETS * 256);
    const int N = sel->N, nt = g.quant ? 2 * g.Q : 0;
    if (pass == 0 && tid == 0) {
        if (N == 0) {
            mo_write_empty(g, row);
        } else {
            const double* ps = p.psum + y * (long)p.nblk_row;
            double total = 0.0;
            for (int b = 0; b < p.nblk_row; ++b) total += ps[b];
            sel->mean = total / (double)N;
            mo_write_head(g, row, total, N, sel->still, __longlong_as_double((long long)sel->maxbits));
        }
    }
    if (pass == 1 && tid == 0 && N > 0) {
        const double* ps = p.pss + y * (long)p.nblk_row;
        double ss = 0.0;
        for (int b = 0; b < p.nblk_row; ++b) ss += ps[b];
        g.stats[g.rows + row] = mo_sd(ss, N);
    }
    const int G = pass == 0 ? (N > 0 && nt ? 1 : 0) : sel->G;
    if (G == 0) {                                                // uniform: no rank is wanted of this row
        if (pass == 0) {
            for (int i = tid; i < 256; i += WAVE) rh[i] = 0u;
            if (tid == 0) sel->G = 0;
        }
        return;
    }
    if (tid < nt) {
        unsigned long long prefix = 0ull;
        unsigned rank;
        int grp = 0;
        if (pass == 0) {
            double pos; int i;
            mo_rank_of(g.q[tid >> 1], N, pos, i);
            rank = (unsigned)((tid & 1) ? min(i + 1, N - 1) : i);
        } else {
            prefix = sel->prefix[tid]; rank = sel->rank[tid]; grp = sel->group[tid];
        }
        const unsigned* h = rh + grp * 256;
        unsigned cum = 0u;
        int d = 0;
        for (; d < 255; ++d) {
            const unsigned c = h[d];
            if (rank < cum + c) break;
            cum += c;
        }
        sel->prefix[tid] = (prefix << 8) | (unsigned long long)d;
        sel->rank[tid] = rank - cum;
    }
    __syncthreads();
    for (int i = tid; i < G * 256; i += WAVE) rh[i] = 0u;
    if (tid == 0) {
        int G2 = 0;
        for (int j = 0; j < nt; ++j) {
            const unsigned long long pre = sel->prefix[j];
            int gi = 0;
            while (gi < G2 && sel->gprefix[gi] != pre) ++gi;
            if (gi == G2) sel->gprefix[G2++] = pre;
            sel->group[j] = gi;
        }
        sel->G = G2;
    }
    if (pass == MO_PASSES - 1 && tid < g.Q) {
        double pos; int i;
        mo_rank_of(g.q[tid], N, pos, i);
        const double xi = __longlong_as_double((long long)sel->prefix[2 * tid]);
        const double xj = __longlong_as_double((long long)sel->prefix[2 * tid + 1]);
        g.quant[row * g.Q + tid] = i >= N - 1 ? xi : mo_lerp(xi, xj, pos, i);
    }
}

}  // namespace vet

namespace vh {

// What vet_head_motion* refuse about their arguments, before anything is staged, allocated or launched.
int check_motion_args(const vet_plan* pl, int U, int T, int window, int stride, int lag, int per_user, const double* fractions, int Q,
                      const double* edges, int B, const void* stats) {
    int rc = check_run_args(pl, U, T, stats);
    if (rc) return rc;
    if (lag < 1) return fail(VET_ERR_INVALID, "lag must be at least 1 frame (got %d)", lag);
    if (lag > T - 1) return fail(VET_ERR_INVALID, "lag of %d frames leaves no pair in a video of %d frames", lag, T);
    if (window < 1) return fail(VET_ERR_INVALID, "window must be at least 1 frame pair (got %d)", window);
    if (stride < 1) return fail(VET_ERR_INVALID, "stride must be at least 1 frame pair (got %d)", stride);
    if (window > T - lag)
        return fail(VET_ERR_INVALID, "window of %d frame pairs is longer than the video's %d frame pairs at lag %d", window, T - lag, lag);
    if (Q < 0 || Q > vet::MO_MAX_Q) return fail(VET_ERR_INVALID, "need 0 to %d quantile fractions (got %d)", vet::MO_MAX_Q, Q);
    if (Q && !fractions) return fail(VET_ERR_INVALID, "fractions is NULL");
    for (int i = 0; i < Q; ++i)
        if (!(fractions[i] >= 0.0 && fractions[i] <= 1.0) || (i && !(fractions[i] > fractions[i - 1])))
            return fail(VET_ERR_INVALID, "quantile fractions must lie in [0, 1] and be strictly increasing (fraction %d is %g)", i,
                        fractions[i]);
    if (B < 0 || B > vet::MO_MAX_BINS) return fail(VET_ERR_INVALID, "need 0 to %d histogram bins (got %d)", vet::MO_MAX_BINS, B);
    if (B && !edges) return fail(VET_ERR_INVALID, "edges is NULL");
    for (int i = 0; i <= B && B; ++i)
        if (!std::isfinite(edges[i]) || (i && !(edges[i] > edges[i - 1])))
            return fail(VET_ERR_INVALID, "histogram edges must be finite and strictly ascending (edge %d is %g)", i, edges[i]);
    if ((int64_t)window * U > (int64_t)0x7FFFFFFF)
        return fail(VET_ERR_UNSUPPORTED, "head motion: window * n_users = %lld values per row (at most 2^31 - 1)", (long long)window * U);
    if (per_user) return check_user_dirs_frames(T, "head motion");
    return VET_OK;
}

namespace {

constexpr size_t kMotionPassBudget = (size_t)256 << 20;   // bytes of per-row workspace a pass of the chunked shape may take

int launch_motion(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window, int stride,
                  int lag, int per_user, const double* fractions, int Q, const double* edges, int B, double* d_stats,
                  double* d_quant, int32_t* d_hist, int32_t* d_still, int32_t* d_samples, int32_t* d_status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const long P = T - lag, R = (long)vet_window_rows((int)P, window, stride);
    const long rows = per_user ? R * U : R, W = per_user ? window : (long)window * U;
    if (!d_quant) Q = 0;
    if (!Q) d_quant = nullptr;
    if (!d_hist) B = 0;
    if (!B) d_hist = nullptr;
    int bound = vet::MO_LDS_VALUES;
    if (c->tune.motion_lds_values > 0)
        bound = std::min(bound, std::max(vet::MO_BLOCK, c->tune.motion_lds_values / vet::MO_BLOCK * vet::MO_BLOCK));
    const bool one_wg = W <= bound;
    const long nblk_row = (W + vet::MO_BLOCK - 1) / vet::MO_BLOCK, chunks = (W + bound - 1) / bound;
    const size_t per_row = (size_t)nblk_row * 16 + (size_t)vet::MO_TARGETS * 256 * 4 + sizeof(vet::MotionSel);
    long CR = std::max(1L, std::min({(long)(kMotionPassBudget / per_row), rows, 65535L}));
    // workspace: the angles | the transposed ids of the per-viewer layout | the chunked shape's per-row arrays of a pass
    WsLayout lay;
    const size_t ang_o = lay.take<double>((size_t)P * U), dirs_o = lay.take<int32_t>(per_user ? (size_t)U * T : 0),
                 psum_o = lay.take<double>(one_wg ? 0 : (size_t)CR * nblk_row), pss_o = lay.take<double>(one_wg ? 0 : (size_t)CR * nblk_row),
                 rh_o = lay.take<uint32_t>(one_wg ? 0 : (size_t)CR * vet::MO_TARGETS * 256),
                 sel_o = lay.take<vet::MotionSel>(one_wg ? 0 : (size_t)CR);
    int rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    double* angles = (double*)(ws + ang_o);
    {   // stage 1
        vet::MotionAnglesParams q{};
        q.src = vet::SampleSrc{d_mu, d_mv, d_ids, pl->W, pl->H, (long)pl->n_dirs};
        q.unit = pl->d_dir_unit; q.raw = pl->d_dir_raw;
        q.U = U; q.T = T; q.lag = lag; q.P = P; q.angles = angles; q.status = d_status;
        const dim3 grid((unsigned)grid_for(P * U, vet::MO_THREADS, c->n_cu));
        if (per_user) {
            int32_t* dirs = (int32_t*)(ws + dirs_o);
            rc = user_dirs_run(pl, d_mu, d_mv, d_ids, U, T, dirs, d_status, "head motion", s);
            if (rc) return rc;
            q.dirs = dirs;
            ProfScope ps(c, s, KID_SPATIAL);
            hipLaunchKernelGGL(vet::k_motion_angles<2>, grid, dim3(vet::MO_THREADS), 0, s, q);
        } else {
            ProfScope ps(c, s, KID_SPATIAL);
            if (d_ids) hipLaunchKernelGGL(vet::k_motion_angles<1>, grid, dim3(vet::MO_THREADS), 0, s, q);
            else hipLaunchKernelGGL(vet::k_motion_angles<0>, grid, dim3(vet::MO_THREADS), 0, s, q);
        }
        HIP_TRY(hipGetLastError());
    }
    vet::MotionRows g{};
    g.angles = angles; g.R = R; g.P = P; g.W = W; g.U = U; g.stride = stride; g.per_user = per_user ? 1 : 0; g.rows = rows;
    g.Q = Q; g.B = B;
    for (int i = 0; i < Q; ++i) g.q[i] = fractions[i];
    for (int i = 0; i <= B && B; ++i) g.edges[i] = edges[i];
    g.stats = d_stats; g.quant = d_quant; g.hist = d_hist; g.still = d_still; g.samples = d_samples; g.status = d_status;
    if (W <= vet::WAVE) {
        const int grid = grid_for(rows * vet::WAVE, vet::MO_THREADS, c->n_cu);
        ProfScope ps(c, s, KID_TRANSITION);
        hipLaunchKernelGGL(vet::k_motion_wave, dim3((unsigned)grid), dim3(vet::MO_THREADS), 0, s, g);
        HIP_TRY(hipGetLastError());
        return VET_OK;
    }
    if (one_wg) {
        int Psort = 256;
        while (Psort < W) Psort <<= 1;
        const size_t lds = d_quant ? (size_t)Psort * 8 : 0;
        const long per_cu = std::min<long>((long)(kWholeLds / (lds + 2048)), 32 / (vet::MO_THREADS / vet::WAVE));
        const long grid = std::max<long>(1, std::min<long>(rows, (long)c->n_cu * std::max(1L, per_cu)));
        ProfScope ps(c, s, KID_TRANSITION);
        hipLaunchKernelGGL(vet::k_motion_rows, dim3((unsigned)grid), dim3(vet::MO_THREADS), lds, s, g, Psort);
        HIP_TRY(hipGetLastError());
        return VET_OK;
    }
    ProfScope ps(c, s, KID_TRANSITION);
    for (long r0 = 0; r0 < rows; r0 += CR) {
        const long cr = std::min(CR, rows - r0);
        vet::MotionChunkParams q{};
        q.g = g; q.r0 = r0; q.chunk = bound; q.nblk_row = (int)nblk_row;
        q.psum = (double*)(ws + psum_o); q.pss = (double*)(ws + pss_o); q.rhist = (uint32_t*)(ws + rh_o);
        q.sel = (vet::MotionSel*)(ws + sel_o);
        vet::MotionSelectParams t{};
        t.g = g; t.r0 = r0; t.nblk_row = (int)nblk_row; t.psum = q.psum; t.pss = q.pss; t.rhist = q.rhist; t.sel = q.sel;
        HIP_TRY(hipMemsetAsync(q.rhist, 0, (size_t)cr * vet::MO_TARGETS * 256 * 4, s));
        HIP_TRY(hipMemsetAsync(q.sel, 0, (size_t)cr * sizeof(vet::MotionSel), s));
        if (d_hist) HIP_TRY(hipMemsetAsync(d_hist + r0 * B, 0, (size_t)cr * B * 4, s));
        const int passes = d_quant ? vet::MO_PASSES : 2;
        for (int pass = 0; pass < passes; ++pass) {
            hipLaunchKernelGGL(vet::k_motion_chunk, dim3((unsigned)chunks, (unsigned)cr), dim3(vet::MO_THREADS), 0, s, q, pass);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(vet::k_motion_select, dim3((unsigned)cr), dim3(vet::WAVE), 0, s, t, pass);
            HIP_TRY(hipGetLastError());
        }
    }
    return VET_OK;
}

}  // namespace

int motion_set_attrs(vet_ctx*) {
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_motion_rows, hipFuncAttributeMaxDynamicSharedMemorySize,
                                vet::MO_LDS_VALUES * 8));
    return VET_OK;
}

}  // namespace vh

using namespace vh;

extern "C" {

int vet_head_motion(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, int lag, int per_user,
                    const double* h_fractions, int Q, const double* h_edges, int B, double* d_stats, double* d_quantiles,
                    int32_t* d_hist, int32_t* d_still, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_motion_args(pl, U, T, window, stride, lag, per_user, h_fractions, Q, h_edges, B, d_stats);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_head_motion_ids", stream, &s);
    return rc ? rc : launch_motion(pl, d_mu, d_mv, nullptr, U, T, window, stride, lag, per_user, h_fractions, Q, h_edges, B, d_stats,
                                   d_quantiles, d_hist, d_still, d_samples, d_status, s);
}

int vet_head_motion_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, int lag, int per_user,
                        const double* h_fractions, int Q, const double* h_edges, int B, double* d_stats, double* d_quantiles,
                        int32_t* d_hist, int32_t* d_still, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_motion_args(pl, U, T, window, stride, lag, per_user, h_fractions, Q, h_edges, B, d_stats);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_motion(pl, nullptr, nullptr, d_ids, U, T, window, stride, lag, per_user, h_fractions, Q, h_edges, B, d_stats,
                                   d_quantiles, d_hist, d_still, d_samples, d_status, s);
}

}  // extern "C"
