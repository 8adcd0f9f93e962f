// vet_group.hip — the two-audience permutation test behind vet_group_divergence* (include/vet.h): the kernels and their launch
// logic.  Two sets of viewers, A and B, are compared row by row with the mass-weighted Jensen-Shannon divergence of the divergence
// calls, D_k = S(A + B) - (W_A S(A) + W_B S(B)) / (W_A + W_B) per lattice, and the observed value is placed in the distribution of
// the same statistic under P relabellings of the included viewers that keep the two group sizes.  A labelling's group histogram is
//     A = sum_{u in A} h_u,   h_u = viewer u's own row histogram (vet_user_entropy's d_weights),
// the bootstrap's [B x U] . [U x n] FP64 contraction with 0/1 masks in place of resample counts: both groups of a labelling read the
// same histogram operand, so one 16 x 16 x 4 MFMA tile carries the A sums of eight labellings in rows 0-7 and their B sums in rows
// 8-15.  B is never taken as pooled - A: the subtraction would leave rounding residue on tiles that must be exactly 0.
// Stages, rows in chunks so that the workspace stays bounded whatever R is:
//   1  k_user_dirs (vet_user_dirs.hpp, unchanged): direction ids transposed once, dirs[U][T];
//   2  k_group_labels: labels[P + 1][U] u8 (0 = A, 1 = B, 255 = excluded); row 0 is the observed grouping, row b + 1 permutation b:
//      its keys ranked by a bitonic sort in LDS, no atomics;
//   3  per lattice and chunk of rows, k_user_hist_w/_c (user_hist_run, unchanged) and on weighted lattices k_bootstrap_zero_keys
//      (zero_keys_run, unchanged);
//   4  k_group_gemm: one workgroup per (row, block of 8 labellings): the product into LDS, then per labelling W and S of A, of B and
//      of a_t + b_t (row_total / row_entropy, vet_row_hist.hpp) and D_k; lattice 0 stores D_0 / K, later lattices add;
//   5  k_group_samples (the observed groups' present samples per row), k_group_maxnull (per permutation the largest finite null
//      value over the rows), k_group_summary (one workgroup per row: counts, mean and the sorted quantile).
// A labelling's bits depend on the plan, the window, the row's frames and the labelling's two viewer sets only: labelling 0 goes
// through the same kernel and the same operand order as the permutations, so a permutation that reproduces the observed partition
// reproduces its bits, and ties in the p-value are exact.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_user_dirs.hpp"
#include "vet_row_hist.hpp"
#include "vet_rank.hpp"

#include <algorithm>

namespace vet {

constexpr int GROUP_LB = 8;            // labellings per workgroup of k_group_gemm: rows i and i + 8 of the 16x16x4 MFMA's M
constexpr int GROUP_NT = 4;            // column blocks a wave of k_group_gemm holds accumulators for at a time
constexpr int GROUP_MAX_P = 4096;      // permutations of a call: k_group_summary sorts them in LDS
constexpr int GROUP_MAX_N = 16384;     // included viewers: k_group_labels ranks one permutation's keys in LDS
constexpr unsigned char GROUP_OUT = 255;   // the label of an excluded viewer (-1 as a byte)

// ------------------------------------------------------------------------------------------
// k_group_labels — stage 2.  Workgroup 0 copies the observed groups; workgroup b + 1 makes permutation b: for the included index
// i = 0 .. N-1 (viewer inc[i], ascending) the SplitMix64 finaliser z of seed + (b N + i + 1) * golden ratio and the key
// (z >> 16 << 16) | i — distinct keys, N <= 2^14 —, a bitonic sort of the keys, and the U_A smallest are audience A.
// LDS: u64 [next power of two >= N] dynamic.
// ------------------------------------------------------------------------------------------
struct GroupLabelsParams {
    const unsigned char* groups; // [U] 0, 1, 255
    const int32_t* inc;          // [N] the included viewers, ascending
    int U, N, UA;
    unsigned long long seed;
    unsigned char* labels;       // [P + 1][U]
};

__global__ __launch_bounds__(256) void k_group_labels(const GroupLabelsParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* key = (unsigned long long*)smem;
    const int tid = threadIdx.x;
    const long row = blockIdx.x;
    unsigned char* out = p.labels + row * (long)p.U;
    for (int u = tid; u < p.U; u += 256) {
        const unsigned char g = p.groups[u];
        if (row == 0 || g == GROUP_OUT) out[u] = g;
    }
    if (row == 0) return;
    int Np = 1;
    while (Np < p.N) Np <<= 1;
    const unsigned long long base = (unsigned long long)(row - 1) * (unsigned long long)p.N;
    for (int i = tid; i < Np; i += 256) {
        unsigned long long k = ~0ull;
        if (i < p.N) {
            unsigned long long z = p.seed + (base + (unsigned long long)i + 1ull) * 0x9E3779B97F4A7C15ull;
            z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
            z ^= z >> 27; z *= 0x94D049BB133111EBull;
            z ^= z >> 31;
            k = (z >> 16 << 16) | (unsigned long long)i;
        }
        key[i] = k;
    }
    lds_bitonic_sort(key, Np);
    for (int j = tid; j < p.N; j += 256) out[p.inc[(int)(key[j] & 0xFFFFull)]] = j < p.UA ? 0 : 1;
}

// ------------------------------------------------------------------------------------------
// k_group_gemm — stage 4.  One workgroup: one row of the chunk, labellings [8 x, 8 x + 8); 256 threads = 4 waves.  The launch is
// one-dimensional and the workgroup id is remapped (bijectively) so that the blocks that share an XCD — ids equal mod 8 — take
// consecutive (row, x): the workgroups of one row then read its U x n histograms through one L2 instead of through eight.  A pure
// speed choice: every workgroup computes the same values wherever it runs.
// Product, as k_bootstrap_gemm runs it: wave w takes the 16-tile column blocks w, w + 4, ... (four of them at a time); for each it
// runs the whole K loop over the viewers in ascending blocks of four into ONE accumulator with v_mfma_f64_16x16x4_f64 (no split-K,
// no atomics):
//     A[i = lane & 15][k = lane >> 4] = labels[l0 + (i & 7)][u0 + k] == (i >> 3) ? 1.0 : 0.0
//     B[k = lane >> 4][j = lane & 15] = hist[u0 + k][t0 + j]            (loaded once, serves both groups)
//     D: col = lane & 15, row = (lane >> 4) + 4 * reg   (the f64 form's own map, not the f32 one)
// with the edges predicated to 0.0, and leaves the 16 x n block in LDS: rows 0-7 the A sums of the eight labellings, rows 8-15
// their B sums.  A viewer outside a group adds 1.0 * 0.0 or 0.0 * h = +0.0: a group's sum is the sum over its members in ascending
// order, whatever the other rows of the tile hold.
// Epilogue: wave w takes labellings 2 w and 2 w + 1: a tile is a key of A iff a_t > 0.0, of B iff b_t > 0.0, of the pooled dict iff
// a_t + b_t > 0.0; W = row_total and S = row_entropy of each (q = 0 by underflow gives the reference's NaN by itself);
// D_k = S(A + B) - (W_A S(A) + W_B S(B)) / (W_A + W_B), NaN where W_A or W_B is not > 0 (a group without a sample in the row, or
// all of whose keys are 0.0).  Zero-key rule: only where the row has a slot with zflag set, NaN iff a marked tile of a member of A
// sums to 0.0 in A, of a member of B in B, or of any included viewer in a_t + b_t.  Output: labelling 0 to obs[row], labelling
// b + 1 to null[row][b]; `first` stores D_k / K, later lattices add; lattice 0 may also leave labelling 0's two histograms as
// weights[row][2][n] (plain values, +0.0 = no weight).
// LDS: f64 [16][n] dynamic.
// ------------------------------------------------------------------------------------------
typedef double group_v4d __attribute__((ext_vector_type(4)));

struct GroupGemmParams {
    const double* hist;          // [CR][U][n]
    const int32_t* zflag;        // [CR][U], null for counting lattices
    const uint32_t* zmask;       // [CR][U][zw]
    const unsigned char* labels; // [L][U]
    int U, n, L, zw;             // L = P + 1 labellings
    int lblocks;                 // ceil(L / 8): workgroups per row
    int first;                   // lattice 0: store; later lattices: add
    double K;                    // lattices of the plan
    double* obs;                 // [CR], the chunk's first row
    double* null;                // [CR][L - 1], the chunk's first row
    double* weights;             // [CR][2][n], the chunk's first row, or null
};

// Two waves per SIMD as the register budget (what 64 KB of LDS per workgroup gives at 501 tiles): at most 256 registers, so the
// MFMAs take their accumulators in VGPRs and the K loop carries them without copies to and from the accumulation registers.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_group_gemm(const GroupGemmParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* S = (double*)smem;                                     // [16][n]
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int n = p.n, U = p.U;
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7u, q8 = nwg >> 3, r8 = nwg & 7u;
    const unsigned wg = (xcd < r8 ? xcd * (q8 + 1u) : r8 * (q8 + 1u) + (xcd - r8) * q8) + (blockIdx.x >> 3);
    const long rc = wg / (unsigned)p.lblocks;
    const int l0 = (int)(wg % (unsigned)p.lblocks) * GROUP_LB;
    const double* H = p.hist + rc * (long)U * n;
    {
        const int i = lane & 15, kk = lane >> 4;
        const bool row_ok = l0 + (i & 7) < p.L;
        const unsigned char want = (unsigned char)(i >> 3);
        const unsigned char* lrow = p.labels + (long)(row_ok ? l0 + (i & 7) : 0) * U;
        const int ntb = (n + 15) >> 4;
        for (int tb0 = wv; tb0 < ntb; tb0 += 4 * GROUP_NT) {
            int t[GROUP_NT];
            bool col_ok[GROUP_NT];
            group_v4d acc[GROUP_NT];
#pragma unroll
            for (int j = 0; j < GROUP_NT; ++j) {
                t[j] = (tb0 + 4 * j) * 16 + i;
                col_ok[j] = t[j] < n;
                acc[j] = group_v4d{0.0, 0.0, 0.0, 0.0};
            }
            // Two K blocks per trip; a K block beyond U adds 0.0 * 0.0.  The ten loads of the NEXT trip are issued before the eight
            // MFMAs of this one, so that their latency runs under the matrix unit's 8 x 64 cycles (two waves per SIMD do not hide
            // it by themselves).  Every accumulator still sees its K blocks in ascending order.
            // The loads carry no branch: an index beyond an edge is clamped into the array (viewer U - 1, tile n - 1), so that the
            // ten loads leave back to back and the wait sits behind the MFMAs.  The edges are predicated through the A operand
            // alone: a viewer beyond U or a labelling beyond L has the mask 0.0, and 0.0 * h = +0.0 for the finite h >= 0 that was
            // loaded in its place; a column beyond n holds sums that are never stored.
            int tc[GROUP_NT];
#pragma unroll
            for (int j = 0; j < GROUP_NT; ++j) tc[j] = min(t[j], n - 1);
            const auto fetch = [&](int u0, unsigned char (&ra)[2], double (&b)[2][GROUP_NT]) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const int u = min(u0 + 4 * s2 + kk, U - 1);
                    ra[s2] = lrow[u];
#pragma unroll
                    for (int j = 0; j < GROUP_NT; ++j) b[s2][j] = H[(long)u * n + tc[j]];
                }
            };
            const auto mask = [&](int u0, const unsigned char (&ra)[2], double (&a)[2]) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) a[s2] = (u0 + 4 * s2 + kk < U && row_ok && ra[s2] == want) ? 1.0 : 0.0;
            };
            unsigned char ra[2];
            double a[2], b[2][GROUP_NT], b_next[2][GROUP_NT];
            fetch(0, ra, b);
            mask(0, ra, a);
            for (int u0 = 0; u0 < U; u0 += 8) {
                fetch(u0 + 8, ra, b_next);                         // beyond U: viewer U - 1 again, under the mask 0.0
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                    for (int j = 0; j < GROUP_NT; ++j)
                        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s2], b[s2][j], acc[j], 0, 0, 0);
                mask(u0 + 8, ra, a);
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                    for (int j = 0; j < GROUP_NT; ++j) b[s2][j] = b_next[s2][j];
            }
#pragma unroll
            for (int j = 0; j < GROUP_NT; ++j)
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
    if (p.weights && l0 == 0) {
        double* out = p.weights + rc * 2L * n;
        for (int i = tid; i < 2 * n; i += 256)
            __builtin_nontemporal_store(S[(i < n ? 0L : (long)GROUP_LB * n) + (i < n ? i : i - n)], out + i);
    }
    for (int q = 0; q < 2; ++q) {
        const int ii = wv * 2 + q, l = l0 + ii;
        if (l >= p.L) break;
        const double* Sa = S + (long)ii * n;
        const double* Sb = S + (long)(ii + GROUP_LB) * n;
        const auto keys_a = [&](int t, double& v) { v = Sa[t]; return v > 0.0; };
        const auto keys_b = [&](int t, double& v) { v = Sb[t]; return v > 0.0; };
        const auto keys_p = [&](int t, double& v) { v = Sa[t] + Sb[t]; return v > 0.0; };
        const double wa = row_total(n, keys_a), sa = row_entropy(n, wa, keys_a);
        const double wb = row_total(n, keys_b), sb = row_entropy(n, wb, keys_b);
        const double wp = row_total(n, keys_p), sp = row_entropy(n, wp, keys_p);
        bool bad = false;
        if (any_z) {
            const unsigned char* lrow = p.labels + (long)l * U;
            for (int u0 = 0; u0 < U; u0 += WAVE) {
                const int u = u0 + lane;
                const int lab = u < U ? (int)lrow[u] : (int)GROUP_OUT;
                const bool f = u < U && lab != (int)GROUP_OUT && p.zflag[rc * (long)U + u] != 0;
                unsigned long long who = __ballot(f);
                while (who) {
                    const int j = __ffsll((long long)who) - 1;
                    who &= who - 1ull;
                    const int labj = __shfl(lab, j);
                    const double* own = labj == 0 ? Sa : Sb;
                    const uint32_t* zm = p.zmask + (rc * (long)U + u0 + j) * (long)p.zw;
                    for (int w = lane; w < p.zw; w += WAVE) {
                        unsigned bits = zm[w];
                        while (bits) {
                            const int t = w * 32 + __ffs((int)bits) - 1;
                            bits &= bits - 1u;
                            bad |= own[t] == 0.0 || Sa[t] + Sb[t] == 0.0;
                        }
                    }
                }
            }
            bad = __ballot(bad) != 0ull;
        }
        if (lane == 0) {
            double d = sp - (wa * sa + wb * sb) / (wa + wb);
            if (!(wa > 0.0) || !(wb > 0.0) || bad) d = __builtin_nan("");
            double* dst = l == 0 ? p.obs + rc : p.null + rc * (long)(p.L - 1) + (l - 1);
            *dst = p.first ? d / p.K : *dst + d / p.K;
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_group_samples — one thread per row: the present samples of the observed A and B, from user_hist_run's per-(viewer, row)
// samples su[U][R] (the threads of a wave read neighbouring rows of one viewer).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_group_samples(const int32_t* su, const unsigned char* groups, int U, long R, int32_t* samples) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    int sa = 0, sb = 0;
    for (int u = 0; u < U; ++u) {
        const unsigned char g = groups[u];
        if (g == GROUP_OUT) continue;
        const int v = su[u * R + r];
        if (g == 0) sa += v; else sb += v;
    }
    samples[r] = sa;
    samples[R + r] = sb;
}

// ------------------------------------------------------------------------------------------
// k_group_maxnull — one thread per permutation b walks the rows of null[R][P] (coalesced across the threads): the largest finite
// value, NaN where the permutation has none.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_group_maxnull(const double* null, int P, long R, double* maxnull) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P) return;
    double best = __builtin_nan("");
    for (long r = 0; r < R; ++r) {
        const double v = null[r * P + b];
        if (isfinite(v) && !(best >= v)) best = v;
    }
    maxnull[b] = best;
}

// ------------------------------------------------------------------------------------------
// k_group_summary — one workgroup per row: null[r][0 .. P) to LDS, everything that is not finite replaced by +inf (so are the
// slots up to the next power of two), the counts (integers: exact in any order), a bitonic sort (vet_rank.hpp), then wave 0 over
// the m finite values in ascending order: the mean in lane order + wave_sum and the quantile `confidence` (lerp_quantile).
// summary [5][R]: observed (already there: k_group_gemm wrote it), p_value = (1 + #{finite null >= observed}) / (1 + m),
// p_adjusted = (1 + #{b: maxnull[b] >= observed}) / (1 + M), M the permutations that have a maxnull; null_mean, null_crit.
// observed NaN: both p NaN; m = 0: null_mean and null_crit NaN.
// LDS: f64 [4096] static.
// ------------------------------------------------------------------------------------------
struct GroupSummaryParams {
    const double* null;          // [R][P]
    const double* maxnull;       // [P]
    int P;
    long R;
    double confidence;
    double* summary;             // [5][R]
    int32_t* valid;              // [R] or null
};

__global__ __launch_bounds__(256) void k_group_summary(const GroupSummaryParams p) {
    __shared__ double x[GROUP_MAX_P];
    __shared__ int cnt[4];                                         // m, #{null >= observed}, M, #{maxnull >= observed}
    const int tid = threadIdx.x, lane = lane_id();
    const long r = blockIdx.x;
    const double o = p.summary[r];
    int Pp = 1;
    while (Pp < p.P) Pp <<= 1;
    if (tid < 4) cnt[tid] = 0;
    __syncthreads();
    int m_ = 0, ge = 0, M_ = 0, adj = 0;
    for (int i = tid; i < Pp; i += 256) {
        double v = __builtin_inf();
        if (i < p.P) {
            const double w = p.null[r * p.P + i];
            if (isfinite(w)) { v = w; ++m_; ge += w >= o; }
            const double mx = p.maxnull[i];
            if (isfinite(mx)) { ++M_; adj += mx >= o; }
        }
        x[i] = v;
    }
    if (m_) atomicAdd(&cnt[0], m_);
    if (ge) atomicAdd(&cnt[1], ge);
    if (M_) atomicAdd(&cnt[2], M_);
    if (adj) atomicAdd(&cnt[3], adj);
    lds_bitonic_sort(x, Pp);
    if (wave_id() != 0) return;
    const int m = cnt[0];
    double s = 0.0;
    for (int i = lane; i < m; i += WAVE) s += x[i];
    s = wave_sum(s);
    if (lane == 0) {
        const double nan = __builtin_nan("");
        const bool has = o == o;
        p.summary[1 * p.R + r] = has ? (double)(1 + cnt[1]) / (double)(1 + m) : nan;
        p.summary[2 * p.R + r] = has ? (double)(1 + cnt[3]) / (double)(1 + cnt[2]) : nan;
        p.summary[3 * p.R + r] = m ? s / (double)m : nan;
        p.summary[4 * p.R + r] = m ? lerp_quantile(x, m, p.confidence) : nan;
        if (p.valid) p.valid[r] = m;
    }
}

}  // namespace vet

namespace vh {

namespace {

constexpr size_t kGroupHistBudget = (size_t)256 << 20;    // bytes of histograms a chunk of rows may take in the workspace

size_t group_lds_bytes(int n) { return (size_t)2 * vet::GROUP_LB * n * sizeof(double); }

// the groups as the kernels read them: N included viewers, UA of them in A
struct GroupSizes { int N = 0, UA = 0; };

int scan_groups(int U, const int8_t* groups, GroupSizes* out) {
    if (!groups) return fail(VET_ERR_INVALID, "groups is NULL");
    GroupSizes g;
    for (int u = 0; u < U; ++u) {
        if (groups[u] < -1 || groups[u] > 1)
            return fail(VET_ERR_INVALID, "groups[%d] = %d (0 = audience A, 1 = audience B, -1 = excluded)", u, (int)groups[u]);
        g.N += groups[u] >= 0;
        g.UA += groups[u] == 0;
    }
    if (g.UA < 1 || g.N - g.UA < 1)
        return fail(VET_ERR_INVALID, "both audiences need a viewer (got %d in A, %d in B)", g.UA, g.N - g.UA);
    *out = g;
    return VET_OK;
}

int check_permutations(int permutations) {
    if (permutations < 1 || permutations > vet::GROUP_MAX_P)
        return fail(VET_ERR_INVALID, "permutations must be between 1 and %d (got %d)", vet::GROUP_MAX_P, permutations);
    return VET_OK;
}

int check_included(const GroupSizes& g) {
    if (g.N > vet::GROUP_MAX_N)
        return fail(VET_ERR_UNSUPPORTED, "group divergence: %d included viewers (one permutation's keys are ranked in the LDS: at most %d)",
                    g.N, vet::GROUP_MAX_N);
    return VET_OK;
}

// The caller's groups on the device: the blob holds groups [U] as bytes, then inc [N] (the included viewers, ascending).  The host
// array is read here, before the call returns.
struct GroupBlob {
    BatchBlob blob;
    const unsigned char* groups = nullptr;
    const int32_t* inc = nullptr;
    int stage(vet_ctx* c, int U, const int8_t* h_groups, int N, hipStream_t s) {
        const size_t inc_o = pad16((size_t)U);
        int rc = blob.acquire(c, inc_o + (size_t)N * sizeof(int32_t));
        if (rc) return rc;
        unsigned char* g = (unsigned char*)blob.host();
        int32_t* list = (int32_t*)(g + inc_o);
        for (int u = 0, i = 0; u < U; ++u) {
            g[u] = (unsigned char)h_groups[u];
            if (h_groups[u] >= 0) list[i++] = u;
        }
        groups = (const unsigned char*)blob.dev();
        inc = (const int32_t*)((const char*)blob.dev() + inc_o);
        return blob.upload(s);
    }
};

// labels [P + 1][U] at `labels`, on s; charged to k_finalize
int group_labels_run(vet_ctx* c, const GroupBlob& gb, int U, const GroupSizes& g, int P, uint64_t seed, unsigned char* labels,
                     hipStream_t s) {
    vet::GroupLabelsParams q{};
    q.groups = gb.groups; q.inc = gb.inc; q.U = U; q.N = g.N; q.UA = g.UA; q.seed = (unsigned long long)seed; q.labels = labels;
    size_t np = 1;
    while (np < (size_t)g.N) np <<= 1;
    ProfScope ps(c, s, KID_FINALIZE);
    hipLaunchKernelGGL(vet::k_group_labels, dim3((unsigned)(P + 1)), dim3(256), np * sizeof(unsigned long long), s, q);
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

int launch_group(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window, int stride,
                 const int8_t* groups, int P, uint64_t seed, double confidence, double* d_summary, double* d_null, double* d_weights,
                 int32_t* d_samples, int32_t* d_valid, int32_t* d_status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const int K = (int)pl->lat.size();
    const long R = (long)vet_window_rows(T, window, stride);
    // ---- what the call refuses, before anything is launched or allocated
    int rc = check_group_args(pl, U, groups, P, confidence);
    if (rc) return rc;
    GroupSizes g;
    rc = scan_groups(U, groups, &g);
    if (rc) return rc;
    if (R * (long)U >= (1L << 31))
        return fail(VET_ERR_UNSUPPORTED, "group divergence: %ld rows x users in one call (fewer than 2^31)", R * (long)U);
    rc = check_user_dirs_frames(T, "group divergence");
    if (rc) return rc;
    rc = check_user_plan(pl, "group divergence", s);
    if (rc) return rc;
    int n_max = 0;
    for (int k = 0; k < K; ++k) n_max = std::max(n_max, pl->lat[k].n);
    const int zw_max = (n_max + 31) / 32;
    const int L = P + 1;
    // rows per chunk: the histogram budget, the extent of the product's launch (16 bits of rows, at most 513 workgroups each) and the
    // x extent of the histogram launch
    long CR = c->tune.group_chunk_rows > 0 ? c->tune.group_chunk_rows : (long)(kGroupHistBudget / ((size_t)U * n_max * sizeof(double)));
    CR = std::max(1L, std::min({CR, R, 65535L, ((1L << 31) - 1) / U}));
    // workspace: dirs [U][T] | labels [L][U] u8 | hist [CR][U][n_max] | tot [CR][U] | flag [CR][U] | zmask [CR][U][zw] |
    //            zflag [CR][U] | su [U][R] where the samples are wanted | maxnull [P] | null [R][P] where the caller does not take it
    WsLayout lay;
    const size_t dirs_o = lay.take<int32_t>((size_t)U * T), lab_o = lay.take<unsigned char>((size_t)L * U),
                 hist_o = lay.take<double>((size_t)CR * U * n_max), tot_o = lay.take<double>((size_t)CR * U),
                 flag_o = lay.take<int32_t>((size_t)CR * U), zmask_o = lay.take<uint32_t>((size_t)CR * U * zw_max),
                 zflag_o = lay.take<int32_t>((size_t)CR * U), su_o = lay.take<int32_t>(d_samples ? (size_t)U * R : 0),
                 max_o = lay.take<double>((size_t)P), null_o = lay.take<double>(d_null ? 0 : (size_t)R * P);
    rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    int32_t* dirs = (int32_t*)(ws + dirs_o);
    unsigned char* labels = (unsigned char*)(ws + lab_o);
    double *hist = (double*)(ws + hist_o), *tot = (double*)(ws + tot_o), *maxnull = (double*)(ws + max_o);
    int32_t *flag = (int32_t*)(ws + flag_o), *zflag = (int32_t*)(ws + zflag_o), *su = d_samples ? (int32_t*)(ws + su_o) : nullptr;
    uint32_t* zmask = (uint32_t*)(ws + zmask_o);
    double* null = d_null ? d_null : (double*)(ws + null_o);
    GroupBlob gb;
    rc = gb.stage(c, U, groups, g.N, s);
    if (rc) return rc;
    // ---- stage 1 and 2
    rc = user_dirs_run(pl, d_mu, d_mv, d_ids, U, T, dirs, d_status, "group divergence", s);
    if (rc) return rc;
    rc = group_labels_run(c, gb, U, g, P, seed, labels, s);
    if (rc) return rc;
    const unsigned lblocks = (unsigned)((L + vet::GROUP_LB - 1) / vet::GROUP_LB);
    for (long r0 = 0; r0 < R; r0 += CR) {
        const long cr = std::min(CR, R - r0);
        for (int k = 0; k < K; ++k) {
            const Lattice& Lk = pl->lat[k];
            const bool counting = counts_lattice(pl, k);
            // ---- stage 3; status[1] stays as it is: a row without a sample is data
            rc = user_hist_run(pl, k, dirs, U, T, window, stride, R, r0, cr, hist, tot, flag, k == 0 ? su : nullptr, nullptr, s);
            if (rc) return rc;
            if (!counting) {
                rc = zero_keys_run(pl, k, dirs, U, T, window, stride, r0, cr, hist, flag, zmask, zflag, s);
                if (rc) return rc;
            }
            {   // ---- stage 4, charged to k_transition as the bootstrap's product is
                vet::GroupGemmParams q{};
                q.hist = hist; q.zflag = counting ? nullptr : zflag; q.zmask = zmask; q.labels = labels;
                q.U = U; q.n = Lk.n; q.L = L; q.zw = (Lk.n + 31) / 32; q.lblocks = (int)lblocks;
                q.first = k == 0; q.K = (double)K;
                q.obs = d_summary + r0;
                q.null = null + (size_t)r0 * P;
                q.weights = (k == 0 && d_weights) ? d_weights + (size_t)r0 * 2 * Lk.n : nullptr;
                ProfScope ps(c, s, KID_TRANSITION);
                hipLaunchKernelGGL(vet::k_group_gemm, dim3(lblocks * (unsigned)cr), dim3(256), group_lds_bytes(Lk.n), s, q);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    {   // ---- stage 5, charged to k_finalize
        ProfScope ps(c, s, KID_FINALIZE);
        if (d_samples) {
            hipLaunchKernelGGL(vet::k_group_samples, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, su, gb.groups, U, R, d_samples);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(vet::k_group_maxnull, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, null, P, R, maxnull);
        HIP_TRY(hipGetLastError());
        vet::GroupSummaryParams q{};
        q.null = null; q.maxnull = maxnull; q.P = P; q.R = R; q.confidence = confidence; q.summary = d_summary; q.valid = d_valid;
        hipLaunchKernelGGL(vet::k_group_summary, dim3((unsigned)R), dim3(256), 0, s, q);
        HIP_TRY(hipGetLastError());
    }
    return VET_OK;
}

}  // namespace

int check_group_args(const vet_plan* pl, int U, const int8_t* groups, int permutations, double confidence) {
    GroupSizes g;
    int rc = scan_groups(U, groups, &g);
    if (!rc) rc = check_permutations(permutations);
    if (rc) return rc;
    if (!(confidence > 0.0 && confidence < 1.0))
        return fail(VET_ERR_INVALID, "confidence must be inside (0, 1) (got %g)", confidence);
    rc = check_included(g);
    if (rc) return rc;
    for (const Lattice& L : pl->lat)
        if (group_lds_bytes(L.n) > kWholeLds)
            return fail(VET_ERR_UNSUPPORTED, "group divergence: 8 labellings' two histograms of %d tiles do not fit the LDS (at most %zu tiles)",
                        L.n, kWholeLds / group_lds_bytes(1));
    return VET_OK;
}

int group_set_attrs(vet_ctx*) {
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_group_gemm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWholeLds));
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_group_labels, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWholeLds));
    return VET_OK;
}

}  // namespace vh

using namespace vh;

extern "C" {

int vet_group_divergence(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, const int8_t* groups,
                         int permutations, uint64_t seed, double confidence, double* d_summary, double* d_null, double* d_weights,
                         int32_t* d_samples, int32_t* d_valid, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_args(pl, U, T, window, stride, d_summary);
    if (!rc) rc = check_group_args(pl, U, groups, permutations, confidence);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_group_divergence_ids", stream, &s);
    return rc ? rc : launch_group(pl, d_mu, d_mv, nullptr, U, T, window, stride, groups, permutations, seed, confidence, d_summary,
                                  d_null, d_weights, d_samples, d_valid, d_status, s);
}

int vet_group_divergence_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, const int8_t* groups,
                             int permutations, uint64_t seed, double confidence, double* d_summary, double* d_null, double* d_weights,
                             int32_t* d_samples, int32_t* d_valid, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_args(pl, U, T, window, stride, d_summary);
    if (!rc) rc = check_group_args(pl, U, groups, permutations, confidence);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_group(pl, nullptr, nullptr, d_ids, U, T, window, stride, groups, permutations, seed, confidence, d_summary,
                                  d_null, d_weights, d_samples, d_valid, d_status, s);
}

int vet_group_labels_host(vet_plan* pl, int U, const int8_t* groups, int permutations, uint64_t seed, uint8_t* h_labels) {
    if (!pl || !h_labels) return fail(VET_ERR_INVALID, "plan or h_labels is NULL");
    if (U < 1) return fail(VET_ERR_INVALID, "n_users must be at least 1 (got %d)", U);
    GroupSizes g;
    int rc = scan_groups(U, groups, &g);
    if (!rc) rc = check_permutations(permutations);
    if (!rc) rc = check_included(g);
    if (rc) return rc;
    vet_ctx* c = pl->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)(permutations + 1) * U;
    rc = ensure_ws(c, pad16(bytes));
    if (rc) return rc;
    {
        GroupBlob gb;
        rc = gb.stage(c, U, groups, g.N, c->stream);
        if (!rc) rc = group_labels_run(c, gb, U, g, permutations, seed, (unsigned char*)c->ws, c->stream);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(h_labels, c->ws, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VET_OK;
}

}  // extern "C"
