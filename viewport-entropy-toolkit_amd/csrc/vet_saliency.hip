// vet_saliency.hip — saliency maps behind vet_saliency* (include/vet.h): the spherical kernel density of the viewing directions of a
// window of frames on a W x H equirectangular map, pooled or per viewer, and the row statistics taken from it (mass, peak,
// differential entropy against the uniform sphere, effective area).  Lattice-independent: only the plan's direction table is read.
// Stage 0, k_saliency_ids / k_user_dirs: every sample quantised once (sample_dir) into direction ids — frame-major [T][U] for the
// pooled layout, transposed [U][T] for the per-viewer layout, so that a row's positions are a contiguous slice in both.
// Stage 1, the row LISTS: the distinct ids of a row in ascending id with their multiplicities.  Rows of up to 4096 positions:
// k_saliency_sort, one workgroup per row — lds_bitonic_sort of the ids (absent = the largest key), the heads of the runs compacted in
// order, a head's multiplicity its run length.  Longer rows: k_saliency_count adds into a dense u32 [D] row of the workspace by
// integer atomics (direction tables of up to 32768 entries: counted per workgroup in LDS first) and k_saliency_compact, one
// workgroup per row, walks it in ascending id.
// Stage 2, k_saliency_map: workgroup = (row, 256 pixels), thread = pixel with its direction P in registers.  The row's list is
// staged in LDS in tiles of up to 1024 entries (32 B each: the unit vector and the multiplicity as a double); every lane reads the
// same LDS address — a broadcast — and S = fma(m, exp(kappa * (c - 1)), S) stays in a register across the tiles.  P is built from
// the host's per-column / per-row sines and cosines (five small tables in the workspace) by the heatmap's arithmetic.
// Stage 3, k_saliency_rows: one workgroup per row over the written map: vet_head_motion's summation rule on the pixels in row-major
// order (blocks of 1024; thread t adds t, t + 256, t + 512, t + 768; wave_sum; the four waves in order; the blocks ascending) for
// the mass and the entropy, the peak as the largest (value bits, smallest index).  No FP atomics.  Rows run in passes under a 256 MB
// workspace budget; with d_map NULL the maps of a pass live in the workspace only.
// Saliency similarity (vet_saliency_similarity*): stage 0 once, k_saliency_mask writes the ids once more per audience (every other
// viewer's samples -1), stages 1 and 2 run unchanged for audience A and for audience B per pass, k_saliency_points evaluates each
// audience's density at the other's list entries (NSS without a pixel decision) and k_saliency_compare, one workgroup per row, takes
// the two masses, CC, SIM, JSD and both KL from one pass over the two maps and the NSS from the point values, all by the same rule.
// Viewer congruency (vet_congruency*): stage 0 for both layouts, stage 1 pooled and per viewer per pass, k_congruency_points walks the
// pooled list once per entry of every viewer's own list with the viewer's own multiplicities taken off (the leave-one-out density of
// the others at the viewer's directions; no map), k_congruency_users and k_congruency_rows take the sums by the same rule.
// Saliency scoring (vet_saliency_score*): a predicted map from elsewhere against the pooled audience.  k_score_sort sorts every row
// of the predicted map in LDS (once for a static map), k_score_points samples the map at each list entry's direction (bilinear) and
// takes the entry's area-weighted rank in the map by two binary searches per sorted map row (AUC), k_score_rows takes mass_pred,
// var_pred, the list sums (AUC, NSS, information gain) and, when the distribution metrics are wanted, the audience's map by
// k_saliency_map unchanged and k_saliency_compare's pixel sums against the prediction (CC, SIM, JSD, KL).
// What the calls promise each other bit for bit is written once and called: sal_walk (the density of a list at a direction:
// k_saliency_map, k_saliency_points; k_congruency_points shares its staging, sal_stage), sal_rule (the summation rule of a
// workgroup, every sum of the rows kernels; cg_wave_rule is the same rule played by one wave), sal_pixel_terms (the comparison
// terms of a pixel: k_saliency_compare, k_score_rows), sal_list_end and sal_row_counts (the tail of a list kernel, the head of a rows
// kernel).  On the host a SalShape holds what a call derives from its arguments, and the launch_* functions are their stages in order.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_angle.hpp"
#include "vet_rank.hpp"
#include "vet_user_dirs.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace vet {

constexpr int SM_THREADS = 256;
constexpr int SM_WAVES = SM_THREADS / WAVE;
constexpr int SM_TILE = 1024;           // list entries per LDS tile (32 KB)
constexpr int SM_BLOCK = 1024;          // positions of one block of the summation rule: four per thread
constexpr int SM_SORT_MAX = 4096;       // positions of a row that k_saliency_sort takes (16 KB of keys)
constexpr int SM_LDS_DIRS = 32768;      // direction tables up to this size are counted in LDS by k_saliency_count (128 KB)
constexpr int SM_PART = 256;            // doubles of the host tables that one k_saliency_tables launch carries
constexpr double SM_PI = 3.141592653589793;

// the host tables, a launch argument at a time: ct [W], st [W] (cos / sin of the column's longitude), sp [H], cp [H] (sin / cos of
// the row's polar angle), ay [H] (the cell's share of the sphere)
struct SalTablePart {
    double v[SM_PART];
    double* dst;
    int n;
};
__global__ __launch_bounds__(SM_THREADS) void k_saliency_tables(const SalTablePart p) {
    const int i = threadIdx.x;
    if (i < p.n) p.dst[i] = p.v[i];
}

// k_saliency_ids — stage 0 of the pooled layout: ids [T][U], status[0] raised once per sample outside [0, 1].
template <bool FROM_IDS>
__global__ __launch_bounds__(SM_THREADS) void k_saliency_ids(const SampleSrc src, const long n, int32_t* __restrict__ ids,
                                                             int32_t* status) {
    const long i = (long)blockIdx.x * SM_THREADS + threadIdx.x;
    bool bad = false;
    if (i < n) ids[i] = sample_dir<FROM_IDS>(src, i, bad);
    if (status) {
        const unsigned long long anybad = __ballot(bad);
        if (anybad && lane_id() == 0) atomicAdd(&status[0], (int)__popcll(anybad));
    }
}

// ------------------------------------------------------------------------------------------
// stage 1: the lists
// ------------------------------------------------------------------------------------------
struct SalListParams {
    const int32_t* ids;          // [T][U], or [U][T] per viewer
    long R, Wpos, D, cap, r0;    // rows per viewer (or of the call), positions per row, directions, list slots per row, first row
    int U, T, stride, per_user, P;
    uint2* list;                 // [rows of the pass][cap]: (id, multiplicity) in ascending id
    int32_t* nlist;              // [rows of the pass] distinct
    unsigned long long* nsamp;   // [rows of the pass] N
    unsigned* dense;             // [rows of the pass][D], zeroed by the host (the long-row path)
};

__device__ __forceinline__ long sal_row(const SalListParams& g, long row) {  // the row's first position in ids
    if (g.per_user) {
        const long u = row / g.R;
        return u * g.T + (row - u * g.R) * g.stride;
    }
    return row * (long)g.stride * g.U;
}

// Where the flagged threads of this step write: base + the flagged threads of lower index.  Every thread of the workgroup calls
// it; base advances by the step's flags.  s_wc: int [4] in LDS.
__device__ __forceinline__ int sal_slot(bool flag, int& base, int* s_wc) {
    const unsigned long long b = __ballot(flag);
    const int wv = wave_id();
    if (lane_id() == 0) s_wc[wv] = (int)__popcll(b);
    __syncthreads();
    int off = base + below(b), tot = 0;
#pragma unroll
    for (int w = 0; w < SM_WAVES; ++w) {
        const int c = s_wc[w];
        off += w < wv ? c : 0;
        tot += c;
    }
    __syncthreads();
    base += tot;
    return off;
}

// The tail of a list kernel: row y's distinct entries (base) and its samples, the threads' counts n added up.  s_n: u64 [4] in LDS.
__device__ __forceinline__ void sal_list_end(const SalListParams& g, long y, int base, unsigned long long n, unsigned long long* s_n) {
    n = wave_sum(n);
    if (lane_id() == 0) s_n[wave_id()] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        g.nlist[y] = base;
        g.nsamp[y] = ((s_n[0] + s_n[1]) + s_n[2]) + s_n[3];
    }
}

// k_saliency_sort — one workgroup per row of up to 4096 positions.  P = the power of two (>= 2) that holds the positions.
__global__ __launch_bounds__(SM_THREADS) void k_saliency_sort(const SalListParams g) {
    __shared__ unsigned keys[SM_SORT_MAX];
    __shared__ int s_wc[SM_WAVES];
    __shared__ unsigned long long s_n[SM_WAVES];
    const int tid = threadIdx.x;
    const long y = blockIdx.x;
    const int32_t* src = g.ids + sal_row(g, g.r0 + y);
    for (int i = tid; i < g.P; i += SM_THREADS) {
        int id = -1;
        if (i < g.Wpos) id = src[i];
        keys[i] = id >= 0 ? (unsigned)id : EMPTY_KEY;
    }
    lds_bitonic_sort(keys, g.P);
    uint2* out = g.list + y * g.cap;
    int base = 0;
    unsigned long long n = 0ull;
    for (int i0 = 0; i0 < g.P; i0 += SM_THREADS) {
        if (keys[i0] == EMPTY_KEY) break;                        // uniform: everything behind is absent
        const int i = i0 + tid;
        const unsigned key = i < g.P ? keys[i] : EMPTY_KEY;
        const bool head = key != EMPTY_KEY && (i == 0 || keys[i - 1] != key);
        n += key != EMPTY_KEY ? 1ull : 0ull;
        const int off = sal_slot(head, base, s_wc);
        if (head) {
            unsigned m = 1u;
            while (i + (int)m < g.P && keys[i + m] == key) ++m;
            out[off] = make_uint2(key, m);
        }
    }
    sal_list_end(g, y, base, n, s_n);
}

// k_saliency_count — the long-row path: workgroup (x, y) strides over the positions of row r0 + y.  LDS_HIST (direction tables of up
// to 32768 entries; dynamic LDS u32 [D]): the workgroup counts in LDS and adds its non-zero counts to the row's dense counts, one
// integer atomic per (workgroup, direction) instead of one per sample.  Integers: exact in any order.
template <bool LDS_HIST>
__global__ __launch_bounds__(SM_THREADS) void k_saliency_count(const SalListParams g) {
    extern __shared__ unsigned s_cnt[];
    const long y = blockIdx.y;
    const int32_t* src = g.ids + sal_row(g, g.r0 + y);
    unsigned* cnt = g.dense + y * g.D;
    if (LDS_HIST) {
        for (int i = threadIdx.x; i < g.D; i += SM_THREADS) s_cnt[i] = 0u;
        __syncthreads();
    }
    for (long q = (long)blockIdx.x * SM_THREADS + threadIdx.x; q < g.Wpos; q += (long)gridDim.x * SM_THREADS) {
        const int id = src[q];
        if (id >= 0) atomicAdd(LDS_HIST ? &s_cnt[id] : &cnt[id], 1u);
    }
    if (LDS_HIST) {
        __syncthreads();
        for (int i = threadIdx.x; i < g.D; i += SM_THREADS) {
            const unsigned c = s_cnt[i];
            if (c) atomicAdd(&cnt[i], c);
        }
    }
}

// k_saliency_compact — one workgroup per row: the dense counts in ascending id.
__global__ __launch_bounds__(SM_THREADS) void k_saliency_compact(const SalListParams g) {
    __shared__ int s_wc[SM_WAVES];
    __shared__ unsigned long long s_n[SM_WAVES];
    const int tid = threadIdx.x;
    const long y = blockIdx.x;
    const unsigned* cnt = g.dense + y * g.D;
    uint2* out = g.list + y * g.cap;
    int base = 0;
    unsigned long long n = 0ull;
    for (long i0 = 0; i0 < g.D; i0 += SM_THREADS) {
        const long i = i0 + tid;
        const unsigned c = i < g.D ? cnt[i] : 0u;
        n += c;
        const int off = sal_slot(c > 0u, base, s_wc);
        if (c > 0u) out[off] = make_uint2((unsigned)i, c);
    }
    sal_list_end(g, y, base, n, s_n);
}

// ------------------------------------------------------------------------------------------
// The density walk.  A staged list entry is 32 B: the unit vector and what its walk needs beside it.
// ------------------------------------------------------------------------------------------
struct SalEntry {                       // sal_walk's: the multiplicity as a double
    double x, y, z, m;
    static __device__ __forceinline__ SalEntry make(const double* A, uint2 e) { return SalEntry{A[0], A[1], A[2], (double)e.y}; }
};
struct CgEntry {                        // k_congruency_points': the id packed next to the multiplicity
    double x, y, z;
    unsigned id, m;
    static __device__ __forceinline__ CgEntry make(const double* A, uint2 e) { return CgEntry{A[0], A[1], A[2], e.x, e.y}; }
};

// One tile: entries [e0, e0 + cnt) of list into s_tile, between the barrier that ends the reads of the tile before and the one
// that publishes this one.  Every thread of the workgroup calls it.
template <class Entry>
__device__ __forceinline__ void sal_stage(Entry* s_tile, const uint2* list, int e0, int cnt, const double* unit) {
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += SM_THREADS) {
        const uint2 e = list[e0 + i];
        s_tile[i] = Entry::make(unit + 3L * e.x, e);
    }
    __syncthreads();
}

// S = the sequential sum over the list's n entries, in ascending id, of m * exp(kappa * (c - 1)) at the direction (Px, Py, Pz): the
// list staged in tiles of `tile` entries, every lane reading the same LDS address (a broadcast).  Every thread of the workgroup
// calls it with the same list.
__device__ __forceinline__ double sal_walk(SalEntry* s_tile, const uint2* list, int n, int tile, const double* unit, double kappa,
                                           double Px, double Py, double Pz) {
    double S = 0.0;
    for (int e0 = 0; e0 < n; e0 += tile) {
        const int cnt = min(tile, n - e0);
        sal_stage(s_tile, list, e0, cnt, unit);
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const SalEntry a = s_tile[j];
            const double c = fma(Pz, a.z, fma(Py, a.y, Px * a.x));
            S = fma(a.m, exp(kappa * (c - 1.0)), S);
        }
    }
    return S;
}

// ------------------------------------------------------------------------------------------
// The summation rule of a 256-thread workgroup over positions [0, n): blocks of 1024 ascending; in a block thread t adds its terms at
// t, t + 256, t + 512, t + 768 in that order, wave_sum, the four waves in order.  K sums are carried together: term(q, t) adds
// position q's K terms into t[0..K), and the block step takes as many sums at a time as s_w has rows (one barrier pair each time).
// The totals end in every thread.  Every thread of the workgroup calls it.
// ------------------------------------------------------------------------------------------
template <int K, int L, class Term>
__device__ __forceinline__ void sal_rule(int n, double (&s_w)[L][SM_WAVES], double (&sum)[K], Term term) {
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
#pragma unroll
    for (int k = 0; k < K; ++k) sum[k] = 0.0;
    for (int b0 = 0; b0 < n; b0 += SM_BLOCK) {
        double t[K];
#pragma unroll
        for (int k = 0; k < K; ++k) t[k] = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = b0 + j * SM_THREADS + tid;
            if (q < n) term(q, t);
        }
#pragma unroll
        for (int k0 = 0; k0 < K; k0 += L) {
#pragma unroll
            for (int k = k0; k < K && k < k0 + L; ++k) {
                const double s = wave_sum(t[k]);
                if (lane == 0) s_w[k - k0][wv] = s;
            }
            __syncthreads();
#pragma unroll
            for (int k = k0; k < K && k < k0 + L; ++k) sum[k] += mo_block_total(s_w[k - k0]);
            __syncthreads();
        }
    }
}

// one sum: term(q, t) adds position q's term into t
template <int L, class Term>
__device__ __forceinline__ double sal_rule1(int n, double (&s_w)[L][SM_WAVES], Term term) {
    double sum[1];
    sal_rule(n, s_w, sum, [&](int q, double (&t)[1]) { term(q, t[0]); });
    return sum[0];
}

// The same rule by ONE wave, which plays the four waves in turn (lane l as thread l, 64 + l, 128 + l, 192 + l): no LDS, no barrier.
// It must give the bits of sal_rule — the same positions per thread in the same order, wave_sum, mo_block_total, the blocks ascending.
template <class Term>
__device__ __forceinline__ double cg_wave_rule(int n, Term term) {
    const int lane = lane_id();
    double acc = 0.0;
    for (int b0 = 0; b0 < n; b0 += SM_BLOCK) {
        double s[SM_WAVES];
#pragma unroll
        for (int w = 0; w < SM_WAVES; ++w) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = b0 + k * SM_THREADS + w * WAVE + lane;
                if (q < n) t += term(q);
            }
            s[w] = wave_sum(t);
        }
        acc += mo_block_total(s);
    }
    return acc;
}

// the rule's sum of M_p * a_y over a map, in every thread: the mass of every call
template <int L>
__device__ __forceinline__ double sal_mass(const double* M, const double* ay, int W, int npix, double (&s_w)[L][SM_WAVES]) {
    return sal_rule1(npix, s_w, [&](int q, double& t) { t += M[q] * ay[q / W]; });
}

// The head of a rows kernel, by thread 0: the row's counts, one plane of [K][rows] each, and status[1] raised for a row that
// cannot be scored.
template <int K>
__device__ __forceinline__ void sal_row_counts(long long* counts, int32_t* status, long rows, long row, const long long (&v)[K],
                                               bool unscored) {
    if (threadIdx.x != 0) return;
    if (counts) {
#pragma unroll
        for (int k = 0; k < K; ++k) counts[k * rows + row] = v[k];
    }
    if (unscored && status) atomicAdd(&status[1], 1);
}

// The comparison terms of one pixel: a and b the two maps' values, ay the cell's share of the sphere, mass_a and mass_b the maps'
// masses.  k_saliency_compare sums all seven; k_score_rows (a = the audience, b = the prediction) leaves vb and kl_ba out.
struct SalPixelTerms {
    double va, vb, cov, sim, jsd, kl_ab, kl_ba;
};
__device__ __forceinline__ SalPixelTerms sal_pixel_terms(double a, double b, double ay, double mass_a, double mass_b) {
    const double qa = (a * ay) / mass_a, qb = (b * ay) / mass_b;
    const double da = a - mass_a, db = b - mass_b;
    const double m = 0.5 * (qa + qb);
    const double ta = qa != 0.0 ? qa * log2(qa / m) : 0.0;
    const double tb = qb != 0.0 ? qb * log2(qb / m) : 0.0;
    SalPixelTerms x;
    x.va = ay * (da * da);
    x.vb = ay * (db * db);
    x.cov = ay * (da * db);
    x.sim = fmin(qa, qb);
    x.jsd = ta + tb;
    x.kl_ab = qa != 0.0 ? qa * log2(qa / qb) : 0.0;
    x.kl_ba = qb != 0.0 ? qb * log2(qb / qa) : 0.0;
    return x;
}

// ------------------------------------------------------------------------------------------
// k_saliency_map — stage 2.  grid (ceil(W * H / 256), rows of the pass); thread = pixel blockIdx.x * 256 + tid of row blockIdx.y.
// LDS: SalEntry [1024] static (32 KB).  S is sal_walk's sum over the list at the pixel's direction; M = S * g_r, the multiply
// skipped at scale 0.  A row without a sample writes +0.0.
// Resources (hipcc, gfx950, -Rpass-analysis=kernel-resource-usage): 69 VGPRs, no scratch, 32 768 B LDS, 5 waves per SIMD (LDS-bound).
// ------------------------------------------------------------------------------------------
struct SalMapParams {
    const uint2* list;
    const int32_t* nlist;
    const unsigned long long* nsamp;
    const double* unit;          // [n_dirs][3]
    const double* tab;           // ct [W] | st [W] | sp [H] | cp [H] | ay [H]
    long cap, out_row0;
    int W, H, tile, scale;
    double kappa, C;
    double* out;                 // row (out_row0 + y) of [..][H][W]
};

__global__ __launch_bounds__(SM_THREADS) void k_saliency_map(const SalMapParams p) {
    __shared__ SalEntry s_tile[SM_TILE];
    const int tid = threadIdx.x;
    const long y = blockIdx.y;
    const int npix = p.W * p.H, px = blockIdx.x * SM_THREADS + tid;
    double Px = 0.0, Py = 0.0, Pz = 0.0;
    if (px < npix) {                     // Vector.from_spherical of the cell centre, normalised: k_heatmap_map's arithmetic
        const int r = px / p.W, c = px - r * p.W;
        const double sp = p.tab[2 * p.W + r], cp = p.tab[2 * p.W + p.H + r];
        const double x = sp * p.tab[c], yy = sp * p.tab[p.W + c], z = cp;
        const double len = sqrt(x * x + yy * yy + z * z);
        Px = x / len; Py = yy / len; Pz = z / len;
    }
    const double S = sal_walk(s_tile, p.list + y * p.cap, p.nlist[y], p.tile, p.unit, p.kappa, Px, Py, Pz);
    if (px < npix) {
        const unsigned long long N = p.nsamp[y];
        double M = S;
        if (N == 0ull) M = 0.0;
        else if (p.scale == 1) M = S * (1.0 / (double)N);
        else if (p.scale == 2) M = S * (p.C / (double)N);
        p.out[(p.out_row0 + y) * (long)npix + px] = M;
    }
}

// ------------------------------------------------------------------------------------------
// k_saliency_rows — stage 3, one workgroup per row of the pass.
// ------------------------------------------------------------------------------------------
struct SalRowParams {
    const double* map;           // row (map_row0 + y), or null: only the counts are wanted
    const double* ay;            // [H]
    const int32_t* nlist;
    const unsigned long long* nsamp;
    long map_row0, r0, rows;
    int W, H;
    double* stats;               // [4][rows] or null
    int32_t* peak;               // [rows] or null
    long long* counts;           // [2][rows] or null
    int32_t* status;             // [2] or null
};

__global__ __launch_bounds__(SM_THREADS) void k_saliency_rows(const SalRowParams p) {
    __shared__ double s_w[1][SM_WAVES];
    __shared__ unsigned long long s_bits[SM_WAVES];
    __shared__ int s_idx[SM_WAVES];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const long y = blockIdx.x, row = p.r0 + y;
    const unsigned long long N = p.nsamp[y];
    sal_row_counts(p.counts, p.status, p.rows, row, {(long long)N, (long long)p.nlist[y]}, N == 0ull);
    if (!p.map || (!p.stats && !p.peak)) return;
    if (N == 0ull) {                                             // uniform
        const double nan = __builtin_nan("");
        if (tid < 4 && p.stats) p.stats[tid * p.rows + row] = nan;
        if (tid == 0 && p.peak) p.peak[row] = -1;
        return;
    }
    const int npix = p.W * p.H;
    const double* M = p.map + (p.map_row0 + y) * (long)npix;
    unsigned long long bb = 0ull;
    int bi = 0x7FFFFFFF;
    const double mass = sal_rule1(npix, s_w, [&](int q, double& t) {    // sal_mass' terms, the peak tracked on the way
        const double m = M[q];
        t += m * p.ay[q / p.W];
        const unsigned long long bits = (unsigned long long)__double_as_longlong(m);
        if (bits > bb || (bits == bb && q < bi)) { bb = bits; bi = q; }
    });
    for (int o = 32; o > 0; o >>= 1) {                           // the largest value bits, the smallest index that holds them
        const unsigned long long ob = (unsigned long long)__shfl_xor((long long)bb, o, WAVE);
        const int oi = __shfl_xor(bi, o, WAVE);
        if (ob > bb || (ob == bb && oi < bi)) { bb = ob; bi = oi; }
    }
    if (lane == 0) { s_bits[wv] = bb; s_idx[wv] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SM_WAVES; ++w)
            if (s_bits[w] > bb || (s_bits[w] == bb && s_idx[w] < bi)) { bb = s_bits[w]; bi = s_idx[w]; }
        if (p.peak) p.peak[row] = bi;
        if (p.stats) { p.stats[row] = mass; p.stats[p.rows + row] = __longlong_as_double((long long)bb); }
    }
    if (!p.stats) return;
    const double ent = sal_rule1(npix, s_w, [&](int q, double& t) {     // Wsum is the mass: the same terms by the same rule
        const double a = p.ay[q / p.W], w = M[q] * a;
        if (w != 0.0) {
            const double qq = w / mass;
            t += qq * log2(qq / a);
        }
    });
    if (tid == 0) {
        p.stats[2 * p.rows + row] = -ent;
        p.stats[3 * p.rows + row] = exp2(-ent);
    }
}

// ------------------------------------------------------------------------------------------
// Saliency similarity (vet_saliency_similarity*): two audiences of one video, their maps compared row by row.
// k_saliency_mask — after stage 0: the ids [T][U] once more per audience, every other viewer's samples -1.  The list and map kernels
// above then run on each copy unchanged, so an audience's list and map are vet_saliency_ids' on the masked ids by construction.
// Resources: 14 VGPRs, no scratch, no LDS, 8 waves per SIMD.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_THREADS) void k_saliency_mask(const int32_t* __restrict__ ids, const unsigned char* __restrict__ groups,
                                                              const long n, const int U, int32_t* __restrict__ ids_a,
                                                              int32_t* __restrict__ ids_b) {
    const long i = (long)blockIdx.x * SM_THREADS + threadIdx.x;
    if (i >= n) return;
    const int id = ids[i];
    const unsigned char g = groups[i % U];
    ids_a[i] = g == 0 ? id : -1;
    ids_b[i] = g == 1 ? id : -1;
}

// ------------------------------------------------------------------------------------------
// k_saliency_points — NSS by point evaluation.  grid (ceil(cap / 256), rows of the pass, 2); blockIdx.z = 0: X = A on Y = B's
// density (nss_ab), 1: X = B on Y = A.  Thread = entry blockIdx.x * 256 + tid of X's list with its unit vector in registers; S is
// sal_walk's sum over Y's list — k_saliency_map's, the cell direction replaced by the entry's.  Writes v_i = m_i * (S_i * g_Y) to
// pts [2][CR][cap].  Rows with an empty audience write nothing.
// Resources (hipcc, gfx950, -Rpass-analysis=kernel-resource-usage): 77 VGPRs, no scratch, 32 768 B LDS, 5 waves per SIMD (LDS-bound).
// ------------------------------------------------------------------------------------------
struct SalPointParams {
    const uint2* list[2];        // A, B: [rows of the pass][cap]
    const int32_t* nlist[2];
    const unsigned long long* nsamp[2];
    const double* unit;          // [n_dirs][3]
    long cap, CR;
    int tile;
    double kappa, C;
    double* pts;                 // [2][CR][cap]
};

__global__ __launch_bounds__(SM_THREADS) void k_saliency_points(const SalPointParams p) {
    __shared__ SalEntry s_tile[SM_TILE];
    const int tid = threadIdx.x;
    const long y = blockIdx.y;
    const int dx = blockIdx.z, dy = dx ^ 1;
    const int nx = p.nlist[dx][y], n = p.nlist[dy][y];
    const int i = blockIdx.x * SM_THREADS + tid;
    if ((int)blockIdx.x * SM_THREADS >= nx || n == 0) return;   // uniform
    double Px = 0.0, Py = 0.0, Pz = 0.0, mi = 0.0;
    if (i < nx) {
        const uint2 e = p.list[dx][y * p.cap + i];
        const double* A = p.unit + 3L * e.x;
        Px = A[0]; Py = A[1]; Pz = A[2]; mi = (double)e.y;
    }
    const double S = sal_walk(s_tile, p.list[dy] + y * p.cap, n, p.tile, p.unit, p.kappa, Px, Py, Pz);
    if (i < nx) {
        const double g = p.C / (double)p.nsamp[dy][y];
        p.pts[((long)dx * p.CR + y) * p.cap + i] = mi * (S * g);
    }
}

// ------------------------------------------------------------------------------------------
// k_saliency_compare — one workgroup per row of the pass: the two masses (sal_mass: k_saliency_rows' bits), one pass over both maps
// with the seven sums of sal_pixel_terms carried together through the rule's block step, the v_i of both directions by the rule
// over the list positions, then the nine values, the counts and status[1].
// Resources (hipcc, gfx950, -Rpass-analysis=kernel-resource-usage): 97 VGPRs, no scratch, 224 B LDS, 4 waves per SIMD.
// ------------------------------------------------------------------------------------------
constexpr int SC_SUMS = 7;              // va, vb, cov, sim, jsd, kl_ab, kl_ba
struct SalCompareParams {
    const double* map[2];        // row (map_row0 + y) of each audience's maps, or null: only the counts are wanted
    const double* ay;            // [H]
    const int32_t* nlist[2];
    const unsigned long long* nsamp[2];
    const double* pts;           // [2][CR][cap]
    long cap, CR, map_row0, r0, rows;
    int W, H;
    double* stats;               // [9][rows] or null
    long long* counts;           // [4][rows] or null
    int32_t* status;             // [2] or null
};

__global__ __launch_bounds__(SM_THREADS) void k_saliency_compare(const SalCompareParams p) {
    __shared__ double s_w[SC_SUMS][SM_WAVES];
    const int tid = threadIdx.x;
    const long y = blockIdx.x, row = p.r0 + y;
    const unsigned long long NA = p.nsamp[0][y], NB = p.nsamp[1][y];
    const int na = p.nlist[0][y], nb = p.nlist[1][y];
    const bool empty = NA == 0ull || NB == 0ull;
    sal_row_counts(p.counts, p.status, p.rows, row, {(long long)NA, (long long)NB, (long long)na, (long long)nb}, empty);
    if (!p.stats) return;
    const int npix = p.W * p.H;
    const double* MA = p.map[0] + (p.map_row0 + y) * (long)npix;
    const double* MB = p.map[1] + (p.map_row0 + y) * (long)npix;
    const double nan = __builtin_nan("");
    const double mass_a = NA ? sal_mass(MA, p.ay, p.W, npix, s_w) : nan;
    const double mass_b = NB ? sal_mass(MB, p.ay, p.W, npix, s_w) : nan;
    if (empty) {                                                 // uniform
        if (tid < 7) p.stats[tid * p.rows + row] = nan;
        if (tid == 0) { p.stats[7 * p.rows + row] = mass_a; p.stats[8 * p.rows + row] = mass_b; }
        return;
    }
    double sum[SC_SUMS];
    sal_rule(npix, s_w, sum, [&](int q, double (&t)[SC_SUMS]) {
        const SalPixelTerms x = sal_pixel_terms(MA[q], MB[q], p.ay[q / p.W], mass_a, mass_b);
        t[0] += x.va;
        t[1] += x.vb;
        t[2] += x.cov;
        t[3] += x.sim;
        t[4] += x.jsd;
        t[5] += x.kl_ab;
        t[6] += x.kl_ba;
    });
    double V[2];                                                 // the v_i of X = A, then of X = B, over the list positions
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const double* v = p.pts + ((long)d * p.CR + y) * p.cap;
        V[d] = sal_rule1(d ? nb : na, s_w, [&](int q, double& t) { t += v[q]; });
    }
    if (tid == 0) {
        const double va = sum[0], vb = sum[1];
        p.stats[row] = sum[2] / sqrt(va * vb);
        p.stats[p.rows + row] = sum[3];
        p.stats[2 * p.rows + row] = 0.5 * sum[4];
        p.stats[3 * p.rows + row] = sum[5];
        p.stats[4 * p.rows + row] = sum[6];
        p.stats[5 * p.rows + row] = (V[0] / (double)NA - mass_b) / sqrt(vb);
        p.stats[6 * p.rows + row] = (V[1] / (double)NB - mass_a) / sqrt(va);
        p.stats[7 * p.rows + row] = mass_a;
        p.stats[8 * p.rows + row] = mass_b;
    }
}

// ------------------------------------------------------------------------------------------
// Viewer congruency (vet_congruency*): how well the rest of the audience predicts where a viewer looks — the leave-one-out density
// of the others at the viewer's own directions, without a map.  Stage 0 runs for both layouts, the list stage once pooled and once
// per viewer per pass of rows (the kernels above, unchanged).
// k_congruency_points<NSS> — grid (ceil(U * cap_u / 256), rows of the pass); thread = query q = u * cap_u + slot: entry `slot` of
// viewer u's own list of the row, its unit vector in registers.  The row's pooled list is staged in LDS in tiles by sal_stage, as
// sal_walk stages it, the entry's id packed next to its multiplicity (CgEntry: 32 B an entry still), and read as a broadcast.  Both
// lists ascend in id: the thread holds the id and multiplicity of its viewer's NEXT own entry and, on a match, takes that
// multiplicity off the step's weight and moves on in the own list (global memory, cache-resident) — one integer compare per step,
// w = m - a an integer, no difference of densities.  NSS: the step also adds m * G into T and, on a match, a * G into O (one sqrt,
// exp, expm1 and division more per pair), and the query that sits on its own direction notes the pooled position, where it leaves T
// for the row's Q (every viewer that holds the direction writes the same bits).  A workgroup without an active query returns; a wave
// without one skips the walk, not the barriers of the staging.
// Resources (hipcc, gfx950, -Rpass-analysis=kernel-resource-usage): <false> 64 VGPRs, <true> 96 VGPRs; neither uses scratch;
// 32 768 B LDS (the workgroup's "any query" flag lives in the tile before the first staging); 5 waves per SIMD (LDS-bound).
// ------------------------------------------------------------------------------------------
struct CgPointParams {
    const uint2* plist;          // pooled [rows of the pass][cap_p]
    const int32_t* pn;
    const uint2* ulist;          // per viewer [U][rows of the pass][cap_u]
    const int32_t* un;
    const double* unit;          // [n_dirs][3]
    long cap_p, cap_u, cr, plane;
    int U, tile;
    double kappa, g0;            // g0 = 4 pi exp(-2 kappa)
    double* qs;                  // S [CR][U][cap_u]; NSS: T and O behind it, `plane` doubles apart
    double* tp;                  // NSS: T at the pooled positions [CR][cap_p]
};

constexpr double CG_TWOPI = 2.0 * SM_PI, CG_FOURPI = 4.0 * SM_PI;

// the integral of two kernels' product over the sphere, from the cosine between their centres
__device__ __forceinline__ double cg_overlap(double c, double kappa, double g0) {
    const double r = sqrt(fmax(0.0, fma(2.0, c, 2.0)));
    const double x = kappa * r;
    if (x < 1e-4) return g0 * (1.0 + (x * x) / 6.0);
    return ((CG_TWOPI * exp(kappa * (r - 2.0))) * (-expm1(-2.0 * x))) / x;
}

template <bool NSS>
__global__ __launch_bounds__(SM_THREADS) void k_congruency_points(const CgPointParams p) {
    __shared__ CgEntry s_tile[SM_TILE];
    int& s_any = *(int*)s_tile;                                  // read by all before the first staging barrier
    const int tid = threadIdx.x;
    const long y = blockIdx.y;
    const long q = (long)blockIdx.x * SM_THREADS + tid;
    int u = 0, slot = 0, nown = 0;
    if (q < (long)p.U * p.cap_u) {
        u = (int)(q / p.cap_u);
        slot = (int)(q - (long)u * p.cap_u);
        nown = p.un[(long)u * p.cr + y];
    }
    const bool active = slot < nown;
    if (tid == 0) s_any = 0;
    __syncthreads();
    if (active) s_any = 1;
    __syncthreads();
    if (!s_any) return;                                          // uniform
    const uint2* own = p.ulist + ((long)u * p.cr + y) * p.cap_u;
    double Px = 0.0, Py = 0.0, Pz = 0.0;
    unsigned nid = EMPTY_KEY, na = 0u;                           // the viewer's next own entry
    int ptr = 0, jpos = 0;
    if (active) {
        const double* A = p.unit + 3L * own[slot].x;
        Px = A[0]; Py = A[1]; Pz = A[2];
        const uint2 e = own[0];
        nid = e.x; na = e.y;
    }
    const bool wave_on = __ballot(active) != 0ull;
    const int n = p.pn[y];
    const uint2* list = p.plist + y * p.cap_p;
    const double kappa = p.kappa, g0 = p.g0;
    double S = 0.0, T = 0.0, O = 0.0;
    for (int e0 = 0; e0 < n; e0 += p.tile) {
        const int cnt = min(p.tile, n - e0);
        sal_stage(s_tile, list, e0, cnt, p.unit);
        if (!wave_on) continue;
#pragma unroll 2
        for (int j = 0; j < cnt; ++j) {                          // the same address in every lane: a broadcast
            const CgEntry a = s_tile[j];
            const double c = fma(Pz, a.z, fma(Py, a.y, Px * a.x));
            const double k = exp(kappa * (c - 1.0));
            double G = 0.0;
            if (NSS) {
                G = cg_overlap(c, kappa, g0);
                T = fma((double)a.m, G, T);
            }
            unsigned w = a.m;
            if (a.id == nid) {
                w -= na;
                if (NSS) {
                    O = fma((double)na, G, O);
                    if (ptr == slot) jpos = e0 + j;
                }
                ++ptr;
                nid = EMPTY_KEY;
                if (ptr < nown) {
                    const uint2 e = own[ptr];
                    nid = e.x; na = e.y;
                }
            }
            S = fma((double)w, k, S);
        }
    }
    if (active) {
        const long o = (y * p.U + u) * p.cap_u + slot;
        p.qs[o] = S;
        if (NSS) {
            p.qs[p.plane + o] = T;
            p.qs[2 * p.plane + o] = O;
            p.tp[y * p.cap_p + jpos] = T;
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_congruency_users — one wave per (row, viewer), four to a workgroup: the own-entry sums F = sum a_i f_i, L = sum a_i log2(4 pi f_i)
// and, with NSS, B = sum a_i T_i and A = sum a_i O_i by the rule over the own-list positions (cg_wave_rule: the bits of a 256-thread
// workgroup; no LDS, no barrier).
// Resources: 94 VGPRs, no scratch, no LDS, 5 waves per SIMD.
// ------------------------------------------------------------------------------------------
struct CgUserParams {
    const uint2* ulist;
    const int32_t* un;
    const unsigned long long* uns;   // n_u [U][rows of the pass]
    const unsigned long long* pns;   // N [rows of the pass]
    const double* qs;
    long cap_u, cr, plane;
    int U, nss;
    double C;
    double* sums;                // [rows of the pass][U][4]: F, L, B, A
};

__global__ __launch_bounds__(SM_THREADS) void k_congruency_users(const CgUserParams p) {
    const long pair = (long)blockIdx.x * SM_WAVES + wave_id();
    if (pair >= p.cr * p.U) return;                              // uniform in the wave
    const long y = pair / p.U;
    const int u = (int)(pair - y * p.U);
    const long ur = (long)u * p.cr + y;
    const unsigned long long nu = p.uns[ur], N = p.pns[y];
    double F = 0.0, L = 0.0, B = 0.0, A = 0.0;
    if (nu > 0ull && N > nu) {
        const int n = p.un[ur];
        const uint2* own = p.ulist + ur * p.cap_u;
        const double* S = p.qs + (y * p.U + u) * p.cap_u;
        const double g = p.C / (double)(N - nu);
        F = cg_wave_rule(n, [&](int i) { return (double)own[i].y * (S[i] * g); });
        L = cg_wave_rule(n, [&](int i) { return (double)own[i].y * log2(CG_FOURPI * (S[i] * g)); });
        if (p.nss) {
            B = cg_wave_rule(n, [&](int i) { return (double)own[i].y * S[p.plane + i]; });
            A = cg_wave_rule(n, [&](int i) { return (double)own[i].y * S[2 * p.plane + i]; });
        }
    }
    if (lane_id() == 0) {
        double* o = p.sums + pair * 4;
        o[0] = F; o[1] = L; o[2] = B; o[3] = A;
    }
}

// ------------------------------------------------------------------------------------------
// k_congruency_rows — one workgroup per row of the pass: Q = sum_j m_j T_j by the rule over the pooled list's positions, then by the
// rule over the viewer index the three statistics of every viewer (written on the way), the scored viewers and their sums (one
// row of LDS: the four sums take the block step in turn).
// Resources: 122 VGPRs, no scratch, 32 B LDS, 4 waves per SIMD.
// ------------------------------------------------------------------------------------------
struct CgRowParams {
    const uint2* plist;
    const int32_t* pn;
    const unsigned long long* pns;
    const int32_t* un;
    const unsigned long long* uns;
    const double* tp;
    const double* sums;          // null: only the counts are wanted
    long cap_p, cr, r0, rows;
    int U, nss;
    double C;
    double* stats;               // [3][U][rows] or null
    long long* counts;           // [3][U][rows] or null
    double* out_rows;            // [4][rows] or null
    int32_t* status;             // [2] or null
};

__global__ __launch_bounds__(SM_THREADS) void k_congruency_rows(const CgRowParams p) {
    __shared__ double s_w[1][SM_WAVES];
    const int tid = threadIdx.x;
    const long y = blockIdx.x, row = p.r0 + y;
    const unsigned long long N = p.pns[y];
    const double nan = __builtin_nan("");
    double Q = 0.0;
    if (p.sums && p.nss) {
        const uint2* list = p.plist + y * p.cap_p;
        const double* T = p.tp + y * p.cap_p;
        Q = sal_rule1(p.pn[y], s_w, [&](int q, double& t) { t += (double)list[q].y * T[q]; });
    }
    const double mu = 1.0 / CG_FOURPI;
    double sum[4];                                               // lift, gain, nss, the scored viewers
    sal_rule(p.U, s_w, sum, [&](int u, double (&t)[4]) {
        const long ur = (long)u * p.cr + y, o = (long)u * p.rows + row, plane = (long)p.U * p.rows;
        const unsigned long long nu = p.uns[ur];
        if (p.counts) {
            p.counts[o] = (long long)nu;
            p.counts[plane + o] = (long long)p.un[ur];
            p.counts[2 * plane + o] = (long long)(N - nu);
        }
        const bool scored = nu > 0ull && N > nu;
        t[3] += scored ? 1.0 : 0.0;
        if (p.sums) {
            double lift = nan, gain = nan, nss = nan;
            if (scored) {
                const double* s = p.sums + (y * p.U + u) * 4;
                const double F = s[0];
                lift = (CG_FOURPI * F) / (double)nu;
                gain = s[1] / (double)nu;
                if (p.nss) {
                    const double g = p.C / (double)(N - nu);
                    const double Qu = (Q - 2.0 * s[2]) + s[3];
                    const double v = ((g * g) * Qu) / CG_FOURPI - mu * mu;
                    if (v > 0.0 && v < __builtin_inf()) nss = (F / (double)nu - mu) / sqrt(v);
                }
                t[0] += lift; t[1] += gain; t[2] += nss;
            }
            if (p.stats) {
                p.stats[o] = lift;
                p.stats[plane + o] = gain;
                p.stats[2 * plane + o] = nss;
            }
        }
    });
    const double sc = sum[3];
    if (tid == 0 && p.sums) {
        if (p.out_rows) {
            p.out_rows[row] = sc;
            p.out_rows[p.rows + row] = sum[0] / sc;
            p.out_rows[2 * p.rows + row] = sum[1] / sc;
            p.out_rows[3 * p.rows + row] = sum[2] / sc;
        }
    }
    if (tid == 0 && p.status && sc == 0.0) atomicAdd(&p.status[1], 1);   // fewer than two viewers present
}

// ------------------------------------------------------------------------------------------
// Saliency scoring (vet_saliency_score*): how well a map from elsewhere predicts where the audience looked.  The row's list is
// the pooled list of the kernels above; the audience's own map (k_saliency_map, scale 2) is built only for the distribution metrics.
// k_score_sort — workgroup = (map row y, map of the launch): the row's W values as u64 bit patterns in LDS (non-negative doubles order
// as their bits; -0.0 enters as +0.0), padded to the power of two P with all-ones, lds_bitonic_sort, the first W written to
// sorted [maps][H][W].  A static map is sorted once per call, per-row maps once per pass.
// Resources (hipcc, gfx950, -Rpass-analysis=kernel-resource-usage): 10 VGPRs, no scratch, 32 768 B LDS, 5 waves per SIMD (LDS-bound).
// ------------------------------------------------------------------------------------------
constexpr int SS_SORT_MAX = 4096;       // the widest map row k_score_sort takes (32 KB of keys): vet_saliency's limit on W
constexpr int SS_TILE = 4096;           // sorted values of one LDS tile of k_score_points (32 KB), filled in whole map rows

struct ScoreSortParams {
    const double* pred;          // [maps][H][W]
    unsigned long long* sorted;  // [maps of the launch][H][W]
    long map0;                   // the launch's first map in pred
    int W, P;
};

__global__ __launch_bounds__(SM_THREADS) void k_score_sort(const ScoreSortParams p) {
    __shared__ unsigned long long keys[SS_SORT_MAX];
    const int tid = threadIdx.x;
    const long H = gridDim.x;
    const double* src = p.pred + ((p.map0 + blockIdx.y) * H + blockIdx.x) * p.W;
    for (int i = tid; i < p.P; i += SM_THREADS)
        keys[i] = i < p.W ? (unsigned long long)__double_as_longlong(src[i] + 0.0) : ~0ull;
    lds_bitonic_sort(keys, p.P);
    unsigned long long* out = p.sorted + ((long)blockIdx.y * H + blockIdx.x) * p.W;
    for (int i = tid; i < p.W; i += SM_THREADS) out[i] = keys[i];
}

// The map P [H][W] at the unit vector (x, y, z) by bilinear interpolation on the cell-centre grid: the columns wrap, the rows clamp.
// a + t * (b - a): four equal corners return their value exactly.  Every index is brought into the map whatever the vector holds.
__device__ __forceinline__ double score_sample(const double* __restrict__ P, int W, int H, double x, double y, double z) {
    const double lon = (x == 0.0 && y == 0.0) ? 0.0 : atan2(y, x);
    const double fx = (lon + SM_PI) / (2.0 * SM_PI) * (double)W - 0.5;
    const double flx = floor(fx), tx = fx - flx;
    int c0 = (int)flx % W;
    if (c0 < 0) c0 += W;
    const int c1 = c0 + 1 == W ? 0 : c0 + 1;
    const double fy = fmin(fmax(acos(fmin(fmax(z, -1.0), 1.0)) / SM_PI * (double)H - 0.5, 0.0), (double)(H - 1));
    const double fly = floor(fy), ty = fy - fly;
    const int y0 = min(max((int)fly, 0), H - 1), y1 = min(y0 + 1, H - 1);
    const double* r0 = P + (long)y0 * W;
    const double* r1 = P + (long)y1 * W;
    const double top = r0[c0] + tx * (r0[c1] - r0[c0]);
    const double bot = r1[c0] + tx * (r1[c1] - r1[c0]);
    return top + ty * (bot - top);
}

// ------------------------------------------------------------------------------------------
// k_score_points — grid (ceil(cap / 256), rows of the pass); thread = entry blockIdx.x * 256 + tid of the row's list.  v_i = the
// row's predicted map at the entry's direction (four loads).  The sorted map rows are staged in LDS in tiles of whole map rows (at
// most 4096 values); per map row one lower- and one upper-bound binary search of W values (the same trip count in every lane)
// gives the integer counts #{P < v} and #{P <= v}; L and E stay in registers, added in ascending y.  Writes v_i and
// u_i = L + 0.5 * E to pts [2][CR][cap].  A workgroup beyond the list returns.
// Resources (hipcc, gfx950, -Rpass-analysis=kernel-resource-usage): 28 VGPRs, no scratch, 32 768 B LDS, 5 waves per SIMD (LDS-bound).
// ------------------------------------------------------------------------------------------
struct ScorePointParams {
    const uint2* list;           // [rows of the pass][cap]
    const int32_t* nlist;
    const double* unit;          // [n_dirs][3]
    const double* pred;          // the map of row y: pred + (r0 + y) * pred_stride (0: one static map)
    const double* sorted;        // its sorted rows: sorted + y * sorted_stride
    const double* ay;            // [H]
    long cap, CR, r0, pred_stride, sorted_stride;
    int W, H, tile_rows;
    double* pts;                 // [2][CR][cap]
};

__global__ __launch_bounds__(SM_THREADS) void k_score_points(const ScorePointParams p) {
    __shared__ double s_tile[SS_TILE];
    const int tid = threadIdx.x, W = p.W;
    const long y = blockIdx.y;
    const int n = p.nlist[y];
    if ((int)blockIdx.x * SM_THREADS >= n) return;               // uniform
    const int i = blockIdx.x * SM_THREADS + tid;
    const double* S = p.sorted + y * p.sorted_stride;
    double v = 0.0;
    if (i < n) {
        const double* A = p.unit + 3L * p.list[y * p.cap + i].x;
        v = score_sample(p.pred + (p.r0 + y) * p.pred_stride, W, p.H, A[0], A[1], A[2]);
    }
    double L = 0.0, E = 0.0;
    for (int y0 = 0; y0 < p.H; y0 += p.tile_rows) {
        const int nr = min(p.tile_rows, p.H - y0), cnt = nr * W;
        __syncthreads();                                         // the readers of the tile before
        for (int j = tid; j < cnt; j += SM_THREADS) s_tile[j] = S[(long)y0 * W + j];
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            const double* row = s_tile + r * W;
            int lo = 0, hi = 0, len = W;
            while (len > 1) {                                    // uniform: the trip count depends on W alone
                const int half = len >> 1;
                lo += row[lo + half - 1] < v ? half : 0;
                hi += row[hi + half - 1] <= v ? half : 0;
                len -= half;
            }
            lo += row[lo] < v ? 1 : 0;
            hi += row[hi] <= v ? 1 : 0;
            const double a = p.ay[y0 + r];
            L = L + a * (double)lo;
            E = E + a * (double)(hi - lo);
        }
    }
    if (i < n) {
        p.pts[y * p.cap + i] = v;
        p.pts[(p.CR + y) * p.cap + i] = L + 0.5 * E;
    }
}

// ------------------------------------------------------------------------------------------
// k_score_rows — one workgroup per row of the pass: mass_pred (sal_mass) and var_pred by the rule (sal_pixel_terms' vb terms), the
// three list sums carried together by the rule over the list positions, with the audience's map its mass and five of the sums of
// sal_pixel_terms (a = the audience, b = the prediction) carried together through the rule's block step; then the nine values,
// the counts and status[1].
// Resources (hipcc, gfx950, -Rpass-analysis=kernel-resource-usage): 93 VGPRs, no scratch, 160 B LDS, 5 waves per SIMD.
// ------------------------------------------------------------------------------------------
constexpr int SR_SUMS = 5;              // va, cov, sim, jsd, kl
struct ScoreRowParams {
    const double* pred;          // the map of row r: pred + r * pred_stride (0: one static map)
    const double* map;           // row (map_row0 + y) of the audience's maps, or null: no distribution metrics
    const double* ay;            // [H]
    const uint2* list;
    const int32_t* nlist;
    const unsigned long long* nsamp;
    const double* pts;           // [2][CR][cap]
    long cap, CR, pred_stride, map_row0, r0, rows;
    int W, H;
    double* stats;               // [9][rows] or null
    long long* counts;           // [2][rows] or null
    int32_t* status;             // [2] or null
};

__global__ __launch_bounds__(SM_THREADS) void k_score_rows(const ScoreRowParams p) {
    __shared__ double s_w[SR_SUMS][SM_WAVES];
    const int tid = threadIdx.x;
    const long y = blockIdx.x, row = p.r0 + y;
    const unsigned long long N = p.nsamp[y];
    const int n = p.nlist[y];
    sal_row_counts(p.counts, p.status, p.rows, row, {(long long)N, (long long)n}, N == 0ull);
    if (!p.stats) return;
    const int npix = p.W * p.H;
    const double* P = p.pred + row * p.pred_stride;
    const double nan = __builtin_nan("");
    const double mass_p = sal_mass(P, p.ay, p.W, npix, s_w);
    const double var_p = sal_rule1(npix, s_w, [&](int q, double& t) {
        const double db = P[q] - mass_p;
        t += p.ay[q / p.W] * (db * db);
    });
    if (N == 0ull) {                                             // uniform
        if (tid < 8) p.stats[tid * p.rows + row] = nan;
        if (tid == 0) p.stats[8 * p.rows + row] = mass_p;
        return;
    }
    const uint2* list = p.list + y * p.cap;
    const double* pv = p.pts + y * p.cap;
    const double* pu = p.pts + (p.CR + y) * p.cap;
    double ls[3];                                                // sum m v, sum m log2(v / mass_pred), sum m u
    sal_rule(n, s_w, ls, [&](int q, double (&t)[3]) {
        const double m = (double)list[q].y, v = pv[q];
        t[0] += m * v;
        t[1] += m * log2(v / mass_p);
        t[2] += m * pu[q];
    });
    double mass_a = nan, sum[SR_SUMS] = {};
    if (p.map) {                                                 // uniform
        const double* M = p.map + (p.map_row0 + y) * (long)npix;
        mass_a = sal_mass(M, p.ay, p.W, npix, s_w);
        sal_rule(npix, s_w, sum, [&](int q, double (&t)[SR_SUMS]) {
            const SalPixelTerms x = sal_pixel_terms(M[q], P[q], p.ay[q / p.W], mass_a, mass_p);
            t[0] += x.va;
            t[1] += x.cov;
            t[2] += x.sim;
            t[3] += x.jsd;
            t[4] += x.kl_ab;
        });
    }
    if (tid == 0) {
        const double Nd = (double)N;
        p.stats[row] = ls[2] / Nd;
        p.stats[p.rows + row] = (ls[0] / Nd - mass_p) / sqrt(var_p);
        p.stats[2 * p.rows + row] = ls[1] / Nd;
        p.stats[3 * p.rows + row] = p.map ? sum[1] / sqrt(sum[0] * var_p) : nan;
        p.stats[4 * p.rows + row] = p.map ? sum[2] : nan;
        p.stats[5 * p.rows + row] = p.map ? 0.5 * sum[3] : nan;
        p.stats[6 * p.rows + row] = p.map ? sum[4] : nan;
        p.stats[7 * p.rows + row] = mass_a;
        p.stats[8 * p.rows + row] = mass_p;
    }
}

}  // namespace vet

namespace vh {

// What vet_saliency* refuse about their arguments, before anything is staged, allocated or launched.
int check_saliency_args(const vet_plan* pl, int U, int T, int window, int stride, int per_user, double sigma, int W, int H, int scale) {
    if (!pl) return fail(VET_ERR_INVALID, "plan is NULL");
    if (U <= 0 || T <= 0) return fail(VET_ERR_INVALID, "n_users and n_frames must be positive (got %d, %d)", U, T);
    if (window < 1) return fail(VET_ERR_INVALID, "window must be at least 1 frame (got %d)", window);
    if (stride < 1) return fail(VET_ERR_INVALID, "stride must be at least 1 frame (got %d)", stride);
    if (window > T) return fail(VET_ERR_INVALID, "window of %d frames is longer than the video's %d frames", window, T);
    if (!std::isfinite(sigma) || !(sigma > 0.0) || sigma > vet::SM_PI)
        return fail(VET_ERR_INVALID, "sigma_rad must be finite, above 0 and at most pi (got %g)", sigma);
    if (W < 2 || W > 4096) return fail(VET_ERR_INVALID, "the map needs 2 to 4096 columns (got %d)", W);
    if (H < 1 || H > 2048) return fail(VET_ERR_INVALID, "the map needs 1 to 2048 rows (got %d)", H);
    if (scale < 0 || scale > 2) return fail(VET_ERR_INVALID, "scale must be 0, 1 or 2 (got %d)", scale);
    if (per_user) {
        const int rc = check_user_dirs_frames(T, "saliency");
        if (rc) return rc;
    } else if (((int64_t)U * T + vet::SM_THREADS - 1) / vet::SM_THREADS > (int64_t)0x7FFFFFFF) {
        return fail(VET_ERR_UNSUPPORTED, "saliency: %d frames of %d viewers in one call (at most 2^31 - 1 workgroups)", T, U);
    }
    return VET_OK;
}

namespace {

constexpr size_t kSaliencyPassBudget = (size_t)256 << 20;     // bytes of per-row workspace a pass may take

// The samples of a call as its entry got them: (mu, mv) with the name of the _ids twin for entry_samples' message, or ids alone.
struct SalSamples {
    const double* mu;
    const double* mv;
    const int32_t* ids;
    const char* ids_entry;
};

// After a call's own refusals (rc): what entry_samples refuses, and the stream the call launches on.
int entry_stream(int rc, const vet_plan* pl, const SalSamples& in, void* stream, hipStream_t* s) {
    return rc ? rc : entry_samples(pl, in.mu, in.mv, in.ids, in.ids_entry, stream, s);
}

// What a call derives from its arguments, once: the rows and their lists in one layout (pooled or per viewer), the map and the kernel.
struct SalShape {
    int U, T, stride, per_user, W, H;
    long R, rows, Wpos, D, cap, npix;    // rows per viewer, rows of the layout, positions per row, directions, list slots, pixels
    bool sorted;                         // the rows go to k_saliency_sort, in LDS arrays of P keys
    int P, tile;
    double kappa, C;                     // 1 / sigma^2; the kernel's normalisation on the sphere
    size_t ntab, ay;                     // doubles of the host tables; where ay starts in them
};

SalShape sal_shape(const vet_plan* pl, int U, int T, int window, int stride, int per_user, double sigma, int W, int H) {
    SalShape h{};
    h.U = U; h.T = T; h.stride = stride; h.per_user = per_user ? 1 : 0; h.W = W; h.H = H;
    h.R = (long)vet_window_rows(T, window, stride);
    h.rows = per_user ? h.R * U : h.R;
    h.Wpos = per_user ? window : (long)window * U;
    h.D = (long)pl->n_dirs;
    h.cap = std::min(h.Wpos, h.D);
    h.npix = (long)W * H;
    h.sorted = h.Wpos <= vet::SM_SORT_MAX;
    h.P = 2;
    while (h.sorted && h.P < h.Wpos) h.P <<= 1;
    h.tile = vet::SM_TILE;
    if (pl->ctx->tune.saliency_tile > 0) h.tile = std::min(h.tile, pl->ctx->tune.saliency_tile);
    h.kappa = 1.0 / (sigma * sigma);
    h.C = h.kappa / (2.0 * vet::SM_PI * (1.0 - std::exp(-2.0 * h.kappa)));
    h.ntab = (size_t)2 * W + (size_t)3 * H;
    h.ay = (size_t)2 * W + 2 * (size_t)H;
    return h;
}

// the rows of a pass: what the budget holds at per_row bytes a row, at least one, at most a grid dimension
long pass_rows(size_t per_row, long rows, size_t budget = kSaliencyPassBudget) {
    return std::max(1L, std::min({(long)(budget / per_row), rows, 65535L}));
}

// The host tables of the shape's W x H map (ct | st | sp | cp | ay) written to tab on s: np.radians is x * (pi / 180).
int saliency_tables(vet_ctx* c, const SalShape& sh, double* tab, hipStream_t s) {
    ProfScope ps(c, s, KID_TRANSITION);
    const int W = sh.W, H = sh.H;
    const size_t ntab = sh.ntab;
    std::vector<double> h(ntab);
    constexpr double kRad = vet::SM_PI / 180.0, kPi = vet::SM_PI;
    for (int x = 0; x < W; ++x) {
        const double lon = ((double)x + 0.5) / (double)W * 360.0 - 180.0, theta = lon * kRad;
        h[x] = std::cos(theta); h[(size_t)W + x] = std::sin(theta);
    }
    for (int y = 0; y < H; ++y) {
        const double lat = 90.0 - ((double)y + 0.5) / (double)H * 180.0, phi = (90.0 - lat) * kRad;
        h[(size_t)2 * W + y] = std::sin(phi); h[(size_t)2 * W + H + y] = std::cos(phi);
        h[sh.ay + y] =
            (std::cos(kPi * (double)y / (double)H) - std::cos(kPi * (double)(y + 1) / (double)H)) / (2.0 * (double)W);
    }
    for (size_t o = 0; o < ntab; o += vet::SM_PART) {
        vet::SalTablePart q;
        q.n = (int)std::min((size_t)vet::SM_PART, ntab - o);
        for (int i = 0; i < q.n; ++i) q.v[i] = h[o + i];
        for (int i = q.n; i < vet::SM_PART; ++i) q.v[i] = 0.0;
        q.dst = tab + o;
        hipLaunchKernelGGL(vet::k_saliency_tables, dim3(1), dim3(vet::SM_THREADS), 0, s, q);
        HIP_TRY(hipGetLastError());
    }
    return VET_OK;
}

// Stage 0 (the caller holds the stage's ProfScope).  Pooled: ids [T][U]; per viewer: ids [U][T].
int stage0_pooled(const vet_plan* pl, const SalSamples& in, int U, int T, int32_t* ids, int32_t* d_status, hipStream_t s) {
    const vet::SampleSrc src{in.mu, in.mv, in.ids, pl->W, pl->H, (long)pl->n_dirs};
    const long n = (long)T * U;
    const dim3 grid((unsigned)((n + vet::SM_THREADS - 1) / vet::SM_THREADS));
    if (in.ids) hipLaunchKernelGGL(vet::k_saliency_ids<true>, grid, dim3(vet::SM_THREADS), 0, s, src, n, ids, d_status);
    else hipLaunchKernelGGL(vet::k_saliency_ids<false>, grid, dim3(vet::SM_THREADS), 0, s, src, n, ids, d_status);
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

int stage0_per_viewer(const vet_plan* pl, const SalSamples& in, int U, int T, int32_t* ids, int32_t* d_status, hipStream_t s) {
    vet::UserDirsParams q{};
    q.src = vet::SampleSrc{in.mu, in.mv, in.ids, pl->W, pl->H, (long)pl->n_dirs};
    q.U = U; q.T = T; q.dirs = ids; q.status = d_status;
    const dim3 grid((unsigned)((U + vet::UT - 1) / vet::UT), (unsigned)((T + vet::UT - 1) / vet::UT));
    if (in.ids) hipLaunchKernelGGL(vet::k_user_dirs<true>, grid, dim3(256), 0, s, q);
    else hipLaunchKernelGGL(vet::k_user_dirs<false>, grid, dim3(256), 0, s, q);
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

// The list stage's arguments for the rows of h read from ids; r0 is the pass's to set.
vet::SalListParams list_params(const SalShape& h, const int32_t* ids, uint2* list, int32_t* nlist, unsigned long long* nsamp,
                               unsigned* dense) {
    vet::SalListParams g{};
    g.ids = ids; g.R = h.R; g.Wpos = h.Wpos; g.D = h.D; g.cap = h.cap;
    g.U = h.U; g.T = h.T; g.stride = h.stride; g.per_user = h.per_user; g.P = h.P;
    g.list = list; g.nlist = nlist; g.nsamp = nsamp; g.dense = dense;
    return g;
}

// The list stage of cr rows from g.r0: the LDS sort, or the dense counts and their compaction.
int saliency_lists(vet_ctx* c, const vet::SalListParams& g, bool sorted, long cr, hipStream_t s) {
    ProfScope ps(c, s, KID_TRANSITION);
    if (sorted) {
        hipLaunchKernelGGL(vet::k_saliency_sort, dim3((unsigned)cr), dim3(vet::SM_THREADS), 0, s, g);
        HIP_TRY(hipGetLastError());
        return VET_OK;
    }
    HIP_TRY(hipMemsetAsync(g.dense, 0, (size_t)cr * g.D * 4, s));
    if (g.D <= vet::SM_LDS_DIRS) {                               // 16384 positions or more per workgroup, at most 64 workgroups a row
        const long gx = std::max(1L, std::min(g.Wpos / 16384, 64L));
        hipLaunchKernelGGL(vet::k_saliency_count<true>, dim3((unsigned)gx, (unsigned)cr), dim3(vet::SM_THREADS), (size_t)g.D * 4, s, g);
    } else {
        const long gx = std::min((g.Wpos + vet::SM_THREADS - 1) / vet::SM_THREADS, 4096L);
        hipLaunchKernelGGL(vet::k_saliency_count<false>, dim3((unsigned)gx, (unsigned)cr), dim3(vet::SM_THREADS), 0, s, g);
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(vet::k_saliency_compact, dim3((unsigned)cr), dim3(vet::SM_THREADS), 0, s, g);
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

// Stage 2 of a pass: the maps of the cr rows whose lists g holds, written from row out_row0 of out.
int saliency_maps(const vet_plan* pl, const SalShape& h, const vet::SalListParams& g, const double* tab, int scale, double* out,
                  long out_row0, long cr, hipStream_t s) {
    vet::SalMapParams m{};
    m.list = g.list; m.nlist = g.nlist; m.nsamp = g.nsamp; m.unit = pl->d_dir_unit; m.tab = tab; m.cap = h.cap;
    m.W = h.W; m.H = h.H; m.tile = h.tile; m.scale = scale; m.kappa = h.kappa; m.C = h.C;
    m.out = out; m.out_row0 = out_row0;
    ProfScope pm(pl->ctx, s, KID_SPATIAL);
    const dim3 grid((unsigned)((h.npix + vet::SM_THREADS - 1) / vet::SM_THREADS), (unsigned)cr);
    hipLaunchKernelGGL(vet::k_saliency_map, grid, dim3(vet::SM_THREADS), 0, s, m);
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

// vet_saliency*: stage 0, the tables, then per pass of rows the lists, the maps and the rows.
int launch_saliency(vet_plan* pl, const SalSamples& in, int U, int T, int window, int stride, int per_user, double sigma, int W, int H,
                    int scale, double* d_map, double* d_stats, int32_t* d_peak, int64_t* d_counts, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = entry_stream(check_saliency_args(pl, U, T, window, stride, per_user, sigma, W, H, scale), pl, in, stream, &s);
    if (rc) return rc;
    vet_ctx* c = pl->ctx;
    const SalShape h = sal_shape(pl, U, T, window, stride, per_user, sigma, W, H);
    const bool want_map = d_map || d_stats || d_peak;
    const long CR = pass_rows((size_t)h.cap * 8 + 16 + (h.sorted ? 0 : (size_t)h.D * 4) + (want_map && !d_map ? (size_t)h.npix * 8 : 0),
                              h.rows);
    // workspace: the ids | the host tables | of a pass: the lists, their lengths, N, the dense counts, the maps
    WsLayout lay;
    const size_t ids_o = lay.take<int32_t>((size_t)T * U), tab_o = lay.take<double>(h.ntab), list_o = lay.take<uint2>((size_t)CR * h.cap),
                 nl_o = lay.take<int32_t>((size_t)CR), ns_o = lay.take<unsigned long long>((size_t)CR),
                 dense_o = lay.take<uint32_t>(h.sorted ? 0 : (size_t)CR * h.D),
                 map_o = lay.take<double>(want_map && !d_map ? (size_t)CR * h.npix : 0);
    rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    int32_t* ids = (int32_t*)(ws + ids_o);
    double* tab = (double*)(ws + tab_o);
    double* maps = d_map ? d_map : (double*)(ws + map_o);
    {   // stage 0
        ProfScope ps(c, s, KID_TRANSITION);
        rc = per_user ? stage0_per_viewer(pl, in, U, T, ids, d_status, s) : stage0_pooled(pl, in, U, T, ids, d_status, s);
        if (rc) return rc;
    }
    if (want_map) {
        rc = saliency_tables(c, h, tab, s);
        if (rc) return rc;
    }
    vet::SalListParams g = list_params(h, ids, (uint2*)(ws + list_o), (int32_t*)(ws + nl_o), (unsigned long long*)(ws + ns_o),
                                       (unsigned*)(ws + dense_o));
    vet::SalRowParams q{};
    q.map = want_map ? maps : nullptr; q.ay = tab + h.ay; q.nlist = g.nlist; q.nsamp = g.nsamp; q.rows = h.rows;
    q.W = W; q.H = H; q.stats = d_stats; q.peak = d_peak; q.counts = (long long*)d_counts; q.status = d_status;
    const bool want_rows = d_stats || d_peak || d_counts || d_status;
    for (long r0 = 0; r0 < h.rows; r0 += CR) {
        const long cr = std::min(CR, h.rows - r0);
        g.r0 = r0;
        rc = saliency_lists(c, g, h.sorted, cr, s);
        if (rc) return rc;
        q.map_row0 = d_map ? r0 : 0; q.r0 = r0;
        if (want_map) {
            rc = saliency_maps(pl, h, g, tab, scale, maps, q.map_row0, cr, s);
            if (rc) return rc;
        }
        if (want_rows) {
            ProfScope ps(c, s, KID_TRANSITION);
            hipLaunchKernelGGL(vet::k_saliency_rows, dim3((unsigned)cr), dim3(vet::SM_THREADS), 0, s, q);
            HIP_TRY(hipGetLastError());
        }
    }
    return VET_OK;
}

// vet_saliency_similarity*: stage 0 on all viewers, the mask, then per pass of rows the lists and maps of A and of B by the kernels
// of vet_saliency, the point evaluations and the comparison.  The dense counts of the long-row path serve A, then B.
int launch_similarity(vet_plan* pl, const SalSamples& in, int U, int T, int window, int stride, const int8_t* groups, double sigma, int W,
                      int H, double* d_maps, double* d_stats, int64_t* d_counts, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = entry_stream(check_similarity_args(pl, U, T, window, stride, groups, sigma, W, H), pl, in, stream, &s);
    if (rc) return rc;
    vet_ctx* c = pl->ctx;
    const SalShape h = sal_shape(pl, U, T, window, stride, 0, sigma, W, H);
    const long R = h.R, cap = h.cap, npix = h.npix, n = (long)T * U;
    const bool want_map = d_maps || d_stats;
    // per row of a pass: two lists with their lengths and N, the dense counts, two maps when they stay here, the v_i of both directions
    const long CR = pass_rows((size_t)2 * cap * 8 + 32 + (h.sorted ? 0 : (size_t)h.D * 4) +
                                  (want_map && !d_maps ? (size_t)2 * npix * 8 : 0) + (d_stats ? (size_t)2 * cap * 8 : 0),
                              R);
    WsLayout lay;
    const size_t ids_o = lay.take<int32_t>((size_t)n), ida_o = lay.take<int32_t>((size_t)n), idb_o = lay.take<int32_t>((size_t)n),
                 tab_o = lay.take<double>(h.ntab), list_o = lay.take<uint2>((size_t)2 * CR * cap), nl_o = lay.take<int32_t>((size_t)2 * CR),
                 ns_o = lay.take<unsigned long long>((size_t)2 * CR), dense_o = lay.take<uint32_t>(h.sorted ? 0 : (size_t)CR * h.D),
                 map_o = lay.take<double>(want_map && !d_maps ? (size_t)2 * CR * npix : 0),
                 pts_o = lay.take<double>(d_stats ? (size_t)2 * CR * cap : 0);
    rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    int32_t* ids = (int32_t*)(ws + ids_o);
    int32_t* ids_g[2] = {(int32_t*)(ws + ida_o), (int32_t*)(ws + idb_o)};
    double* tab = (double*)(ws + tab_o);
    BatchBlob blob;                                              // the labels as bytes; the host array is read before the call returns
    rc = blob.acquire(c, pad16((size_t)U));
    if (rc) return rc;
    for (int u = 0; u < U; ++u) ((unsigned char*)blob.host())[u] = (unsigned char)groups[u];
    rc = blob.upload(s);
    if (rc) return rc;
    {   // stage 0 on every viewer (status[0] counts the excluded viewers' samples too), then the mask
        ProfScope ps(c, s, KID_TRANSITION);
        rc = stage0_pooled(pl, in, U, T, ids, d_status, s);
        if (rc) return rc;
        hipLaunchKernelGGL(vet::k_saliency_mask, dim3((unsigned)((n + vet::SM_THREADS - 1) / vet::SM_THREADS)), dim3(vet::SM_THREADS), 0,
                           s, ids, (const unsigned char*)blob.dev(), n, U, ids_g[0], ids_g[1]);
        HIP_TRY(hipGetLastError());
    }
    if (want_map) {
        rc = saliency_tables(c, h, tab, s);
        if (rc) return rc;
    }
    vet::SalListParams g[2];
    double* maps[2];
    vet::SalPointParams pt{};
    vet::SalCompareParams q{};
    for (int a = 0; a < 2; ++a) {
        g[a] = list_params(h, ids_g[a], (uint2*)(ws + list_o) + (size_t)a * CR * cap, (int32_t*)(ws + nl_o) + (size_t)a * CR,
                           (unsigned long long*)(ws + ns_o) + (size_t)a * CR, (unsigned*)(ws + dense_o));
        maps[a] = d_maps ? d_maps + (size_t)a * R * npix : (double*)(ws + map_o) + (size_t)a * CR * npix;
        pt.list[a] = g[a].list; pt.nlist[a] = g[a].nlist; pt.nsamp[a] = g[a].nsamp;
        q.map[a] = want_map ? maps[a] : nullptr; q.nlist[a] = g[a].nlist; q.nsamp[a] = g[a].nsamp;
    }
    pt.unit = pl->d_dir_unit; pt.cap = cap; pt.CR = CR; pt.tile = h.tile; pt.kappa = h.kappa; pt.C = h.C; pt.pts = (double*)(ws + pts_o);
    q.ay = tab + h.ay; q.pts = pt.pts; q.cap = cap; q.CR = CR; q.rows = R; q.W = W; q.H = H;
    q.stats = d_stats; q.counts = (long long*)d_counts; q.status = d_status;
    const bool want_rows = d_stats || d_counts || d_status;
    for (long r0 = 0; r0 < R; r0 += CR) {
        const long cr = std::min(CR, R - r0);
        q.map_row0 = d_maps ? r0 : 0; q.r0 = r0;
        for (int a = 0; a < 2; ++a) {
            g[a].r0 = r0;
            rc = saliency_lists(c, g[a], h.sorted, cr, s);
            if (!rc && want_map) rc = saliency_maps(pl, h, g[a], tab, 2, maps[a], q.map_row0, cr, s);
            if (rc) return rc;
        }
        if (d_stats) {
            ProfScope pp(c, s, KID_SPATIAL);
            const dim3 grid((unsigned)((cap + vet::SM_THREADS - 1) / vet::SM_THREADS), (unsigned)cr, 2);
            hipLaunchKernelGGL(vet::k_saliency_points, grid, dim3(vet::SM_THREADS), 0, s, pt);
            HIP_TRY(hipGetLastError());
        }
        if (want_rows) {
            ProfScope ps(c, s, KID_TRANSITION);
            hipLaunchKernelGGL(vet::k_saliency_compare, dim3((unsigned)cr), dim3(vet::SM_THREADS), 0, s, q);
            HIP_TRY(hipGetLastError());
        }
    }
    return VET_OK;
}

// vet_congruency*: stage 0 for both layouts, then per pass of rows the pooled lists, every viewer's own lists of the same rows, the
// point walk, the own-entry sums and the rows.  The list kernels index a per-viewer row as u * R + r: a pass hands them R = the rows
// of the pass and the ids from the pass's first frame on, so the own lists of a pass are [U][rows of the pass].  The dense counts of
// the long-row path serve the pooled lists, then the viewers' in chunks of the rows they hold.
int launch_congruency(vet_plan* pl, const SalSamples& in, int U, int T, int window, int stride, double sigma, int want_nss,
                      double* d_stats, int64_t* d_counts, double* d_rows, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = entry_stream(check_congruency_args(pl, U, T, window, stride, sigma), pl, in, stream, &s);
    if (rc) return rc;
    vet_ctx* c = pl->ctx;
    const SalShape hp = sal_shape(pl, U, T, window, stride, 0, sigma, 0, 0), hu = sal_shape(pl, U, T, window, stride, 1, sigma, 0, 0);
    const long R = hp.R, D = hp.D, cap_p = hp.cap, cap_u = hu.cap, n = (long)T * U;
    const bool want_vals = d_stats || d_rows, nss = want_vals && want_nss;
    // the dense counts take up to half the budget (at least a row), the rows of a pass the rest
    const long dense_rows = hp.sorted ? 0 : std::max(1L, std::min((long)(kSaliencyPassBudget / 2 / ((size_t)D * 4)), 65535L));
    const size_t per_row = (size_t)cap_p * 8 + 16 + (size_t)U * ((size_t)cap_u * 8 + 16) +
                           (want_vals ? (size_t)U * cap_u * (nss ? 24 : 8) + (size_t)U * 32 + (nss ? (size_t)cap_p * 8 : 0) : 0);
    long CR = std::min(pass_rows(per_row, R, hp.sorted ? kSaliencyPassBudget : kSaliencyPassBudget / 2), (long)0x7FFFFFFF / U);
    if (!hp.sorted) CR = std::min(CR, dense_rows);
    const size_t plane = (size_t)CR * U * cap_u;
    WsLayout lay;
    const size_t idp_o = lay.take<int32_t>((size_t)n), idu_o = lay.take<int32_t>((size_t)n),
                 pl_o = lay.take<uint2>((size_t)CR * cap_p), pn_o = lay.take<int32_t>((size_t)CR),
                 ps_o = lay.take<unsigned long long>((size_t)CR), ul_o = lay.take<uint2>((size_t)CR * U * cap_u),
                 un_o = lay.take<int32_t>((size_t)CR * U), us_o = lay.take<unsigned long long>((size_t)CR * U),
                 dense_o = lay.take<uint32_t>((size_t)dense_rows * D), qs_o = lay.take<double>(want_vals ? plane * (nss ? 3 : 1) : 0),
                 tp_o = lay.take<double>(nss ? (size_t)CR * cap_p : 0), sum_o = lay.take<double>(want_vals ? (size_t)CR * U * 4 : 0);
    rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    int32_t* ids_p = (int32_t*)(ws + idp_o);
    int32_t* ids_u = (int32_t*)(ws + idu_o);
    {   // stage 0, both layouts; status[0] is raised by the pooled one alone
        ProfScope ps(c, s, KID_TRANSITION);
        rc = stage0_pooled(pl, in, U, T, ids_p, d_status, s);
        if (!rc) rc = stage0_per_viewer(pl, in, U, T, ids_u, nullptr, s);
        if (rc) return rc;
    }
    uint2* ulist = (uint2*)(ws + ul_o);
    int32_t* un = (int32_t*)(ws + un_o);
    unsigned long long* uns = (unsigned long long*)(ws + us_o);
    vet::SalListParams gp = list_params(hp, ids_p, (uint2*)(ws + pl_o), (int32_t*)(ws + pn_o), (unsigned long long*)(ws + ps_o),
                                        (unsigned*)(ws + dense_o));
    vet::SalListParams gu = list_params(hu, ids_u, ulist, un, uns, gp.dense);    // ids, R, r0 and the outputs are the chunk's to set
    vet::CgPointParams pt{};
    pt.plist = gp.list; pt.pn = gp.nlist; pt.ulist = ulist; pt.un = un; pt.unit = pl->d_dir_unit; pt.cap_p = cap_p; pt.cap_u = cap_u;
    pt.plane = (long)plane; pt.U = U; pt.tile = hp.tile; pt.kappa = hp.kappa; pt.g0 = 4.0 * vet::SM_PI * std::exp(-2.0 * hp.kappa);
    pt.qs = (double*)(ws + qs_o); pt.tp = (double*)(ws + tp_o);
    vet::CgUserParams us{};
    us.ulist = ulist; us.un = un; us.uns = uns; us.pns = gp.nsamp; us.qs = pt.qs; us.cap_u = cap_u; us.plane = (long)plane; us.U = U;
    us.nss = nss ? 1 : 0; us.C = hp.C; us.sums = (double*)(ws + sum_o);
    vet::CgRowParams q{};
    q.plist = gp.list; q.pn = gp.nlist; q.pns = gp.nsamp; q.un = un; q.uns = uns; q.tp = pt.tp; q.sums = want_vals ? us.sums : nullptr;
    q.cap_p = cap_p; q.rows = R; q.U = U; q.nss = us.nss; q.C = hp.C; q.stats = d_stats; q.counts = (long long*)d_counts;
    q.out_rows = d_rows; q.status = d_status;
    for (long r0 = 0; r0 < R; r0 += CR) {
        const long cr = std::min(CR, R - r0);
        gp.r0 = r0;
        rc = saliency_lists(c, gp, hp.sorted, cr, s);
        if (rc) return rc;
        gu.ids = ids_u + r0 * stride; gu.R = cr;
        const long urows = cr * U, chunk = hu.sorted ? urows : dense_rows;
        for (long c0 = 0; c0 < urows; c0 += chunk) {
            gu.r0 = c0; gu.list = ulist + c0 * cap_u; gu.nlist = un + c0; gu.nsamp = uns + c0;
            rc = saliency_lists(c, gu, hu.sorted, std::min(chunk, urows - c0), s);
            if (rc) return rc;
        }
        if (want_vals) {
            {
                ProfScope pp(c, s, KID_SPATIAL);
                pt.cr = cr;
                const dim3 grid((unsigned)(((long)U * cap_u + vet::SM_THREADS - 1) / vet::SM_THREADS), (unsigned)cr);
                if (nss) hipLaunchKernelGGL(vet::k_congruency_points<true>, grid, dim3(vet::SM_THREADS), 0, s, pt);
                else hipLaunchKernelGGL(vet::k_congruency_points<false>, grid, dim3(vet::SM_THREADS), 0, s, pt);
                HIP_TRY(hipGetLastError());
            }
            ProfScope pu(c, s, KID_TRANSITION);
            us.cr = cr;
            hipLaunchKernelGGL(vet::k_congruency_users, dim3((unsigned)((urows + vet::SM_WAVES - 1) / vet::SM_WAVES)),
                               dim3(vet::SM_THREADS), 0, s, us);
            HIP_TRY(hipGetLastError());
        }
        if (d_stats || d_rows || d_counts || d_status) {
            ProfScope ps(c, s, KID_TRANSITION);
            q.cr = cr; q.r0 = r0;
            hipLaunchKernelGGL(vet::k_congruency_rows, dim3((unsigned)cr), dim3(vet::SM_THREADS), 0, s, q);
            HIP_TRY(hipGetLastError());
        }
    }
    return VET_OK;
}

// vet_saliency_score*: stage 0, the tables, a static map's sorted rows once, then per pass of rows the lists, the audience's maps
// (only for the distribution metrics or d_map), the sorted rows of the pass's own predicted maps, the point walk and the rows.
int launch_score(vet_plan* pl, const SalSamples& in, int U, int T, int window, int stride, double sigma, int W, int H,
                 const double* d_pred, int n_pred, int want_dist, double* d_map, double* d_stats, int64_t* d_counts, int32_t* d_status,
                 void* stream) {
    hipStream_t s;
    int rc = entry_stream(check_score_args(pl, U, T, window, stride, sigma, W, H, d_pred, n_pred), pl, in, stream, &s);
    if (rc) return rc;
    vet_ctx* c = pl->ctx;
    const SalShape h = sal_shape(pl, U, T, window, stride, 0, sigma, W, H);
    const long R = h.R, cap = h.cap, npix = h.npix;
    const bool is_static = n_pred == 1;
    const bool want_map = d_map || (d_stats && want_dist);
    // per row of a pass: the list with its length and N, the dense counts, the audience's map when it stays here, the sorted copy of
    // the row's own predicted map, v_i and u_i
    const long CR = pass_rows((size_t)cap * 8 + 16 + (h.sorted ? 0 : (size_t)h.D * 4) + (want_map && !d_map ? (size_t)npix * 8 : 0) +
                                  (d_stats ? (is_static ? 0 : (size_t)npix * 8) + (size_t)2 * cap * 8 : 0),
                              R);
    WsLayout lay;
    const size_t ids_o = lay.take<int32_t>((size_t)T * U), tab_o = lay.take<double>(h.ntab), list_o = lay.take<uint2>((size_t)CR * cap),
                 nl_o = lay.take<int32_t>((size_t)CR), ns_o = lay.take<unsigned long long>((size_t)CR),
                 dense_o = lay.take<uint32_t>(h.sorted ? 0 : (size_t)CR * h.D),
                 map_o = lay.take<double>(want_map && !d_map ? (size_t)CR * npix : 0),
                 srt_o = lay.take<double>(d_stats ? (size_t)(is_static ? 1 : CR) * npix : 0),
                 pts_o = lay.take<double>(d_stats ? (size_t)2 * CR * cap : 0);
    rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    int32_t* ids = (int32_t*)(ws + ids_o);
    double* tab = (double*)(ws + tab_o);
    double* maps = d_map ? d_map : (double*)(ws + map_o);
    {   // stage 0
        ProfScope ps(c, s, KID_TRANSITION);
        rc = stage0_pooled(pl, in, U, T, ids, d_status, s);
        if (rc) return rc;
    }
    if (want_map || d_stats) {
        rc = saliency_tables(c, h, tab, s);
        if (rc) return rc;
    }
    vet::SalListParams g = list_params(h, ids, (uint2*)(ws + list_o), (int32_t*)(ws + nl_o), (unsigned long long*)(ws + ns_o),
                                       (unsigned*)(ws + dense_o));
    vet::ScoreSortParams so{};
    so.pred = d_pred; so.sorted = (unsigned long long*)(ws + srt_o); so.W = W;
    so.P = 2;
    while (so.P < W) so.P <<= 1;
    vet::ScorePointParams pt{};
    pt.list = g.list; pt.nlist = g.nlist; pt.unit = pl->d_dir_unit; pt.pred = d_pred; pt.sorted = (const double*)(ws + srt_o);
    pt.ay = tab + h.ay; pt.cap = cap; pt.CR = CR; pt.pred_stride = is_static ? 0 : npix;
    pt.sorted_stride = pt.pred_stride; pt.W = W; pt.H = H; pt.tile_rows = std::max(1, vet::SS_TILE / W); pt.pts = (double*)(ws + pts_o);
    vet::ScoreRowParams q{};
    q.pred = d_pred; q.map = d_stats && want_dist ? maps : nullptr; q.ay = pt.ay; q.list = g.list; q.nlist = g.nlist; q.nsamp = g.nsamp;
    q.pts = pt.pts; q.cap = cap; q.CR = CR; q.pred_stride = pt.pred_stride; q.rows = R; q.W = W; q.H = H;
    q.stats = d_stats; q.counts = (long long*)d_counts; q.status = d_status;
    if (d_stats && is_static) {
        ProfScope ps(c, s, KID_TRANSITION);
        so.map0 = 0;
        hipLaunchKernelGGL(vet::k_score_sort, dim3((unsigned)H, 1), dim3(vet::SM_THREADS), 0, s, so);
        HIP_TRY(hipGetLastError());
    }
    const bool want_rows = d_stats || d_counts || d_status;
    for (long r0 = 0; r0 < R; r0 += CR) {
        const long cr = std::min(CR, R - r0);
        g.r0 = r0;
        rc = saliency_lists(c, g, h.sorted, cr, s);
        if (rc) return rc;
        q.map_row0 = d_map ? r0 : 0; q.r0 = r0;
        if (want_map) {
            rc = saliency_maps(pl, h, g, tab, 2, maps, q.map_row0, cr, s);
            if (rc) return rc;
        }
        if (d_stats) {
            if (!is_static) {
                ProfScope ps(c, s, KID_TRANSITION);
                so.map0 = r0;
                hipLaunchKernelGGL(vet::k_score_sort, dim3((unsigned)H, (unsigned)cr), dim3(vet::SM_THREADS), 0, s, so);
                HIP_TRY(hipGetLastError());
            }
            ProfScope pp(c, s, KID_SPATIAL);
            pt.r0 = r0;
            const dim3 grid((unsigned)((cap + vet::SM_THREADS - 1) / vet::SM_THREADS), (unsigned)cr);
            hipLaunchKernelGGL(vet::k_score_points, grid, dim3(vet::SM_THREADS), 0, s, pt);
            HIP_TRY(hipGetLastError());
        }
        if (want_rows) {
            ProfScope ps(c, s, KID_TRANSITION);
            hipLaunchKernelGGL(vet::k_score_rows, dim3((unsigned)cr), dim3(vet::SM_THREADS), 0, s, q);
            HIP_TRY(hipGetLastError());
        }
    }
    return VET_OK;
}

}  // namespace

// What vet_saliency_score* refuse: check_saliency_args for the pooled layout at scale 2, pred NULL, n_pred other than 1 or the rows.
int check_score_args(const vet_plan* pl, int U, int T, int window, int stride, double sigma, int W, int H, const double* pred,
                     int n_pred) {
    int rc = check_saliency_args(pl, U, T, window, stride, 0, sigma, W, H, 2);
    if (rc) return rc;
    if (!pred) return fail(VET_ERR_INVALID, "pred is NULL");
    const int64_t R = vet_window_rows(T, window, stride);
    if (n_pred != 1 && (int64_t)n_pred != R)
        return fail(VET_ERR_INVALID, "n_pred must be 1 (a static map) or the %lld rows of the call (got %d)", (long long)R, n_pred);
    return VET_OK;
}

// What vet_congruency* refuse: check_saliency_args for both layouts (sigma, window, stride, the frames a per-viewer call takes), and
// fewer than two viewers.
int check_congruency_args(const vet_plan* pl, int U, int T, int window, int stride, double sigma) {
    int rc = check_saliency_args(pl, U, T, window, stride, 0, sigma, 2, 1, 0);
    if (!rc) rc = check_saliency_args(pl, U, T, window, stride, 1, sigma, 2, 1, 0);
    if (rc) return rc;
    if (U < 2) return fail(VET_ERR_INVALID, "congruency needs at least two viewers (got %d)", U);
    return VET_OK;
}

// What vet_saliency_similarity* refuse: check_saliency_args for the pooled layout at scale 2, groups NULL, an audience without a viewer.
int check_similarity_args(const vet_plan* pl, int U, int T, int window, int stride, const int8_t* groups, double sigma, int W, int H) {
    int rc = check_saliency_args(pl, U, T, window, stride, 0, sigma, W, H, 2);
    if (rc) return rc;
    if (!groups) return fail(VET_ERR_INVALID, "groups is NULL");
    int na = 0, nb = 0;
    for (int u = 0; u < U; ++u) {
        na += groups[u] == 0;
        nb += groups[u] == 1;
    }
    if (na < 1 || nb < 1) return fail(VET_ERR_INVALID, "both audiences need a viewer (got %d in A, %d in B)", na, nb);
    return VET_OK;
}

int saliency_set_attrs(vet_ctx*) {
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_saliency_count<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                vet::SM_LDS_DIRS * 4));
    return VET_OK;
}

}  // namespace vh

using namespace vh;

// The device entries: each call's (d_mu, d_mv) entry and its _ids twin hand their samples to the one body of the call.
extern "C" {

int vet_saliency(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, int per_user,
                 double sigma_rad, int W, int H, int scale, double* d_map, double* d_stats, int32_t* d_peak, int64_t* d_counts,
                 int32_t* d_status, void* stream) {
    return launch_saliency(pl, {d_mu, d_mv, nullptr, "vet_saliency_ids"}, U, T, window, stride, per_user, sigma_rad, W, H, scale, d_map,
                           d_stats, d_peak, d_counts, d_status, stream);
}

int vet_saliency_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, int per_user, double sigma_rad, int W,
                     int H, int scale, double* d_map, double* d_stats, int32_t* d_peak, int64_t* d_counts, int32_t* d_status,
                     void* stream) {
    return launch_saliency(pl, {nullptr, nullptr, d_ids, nullptr}, U, T, window, stride, per_user, sigma_rad, W, H, scale, d_map,
                           d_stats, d_peak, d_counts, d_status, stream);
}

int vet_saliency_similarity(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride,
                            const int8_t* groups, double sigma_rad, int W, int H, double* d_maps, double* d_stats, int64_t* d_counts,
                            int32_t* d_status, void* stream) {
    return launch_similarity(pl, {d_mu, d_mv, nullptr, "vet_saliency_similarity_ids"}, U, T, window, stride, groups, sigma_rad, W, H,
                             d_maps, d_stats, d_counts, d_status, stream);
}

int vet_saliency_similarity_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, const int8_t* groups,
                                double sigma_rad, int W, int H, double* d_maps, double* d_stats, int64_t* d_counts, int32_t* d_status,
                                void* stream) {
    return launch_similarity(pl, {nullptr, nullptr, d_ids, nullptr}, U, T, window, stride, groups, sigma_rad, W, H, d_maps, d_stats,
                             d_counts, d_status, stream);
}

int vet_saliency_score(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, double sigma_rad,
                       int W, int H, const double* d_pred, int n_pred, int want_dist, double* d_map, double* d_stats, int64_t* d_counts,
                       int32_t* d_status, void* stream) {
    return launch_score(pl, {d_mu, d_mv, nullptr, "vet_saliency_score_ids"}, U, T, window, stride, sigma_rad, W, H, d_pred, n_pred,
                        want_dist, d_map, d_stats, d_counts, d_status, stream);
}

int vet_saliency_score_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, double sigma_rad, int W, int H,
                           const double* d_pred, int n_pred, int want_dist, double* d_map, double* d_stats, int64_t* d_counts,
                           int32_t* d_status, void* stream) {
    return launch_score(pl, {nullptr, nullptr, d_ids, nullptr}, U, T, window, stride, sigma_rad, W, H, d_pred, n_pred, want_dist, d_map,
                        d_stats, d_counts, d_status, stream);
}

int vet_congruency(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, double sigma_rad,
                   int want_nss, double* d_stats, int64_t* d_counts, double* d_rows, int32_t* d_status, void* stream) {
    return launch_congruency(pl, {d_mu, d_mv, nullptr, "vet_congruency_ids"}, U, T, window, stride, sigma_rad, want_nss, d_stats,
                             d_counts, d_rows, d_status, stream);
}

int vet_congruency_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, double sigma_rad, int want_nss,
                       double* d_stats, int64_t* d_counts, double* d_rows, int32_t* d_status, void* stream) {
    return launch_congruency(pl, {nullptr, nullptr, d_ids, nullptr}, U, T, window, stride, sigma_rad, want_nss, d_stats, d_counts,
                             d_rows, d_status, stream);
}

}  // extern "C"
