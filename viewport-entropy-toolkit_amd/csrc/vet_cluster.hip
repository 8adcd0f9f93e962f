// vet_cluster.hip — viewer clusters behind vet_viewer_clusters* (include/vet.h): which viewers look together in a window of frames.
// Lattice-independent: only the plan's direction table is read.  Two present viewers of a frame are NEAR when their directions are
// the same id, the same Vector, or their fused dot (vet_angle.hpp) reaches cos_threshold; a pair of a row is LINKED when it is NEAR
// in at least min_share of the frames both are in; the row's clusters are the connected components of the LINKED graph.
// Stage 0, k_cluster_ids: the samples quantised to direction ids [T][U] once (sample_dir), status[0] raised.
// Stage 1, k_cluster_links: workgroup (row, 256 viewers u, a tile of up to 128 partners v); lane = viewer u, a wave = 64 consecutive u.
// The partners' records (unit vector, id: 32 B) of a chunk of the row's frames are staged in LDS, one record per thread (256: 8
// partners x 32 frames of a long window, or up to 256 / window partners of a short one); the lane walks the frames with the (co,
// near) counts of 8 partners in registers — every lane reads the same LDS address, a broadcast — decides LINKED, and one __ballot of
// the wave is the word links[v][u / 64], stored by lane 0.  ALL ORDERED PAIRS are walked: LINKED(u, v) is decided from u's side and
// from v's (the same bits: the fused dot is symmetric, the counts are integers); walking the upper triangle and mirroring the word
// through a transpose was NOT built and the two were not measured against each other.  No atomics, no scratch, 8 KB of LDS, no acos.
// Stage 2, k_cluster_components: one workgroup per row, the labels [U] in LDS (see the kernel's comment for why the result does not
// depend on scheduling), then the dense labels, sizes, counts, the streams per fraction, the partition entropy by the summation rule
// of vet_head_motion (wave_sum, mo_block_total), and the centroids where asked for.
// Rows run in passes under a 256 MB budget of link words.  No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_angle.hpp"
#include "vet_rank.hpp"

#include <algorithm>
#include <cmath>

namespace vet {

constexpr int CL_THREADS = 256;
constexpr int CL_GROUP = 8;             // partners whose counts a lane keeps in registers at a time
constexpr int CL_STAGE = 256;           // staged partner records: one per thread (8 KB)
constexpr int CL_FRAMES = 32;           // frames per chunk of a window longer than that
constexpr int CL_TILE = 128;            // partners of one workgroup, at most (fewer where a pass has few rows)
constexpr int CL_AHEAD = 4;             // frames whose own id and unit vector a lane loads together
constexpr int CL_BLOCK = 1024;          // positions of one block of the summation rule: four per thread
constexpr int CL_MAX_USERS = 8192;      // the labels, ranks and dense labels of a row live in LDS (96 KB)
constexpr int CL_MAX_Q = 16;
constexpr int CL_ABSENT = 0x7FFFFFFF;   // the label of a viewer who is not in the row
constexpr int CL_LABEL_BITS = 13;       // a sort record is (U - size) << 13 | label: both below 8192

struct ClusterViewer {                  // one staged partner of a frame
    double x, y, z;
    int id, pad;
};

// ------------------------------------------------------------------------------------------
// k_cluster_ids — stage 0: direction ids [T][U], -1 absent or out of range; status[0] counts the latter.
// ------------------------------------------------------------------------------------------
template <bool FROM_IDS>
__global__ __launch_bounds__(CL_THREADS) void k_cluster_ids(const SampleSrc src, const long n, int32_t* ids, int32_t* status) {
    const long step = (long)gridDim.x * CL_THREADS;
    int nbad = 0;
    for (long i = (long)blockIdx.x * CL_THREADS + threadIdx.x; i < n; i += step) {
        bool bad = false;
        ids[i] = sample_dir<FROM_IDS, false>(src, i, bad);
        nbad += bad ? 1 : 0;
    }
    if (status) {
        nbad = wave_sum(nbad);
        if (lane_id() == 0 && nbad) atomicAdd(&status[0], nbad);
    }
}

// ------------------------------------------------------------------------------------------
// k_cluster_links — stage 1.  blockIdx.x = tile * nub + ub, blockIdx.y = row of the pass; thread = viewer ub * 256 + tid.
// LDS: ClusterViewer [256] static (8 KB).  Tail lanes (u >= U) and absent viewers vote 0; the diagonal is 0.
// ------------------------------------------------------------------------------------------
struct ClusterLinkParams {
    const int32_t* ids;          // [T][U]
    const double* unit;          // [n_dirs][3]
    const double* raw;           // [n_dirs][3]
    int U, words, window, stride, tile, nub;
    long r0;                     // first row of the pass
    double cos_thr, min_share;
    unsigned long long* links;   // [rows of the pass][U][words]
};

__global__ __launch_bounds__(CL_THREADS) void k_cluster_links(const ClusterLinkParams p) {
    __shared__ ClusterViewer s_rec[CL_STAGE];
    const int tid = threadIdx.x, lane = lane_id();
    const int vt = (int)blockIdx.x / p.nub, ub = (int)blockIdx.x - vt * p.nub;
    const int u = ub * CL_THREADS + tid;
    const long f_row = (p.r0 + blockIdx.y) * (long)p.stride;
    const int v_begin = vt * p.tile, v_end = min(p.U, v_begin + p.tile);
    // a short window is staged whole, for as many partners as 256 records hold; a long one in chunks of 32 frames for 8 partners
    const bool single = p.window <= CL_FRAMES;
    const int FC = single ? p.window : CL_FRAMES;
    const int nv = single ? max(CL_GROUP, (CL_STAGE / FC) & ~(CL_GROUP - 1)) : CL_GROUP;
    unsigned long long* out = p.links + (long)blockIdx.y * p.U * p.words;
    const int word = u >> 6;                                     // the same in the 64 lanes of a wave
    int co[CL_GROUP], nr[CL_GROUP];
    auto zero = [&]() {
#pragma unroll
        for (int k = 0; k < CL_GROUP; ++k) { co[k] = 0; nr[k] = 0; }
    };
    auto vote = [&](int vbase) {
#pragma unroll
        for (int k = 0; k < CL_GROUP; ++k) {
            const int v = vbase + k;
            const bool linked = u < p.U && v != u && co[k] >= 1 && (double)nr[k] >= p.min_share * (double)co[k];
            const unsigned long long w = __ballot(linked);
            if (lane == 0 && v < v_end && word < p.words) out[(long)v * p.words + word] = w;
        }
    };
    for (int v0 = v_begin; v0 < v_end; v0 += nv) {
        zero();
        for (int f0 = 0; f0 < p.window; f0 += FC) {
            const int nf = min(FC, p.window - f0);
            __syncthreads();                                     // the readers of the records before
            {
                const int fi = tid / nv, j = tid - fi * nv;
                if (fi < nf) {
                    const int v = v0 + j;
                    ClusterViewer w{0.0, 0.0, 0.0, -1, 0};
                    if (v < v_end) w.id = p.ids[(f_row + f0 + fi) * p.U + v];
                    if (w.id >= 0) { const double* V = p.unit + 3L * w.id; w.x = V[0]; w.y = V[1]; w.z = V[2]; }
                    s_rec[fi * nv + j] = w;
                }
            }
            __syncthreads();
            for (int g = 0; g < nv && v0 + g < v_end; g += CL_GROUP) {
                if (single) zero();
                for (int fi0 = 0; fi0 < nf; fi0 += CL_AHEAD) {   // four frames' own loads in flight together
                    int idu[CL_AHEAD];
                    double ax[CL_AHEAD], ay[CL_AHEAD], az[CL_AHEAD];
#pragma unroll
                    for (int j = 0; j < CL_AHEAD; ++j)
                        idu[j] = u < p.U && fi0 + j < nf ? p.ids[(f_row + f0 + fi0 + j) * p.U + u] : -1;
#pragma unroll
                    for (int j = 0; j < CL_AHEAD; ++j) {
                        const double* A = p.unit + 3L * max(idu[j], 0);
                        ax[j] = A[0]; ay[j] = A[1]; az[j] = A[2];
                    }
#pragma unroll
                    for (int j = 0; j < CL_AHEAD; ++j) {
                        if (idu[j] < 0) continue;
                        const ClusterViewer* b = s_rec + (fi0 + j) * nv + g;
#pragma unroll
                        for (int k = 0; k < CL_GROUP; ++k) {
                            const int idv = __builtin_amdgcn_readfirstlane(b[k].id);     // the same address in every lane
                            if (idv < 0) continue;               // uniform over the wave
                            ++co[k];
                            nr[k] += unit_near(idu[j], idv, ax[j], ay[j], az[j], b[k].x, b[k].y, b[k].z, p.cos_thr, p.raw) ? 1 : 0;
                        }
                    }
                }
                if (single) vote(v0 + g);
            }
        }
        if (!single) vote(v0);
    }
}

// ------------------------------------------------------------------------------------------
// k_cluster_components — stage 2.  One 256-thread workgroup per row; dynamic LDS: three i32 arrays of P2 >= U entries (a power of
// two): lab (the labels, later the sizes), rk (the roots' ranks, later the sort records), dn (the dense labels).
//
// The fixpoint.  lab[u] starts as u for a viewer of the row.  A sweep lowers lab[u] to the smallest label among u and its LINKED
// neighbours, then shortens it by one pointer jump, lab[u] = lab[lab[u]]; only the thread that owns u ever writes lab[u], and it
// reads the other labels while their owners may be writing them.  That is harmless: a label is always the index of a member of u's
// own component (it starts as one, and every value it can take is a label of a neighbour or of a member), a 32-bit LDS word is read
// and written whole, and labels only ever decrease, so a reader sees some earlier or later value of a decreasing sequence of members.
// The sweeps stop when one changes nothing.  Then lab[u] <= lab[v] for every linked pair from both sides, so the labels are equal
// across every link and hence over a component, and the component's smallest member m has lab[m] = m because no member is smaller.
// The fixpoint is therefore the component's smallest member whatever order the lanes read each other's labels in: the result does
// not depend on scheduling although the number of sweeps does, and there is no fixed iteration order to preserve.
// ------------------------------------------------------------------------------------------
struct ClusterRowParams {
    const int32_t* ids;          // [T][U]
    const double* unit;
    const unsigned long long* links;     // [rows of the pass][U][words]
    int U, words, window, stride, Q, P2;
    long r0, R;
    double fractions[CL_MAX_Q];
    int32_t* labels;             // [R][U] or null
    int32_t* sizes;              // [R][U] or null
    long long* counts;           // [5][R] or null
    int32_t* top;                // [R][Q] or null
    double* stats;               // [3][R] or null
    double* centroids;           // [R][U][3] or null
    int32_t* status;             // [2] or null
    unsigned long long* sweeps;  // [2]: the most sweeps a row took, and their sum over the rows
};

// the sum of v over the 256 threads, in every thread; s4 is LDS [4].  Every thread calls it.
__device__ __forceinline__ unsigned long long cl_block_sum(unsigned long long v, unsigned long long* s4) {
    v = wave_sum(v);
    __syncthreads();                                             // the readers of s4 before
    if (lane_id() == 0) s4[wave_id()] = v;
    __syncthreads();
    return s4[0] + s4[1] + s4[2] + s4[3];
}

__global__ __launch_bounds__(CL_THREADS) void k_cluster_components(const ClusterRowParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double s_w[4];
    __shared__ unsigned long long s_sum[4];
    int* lab = (int*)smem;
    int* rk = lab + p.P2;
    int* dn = rk + p.P2;
    volatile int* vl = lab;
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int U = p.U, words = p.words;
    const long row = p.r0 + blockIdx.x, f_row = row * (long)p.stride;
    const unsigned long long* L = p.links + (long)blockIdx.x * U * words;

    unsigned long long mine = 0ull, bits_set = 0ull;             // this thread's viewers of the row, the set bits of their words
    for (int u = tid; u < U; u += CL_THREADS) {
        bool present = false;
        for (int fi = 0; fi < p.window && !present; ++fi) present = p.ids[(f_row + fi) * U + u] >= 0;
        lab[u] = present ? u : CL_ABSENT;
        mine += present ? 1ull : 0ull;
        for (int w = 0; w < words; ++w) bits_set += (unsigned long long)__popcll(L[(long)u * words + w]);
    }
    const int P = (int)cl_block_sum(mine, s_sum);                // (a barrier: lab is complete)
    const unsigned long long n_links = cl_block_sum(bits_set, s_sum) >> 1;

    unsigned sweeps = 0u;
    for (;;) {
        int changed = 0;
        for (int u = tid; u < U; u += CL_THREADS) {
            const int cur = vl[u];
            if (cur == CL_ABSENT) continue;
            int m = cur;
            for (int w = 0; w < words; ++w) {
                unsigned long long bits = L[(long)u * words + w];
                while (bits) {
                    const int v = w * 64 + __ffsll((long long)bits) - 1;
                    bits &= bits - 1ull;
                    m = min(m, vl[v]);
                }
            }
            if (m < cur) { vl[u] = m; changed = 1; }
        }
        __syncthreads();
        for (int u = tid; u < U; u += CL_THREADS) {
            const int cur = vl[u];
            if (cur == CL_ABSENT) continue;
            const int up = vl[cur];
            if (up < cur) { vl[u] = up; changed = 1; }
        }
        ++sweeps;
        if (!__syncthreads_or(changed)) break;
    }

    // the roots ranked in ascending order: the dense labels
    int K = 0;
    for (int u0 = 0; u0 < U; u0 += CL_THREADS) {
        const int u = u0 + tid;
        const bool root = u < U && lab[u] == u;
        const unsigned long long m = __ballot(root);
        const unsigned long long tot = cl_block_sum(lane == 0 ? (unsigned long long)__popcll(m) : 0ull, s_sum);
        int off = 0;
        for (int w = 0; w < wv; ++w) off += (int)s_sum[w];
        if (root) rk[u] = K + off + below(m);
        K += (int)tot;
    }
    __syncthreads();
    for (int u = tid; u < U; u += CL_THREADS) dn[u] = lab[u] == CL_ABSENT ? -1 : rk[lab[u]];
    __syncthreads();
    for (int i = tid; i < p.P2; i += CL_THREADS) lab[i] = 0;    // from here lab holds the sizes
    __syncthreads();
    for (int u = tid; u < U; u += CL_THREADS)
        if (dn[u] >= 0) atomicAdd(&lab[dn[u]], 1);
    __syncthreads();
    for (int u = tid; u < U; u += CL_THREADS) {
        if (p.labels) p.labels[row * U + u] = dn[u];
        if (p.sizes) p.sizes[row * U + u] = lab[u];
    }

    // the (size descending, label ascending) records, sorted
    unsigned* rec = (unsigned*)rk;
    unsigned long long ones = 0ull;
    for (int i = tid; i < p.P2; i += CL_THREADS) {
        rec[i] = i < K ? ((unsigned)(U - lab[i]) << CL_LABEL_BITS) | (unsigned)i : 0xFFFFFFFFu;
        ones += i < K && lab[i] == 1 ? 1ull : 0ull;
    }
    const unsigned long long singletons = cl_block_sum(ones, s_sum);
    lds_bitonic_sort(rec, p.P2);
    const int largest = K ? U - (int)(rec[0] >> CL_LABEL_BITS) : 0;
    if (p.top && tid < p.Q) {
        int n = 0;
        if (P > 0) {
            const double need = p.fractions[tid] * (double)P;
            long s = 0;
            while (n < K) {
                s += U - (int)(rec[n] >> CL_LABEL_BITS);
                ++n;
                if ((double)s >= need) break;
            }
        }
        p.top[row * p.Q + tid] = n;
    }

    // sum_k s_k log2 s_k by the summation rule, the labels as the positions
    double S = 0.0;
    for (int b0 = 0; b0 < K; b0 += CL_BLOCK) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = b0 + j * CL_THREADS + tid;
            if (k < K) { const double s = (double)lab[k]; t += s * log2(s); }
        }
        const double ws = wave_sum(t);
        if (lane == 0) s_w[wv] = ws;
        __syncthreads();
        S += mo_block_total(s_w);
        __syncthreads();
    }
    if (tid == 0) {
        const double nan = __builtin_nan("");
        if (p.counts) {
            p.counts[row] = P;
            p.counts[p.R + row] = K;
            p.counts[2 * p.R + row] = largest;
            p.counts[3 * p.R + row] = (long long)singletons;
            p.counts[4 * p.R + row] = (long long)n_links;
        }
        if (p.stats) {
            const double lp = log2((double)P);
            const double Hp = P > 0 ? lp - S / (double)P : nan;
            p.stats[row] = Hp;
            p.stats[p.R + row] = P > 1 ? Hp / lp : nan;
            p.stats[2 * p.R + row] = P > 0 ? (double)largest / (double)P : nan;
        }
        if (P == 0 && p.status) atomicAdd(&p.status[1], 1);
        atomicMax(&p.sweeps[0], (unsigned long long)sweeps);
        atomicAdd(&p.sweeps[1], (unsigned long long)sweeps);
    }
    if (p.centroids) {                                           // thread = cluster k: its members' samples, frame-major, viewer ascending
        for (int k = tid; k < U; k += CL_THREADS) {
            double cx = 0.0, cy = 0.0, cz = 0.0;
            if (k < K) {
                for (int fi = 0; fi < p.window; ++fi) {
                    const int32_t* fr = p.ids + (f_row + fi) * U;
                    for (int u = 0; u < U; ++u) {
                        if (dn[u] != k) continue;
                        const int id = fr[u];
                        if (id < 0) continue;
                        const double* V = p.unit + 3L * id;
                        const double x = V[0], yy = V[1], z = V[2];
                        if (x == x && yy == yy && z == z) { cx += x; cy += yy; cz += z; }
                    }
                }
            }
            double* c = p.centroids + (row * U + k) * 3;
            c[0] = cx; c[1] = cy; c[2] = cz;
        }
    }
}

}  // namespace vet

namespace vh {

// What vet_viewer_clusters* refuse about their arguments, before anything is staged, allocated or launched.
int check_cluster_args(const vet_plan* pl, int U, int T, int window, int stride, double cos_threshold, double min_share,
                       const double* fractions, int Q) {
    if (!pl) return fail(VET_ERR_INVALID, "plan is NULL");
    if (U <= 0 || T <= 0) return fail(VET_ERR_INVALID, "n_users and n_frames must be positive (got %d, %d)", U, T);
    if (window < 1) return fail(VET_ERR_INVALID, "window must be at least 1 frame (got %d)", window);
    if (stride < 1) return fail(VET_ERR_INVALID, "stride must be at least 1 frame (got %d)", stride);
    if (window > T) return fail(VET_ERR_INVALID, "window of %d frames is longer than the video's %d frames", window, T);
    if (Q < 0 || Q > vet::CL_MAX_Q) return fail(VET_ERR_INVALID, "need 0 to %d fractions (got %d)", vet::CL_MAX_Q, Q);
    if (Q && !fractions) return fail(VET_ERR_INVALID, "fractions is NULL");
    for (int i = 0; i < Q; ++i)
        if (!(fractions[i] > 0.0 && fractions[i] <= 1.0))
            return fail(VET_ERR_INVALID, "fractions must lie in (0, 1] (fraction %d is %g)", i, fractions[i]);
    if (!(min_share > 0.0 && min_share <= 1.0)) return fail(VET_ERR_INVALID, "min_share must lie in (0, 1] (got %g)", min_share);
    if (!(cos_threshold >= -1.0 && cos_threshold <= 1.0))
        return fail(VET_ERR_INVALID, "cos_threshold must lie in [-1, 1] (got %g)", cos_threshold);
    if (U > vet::CL_MAX_USERS)
        return fail(VET_ERR_UNSUPPORTED, "viewer clusters: %d viewers (at most %d: the labels of a row live in LDS)", U, vet::CL_MAX_USERS);
    const int64_t nchunk = (U + vet::CL_THREADS - 1) / vet::CL_THREADS;
    if ((int64_t)T * nchunk > (int64_t)0x7FFFFFFF)
        return fail(VET_ERR_UNSUPPORTED, "viewer clusters: %d frames of %d viewers in one call (at most 2^31 - 1 workgroups)", T, U);
    return VET_OK;
}

namespace {

constexpr size_t kClusterPassBudget = (size_t)256 << 20;      // bytes of link words a pass may take
constexpr int kSweepSlot = 12;                                // vet_ctx::pool: the sweep counts of the last call (16 B)

int launch_clusters(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window, int stride,
                    double cos_threshold, double min_share, const double* fractions, int Q, int32_t* d_labels, int32_t* d_sizes,
                    int64_t* d_counts, int32_t* d_top, double* d_stats, double* d_centroids, uint64_t* d_links, int32_t* d_status,
                    hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const long R = (long)vet_window_rows(T, window, stride);
    const int words = (U + 63) / 64;
    const size_t per_row = (size_t)U * words * 8;
    long CR = std::max(1L, std::min({(long)(kClusterPassBudget / per_row), R, 65535L}));
    if (c->tune.cluster_rows > 0) CR = std::min(CR, (long)c->tune.cluster_rows);
    // partners per workgroup: 128, or as few (a multiple of 8) as gives a pass of few rows some eight workgroups per CU
    const long nub_ = (U + vet::CL_THREADS - 1) / vet::CL_THREADS, target = 8L * c->n_cu;
    int tile = (int)std::min<long>(vet::CL_TILE, std::max<long>(vet::CL_GROUP, (U * nub_ * CR / target + 7) / 8 * 8));
    if (c->tune.cluster_tile > 0) tile = std::min(tile, c->tune.cluster_tile);
    int P2 = 64;
    while (P2 < U) P2 <<= 1;
    // workspace: the direction ids | the link words of a pass (where d_links does not take them)
    WsLayout lay;
    const size_t id_o = lay.take<int32_t>((size_t)T * U), link_o = lay.take<uint64_t>(d_links ? 0 : (size_t)CR * U * words);
    int rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    void* sweeps = nullptr;
    rc = pooled(c, kSweepSlot, 16, &sweeps);
    if (rc) return rc;
    int32_t* ids = (int32_t*)(ws + id_o);
    {   // stage 0
        ProfScope ps(c, s, KID_SPATIAL);
        HIP_TRY(hipMemsetAsync(sweeps, 0, 16, s));
        const vet::SampleSrc src{d_mu, d_mv, d_ids, pl->W, pl->H, (long)pl->n_dirs};
        const long n = (long)T * U;
        const dim3 grid((unsigned)grid_for(n, vet::CL_THREADS, c->n_cu));
        if (d_ids) hipLaunchKernelGGL(vet::k_cluster_ids<true>, grid, dim3(vet::CL_THREADS), 0, s, src, n, ids, d_status);
        else hipLaunchKernelGGL(vet::k_cluster_ids<false>, grid, dim3(vet::CL_THREADS), 0, s, src, n, ids, d_status);
        HIP_TRY(hipGetLastError());
    }
    vet::ClusterLinkParams q{};
    q.ids = ids; q.unit = pl->d_dir_unit; q.raw = pl->d_dir_raw;
    q.U = U; q.words = words; q.window = window; q.stride = stride; q.tile = tile; q.nub = (U + vet::CL_THREADS - 1) / vet::CL_THREADS;
    q.cos_thr = cos_threshold; q.min_share = min_share;
    const int ntile = (U + tile - 1) / tile;
    vet::ClusterRowParams g{};
    g.ids = ids; g.unit = pl->d_dir_unit;
    g.U = U; g.words = words; g.window = window; g.stride = stride; g.Q = d_top ? Q : 0; g.P2 = P2; g.R = R;
    for (int i = 0; i < g.Q; ++i) g.fractions[i] = fractions[i];
    g.labels = d_labels; g.sizes = d_sizes; g.counts = (long long*)d_counts; g.top = g.Q ? d_top : nullptr; g.stats = d_stats;
    g.centroids = d_centroids; g.status = d_status; g.sweeps = (unsigned long long*)sweeps;
    for (long r0 = 0; r0 < R; r0 += CR) {
        const long cr = std::min(CR, R - r0);
        unsigned long long* links = d_links ? (unsigned long long*)d_links + (size_t)r0 * U * words : (unsigned long long*)(ws + link_o);
        q.r0 = g.r0 = r0; q.links = links; g.links = links;
        {
            ProfScope ps(c, s, KID_TRANSITION);
            hipLaunchKernelGGL(vet::k_cluster_links, dim3((unsigned)(q.nub * ntile), (unsigned)cr), dim3(vet::CL_THREADS), 0, s, q);
            HIP_TRY(hipGetLastError());
        }
        ProfScope ps(c, s, KID_FINALIZE);
        hipLaunchKernelGGL(vet::k_cluster_components, dim3((unsigned)cr), dim3(vet::CL_THREADS), (size_t)3 * P2 * 4, s, g);
        HIP_TRY(hipGetLastError());
    }
    return VET_OK;
}

}  // namespace

int cluster_set_attrs(vet_ctx*) {
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_cluster_components, hipFuncAttributeMaxDynamicSharedMemorySize,
                                3 * vet::CL_MAX_USERS * 4));
    return VET_OK;
}

}  // namespace vh

using namespace vh;

extern "C" {

int vet_viewer_clusters(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, double cos_threshold,
                        double min_share, const double* h_fractions, int Q, int32_t* d_labels, int32_t* d_sizes, int64_t* d_counts,
                        int32_t* d_top, double* d_stats, double* d_centroids, uint64_t* d_links, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_cluster_args(pl, U, T, window, stride, cos_threshold, min_share, h_fractions, Q);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_viewer_clusters_ids", stream, &s);
    return rc ? rc : launch_clusters(pl, d_mu, d_mv, nullptr, U, T, window, stride, cos_threshold, min_share, h_fractions, Q, d_labels,
                                     d_sizes, d_counts, d_top, d_stats, d_centroids, d_links, d_status, s);
}

int vet_viewer_clusters_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, double cos_threshold,
                            double min_share, const double* h_fractions, int Q, int32_t* d_labels, int32_t* d_sizes, int64_t* d_counts,
                            int32_t* d_top, double* d_stats, double* d_centroids, uint64_t* d_links, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_cluster_args(pl, U, T, window, stride, cos_threshold, min_share, h_fractions, Q);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_clusters(pl, nullptr, nullptr, d_ids, U, T, window, stride, cos_threshold, min_share, h_fractions, Q,
                                     d_labels, d_sizes, d_counts, d_top, d_stats, d_centroids, d_links, d_status, s);
}

int vet_viewer_clusters_sweeps(vet_plan* pl, int64_t* h_sweeps) {
    if (!pl || !h_sweeps) return fail(VET_ERR_INVALID, "plan or h_sweeps is NULL");
    vet_ctx* c = pl->ctx;
    h_sweeps[0] = h_sweeps[1] = 0;
    if (!c->pool[kSweepSlot]) return VET_OK;                     // no call yet
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h_sweeps, c->pool[kSweepSlot], 16, hipMemcpyDeviceToHost));
    return VET_OK;
}

}  // extern "C"
