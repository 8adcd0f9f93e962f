// vet_dispersion.hip — audience dispersion behind vet_dispersion* (include/vet.h): the great-circle angle between the viewing
// directions of two viewers in the same frame, over all pairs, per window and per viewer.  Lattice-independent: only the plan's
// direction table is read.  A viewer u present in frame f has partners: the other present viewers v of the frame whose angle
// a(u, v) (motion_angle's arithmetic, vet_angle.hpp) is not NaN.
// Stage 1, k_dispersion_pairs: workgroup (frame f, chunk of 256 viewers); thread = viewer u.  The frame's samples are quantised
// (sample_dir) and their unit vectors staged in LDS in tiles of up to 1024 viewers (32 B each: x, y, z, id); the thread walks the
// partners v in ASCENDING v — every lane reads the same LDS address, a broadcast — and keeps u's sum, minimum, maximum, partner
// count and same-count in registers.  ALL ORDERED PAIRS are walked: a(u, v) is evaluated from u's side and from v's (the same
// bits: the fused dot is symmetric), twice the acos and no cross-lane step.  It leaves six partials per (frame, viewer) — frame-
// major [T][U] for the pooled layout, viewer-major [U][T] for the per-viewer layout, so that a row is a contiguous slice in both —
// and, where a histogram is wanted, the frame's edge histogram of the ordered pairs (up to 8 bins: per thread the counts of
// a >= e_k in registers, differenced; more bins: a private LDS column per thread, plain increments; then wave_sum and one integer
// atomicAdd per wave and bin).
// Stage 2, k_dispersion_chunk + k_dispersion_finish: a row's W positions (window * U frame-major, or window) are cut into blocks
// of 1024 from the row's start — vet_head_motion's summation rule (thread t adds positions t, t + 256, t + 512, t + 768,
// wave_sum's butterfly, the four waves in order, the blocks ascending) for five FP sums: the partner sums, the nearest-partner
// minima and the three centroid components.  A workgroup takes a chunk of 16 blocks of one row; one wave per row then adds the
// blocks in order and writes the row.  Counts, the maximum (an integer maximum of bit patterns) and the histograms (the window's
// frame histograms added, halved) are exact in any order.  No FP atomics.  Overlapping windows never recompute a frame.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_angle.hpp"

#include <algorithm>
#include <cmath>

namespace vet {

constexpr int DP_THREADS = 256;
constexpr int DP_TILE = 1024;           // viewers per LDS tile (32 KB)
constexpr int DP_BLOCK = 1024;          // positions of one block of the summation rule: four per thread
constexpr int DP_CHUNK_BLOCKS = 16;     // blocks of a row that one workgroup of stage 2 takes
constexpr int DP_MAX_BINS = 64;
constexpr int DP_REG_BINS = 8;          // histograms of up to 8 bins are counted in registers, wider ones in LDS columns
constexpr int DP_EDGE_BYTES = (DP_MAX_BINS + 1 + 1) * 8;      // the edges in front of the LDS columns, 16-byte padded
constexpr int DP_SUMS = 5;              // partner sums, nearest minima, centroid x, y, z

struct DispViewer {                     // one staged viewer of a frame
    double x, y, z;
    int id, pad;
};

// ------------------------------------------------------------------------------------------
// k_dispersion_pairs — stage 1.  blockIdx.x = f * nchunk + chunk; 256 threads, thread = viewer chunk * 256 + tid.
// LDS: DispViewer [1024] static (32 KB); the LDS-column variant with B > 0 adds, dynamic, the edges (528 B) and u32 [B][256],
// the thread's private histogram column.  Without a histogram and with REG_BINS there is no dynamic LDS.
// status[0] counts a sample outside [0, 1] once: by the thread that owns it.
// ------------------------------------------------------------------------------------------
struct DispPairParams {
    SampleSrc src;
    const double* unit;          // [n_dirs][3]
    const double* raw;           // [n_dirs][3]
    int U, T, tile, B, per_user, nchunk;
    double edges[DP_MAX_BINS + 1];
    double* psum;                // per (frame, viewer): the sum of the partners' angles in ascending v
    double* pmin;                // the nearest partner (NaN: no partner)
    double* pmax;                // the farthest partner (NaN: no partner)
    int32_t* pcnt;               // partners
    int32_t* psame;              // partners at angle 0
    int32_t* pid;                // the direction id, -1 absent
    unsigned* fhist;             // [T][B] ordered pairs per bin (zeroed by the host), or null
    int32_t* status;             // [2] or null
};

template <bool FROM_IDS, bool REG_BINS>
__global__ __launch_bounds__(DP_THREADS) void k_dispersion_pairs(const DispPairParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ DispViewer s_tile[DP_TILE];
    double* s_edges = (double*)smem;                             // [B + 1], the LDS-column variant with B > 0 only
    unsigned* col = (unsigned*)(smem + DP_EDGE_BYTES);           // [B][256]
    const int tid = threadIdx.x, lane = lane_id();
    const long f = (long)blockIdx.x / p.nchunk;
    const int chunk = (int)((long)blockIdx.x - f * p.nchunk);
    const int u = chunk * DP_THREADS + tid;
    const int B = p.fhist ? p.B : 0;                             // REG_BINS: 1 <= B <= 8 (the host's choice)
    // REG_BINS: ge[k] counts the partners with a >= e_k in a register (the edges are uniform: scalar operands), bin b is
    // ge[b] - ge[b + 1]; the edges beyond B are +inf and count nothing.  Else the thread's LDS column, one increment per partner.
    unsigned ge[DP_REG_BINS + 1];
    double eg[DP_REG_BINS + 1];
#pragma unroll
    for (int k = 0; k <= DP_REG_BINS; ++k) { ge[k] = 0u; eg[k] = REG_BINS && k <= B ? p.edges[k] : __builtin_inf(); }
    const long base = f * (long)p.U;
    bool bad = false;
    int idu = -1;
    if (u < p.U) idu = sample_dir<FROM_IDS, false>(p.src, base + u, bad);
    double ax = 0.0, ay = 0.0, az = 0.0;
    if (idu >= 0) { const double* A = p.unit + 3L * idu; ax = A[0]; ay = A[1]; az = A[2]; }
    if (!REG_BINS) {
        for (int i = tid; i <= B && B; i += DP_THREADS) s_edges[i] = p.edges[i];
        for (int b = 0; b < B; ++b) col[b * DP_THREADS + tid] = 0u;
    }
    double sum = 0.0, mn = __builtin_inf(), mx = 0.0;
    int cnt = 0, same = 0;
    for (int v0 = 0; v0 < p.U; v0 += p.tile) {
        const int n = min(p.tile, p.U - v0);
        __syncthreads();                                         // the readers of the tile before (and the edges, the columns)
        for (int i = tid; i < n; i += DP_THREADS) {
            bool ignored = false;
            const int id = sample_dir<FROM_IDS, false>(p.src, base + v0 + i, ignored);
            DispViewer w{0.0, 0.0, 0.0, id, 0};
            if (id >= 0) { const double* V = p.unit + 3L * id; w.x = V[0]; w.y = V[1]; w.z = V[2]; }
            s_tile[i] = w;
        }
        __syncthreads();
        if (idu >= 0) {
            for (int j = 0; j < n; ++j) {
                const int idv = __builtin_amdgcn_readfirstlane(s_tile[j].id);    // the same address in every lane
                if (idv < 0) continue;                           // uniform over the wave
                if (v0 + j == u) continue;
                const double a = unit_angle(idu, idv, ax, ay, az, s_tile[j].x, s_tile[j].y, s_tile[j].z, p.raw);
                if (a == a) {
                    sum += a; mn = fmin(mn, a); mx = fmax(mx, a);
                    ++cnt; same += a == 0.0 ? 1 : 0;
                    if (REG_BINS) {
#pragma unroll
                        for (int k = 0; k <= DP_REG_BINS; ++k) ge[k] += a >= eg[k] ? 1u : 0u;
                    } else {
                        const int bin = mo_bin(s_edges, B, a);
                        if (bin >= 0) col[bin * DP_THREADS + tid] += 1u;
                    }
                }
            }
        }
    }
    if (u < p.U) {
        const long at = p.per_user ? (long)u * p.T + f : base + u;
        const double nan = __builtin_nan("");
        p.psum[at] = sum;
        p.pmin[at] = cnt ? mn : nan;
        p.pmax[at] = cnt ? mx : nan;
        p.pcnt[at] = cnt;
        p.psame[at] = same;
        p.pid[at] = idu;
    }
    if (REG_BINS) {
#pragma unroll
        for (int b = 0; b < DP_REG_BINS; ++b) {
            if (b < B) {                                         // uniform
                const int v = wave_sum((int)(ge[b] - ge[b + 1]));
                if (lane == 0 && v) atomicAdd(&p.fhist[f * B + b], (unsigned)v);
            }
        }
    } else {
        for (int b = 0; b < B; ++b) {                            // a thread reads its own column only: no barrier
            const int v = wave_sum((int)col[b * DP_THREADS + tid]);
            if (lane == 0 && v) atomicAdd(&p.fhist[f * B + b], (unsigned)v);
        }
    }
    if (p.status) {
        const unsigned long long anybad = __ballot(bad);
        if (anybad && lane == 0) atomicAdd(&p.status[0], (int)__popcll(anybad));
    }
}

// ------------------------------------------------------------------------------------------
// stage 2
// ------------------------------------------------------------------------------------------
struct DispRows {
    const double* psum;
    const double* pmin;
    const double* pmax;
    const int32_t* pcnt;
    const int32_t* psame;
    const int32_t* pid;
    const unsigned* fhist;       // [T][B] or null
    const double* unit;
    long R, W;                   // rows per viewer (or of the call), positions per row
    int U, T, window, stride, per_user, B;
    long rows;                   // R, or U * R
    double* stats;               // [3][rows] or null
    double* centroid;            // [rows][3] or null
    long long* hist;             // [rows][B] or null
    long long* counts;           // [4][rows] or null
    int32_t* status;             // [2] or null
};

struct DispAcc {                 // a row's integers, zeroed by the host before the pass
    unsigned long long cnt, same, slots, present, maxbits;
};

struct DispChunkParams {
    DispRows g;
    long r0;                     // first row of the pass
    int nblk_row;                // blocks per row
    double* part;                // [rows of the pass][5][nblk_row] block totals
    DispAcc* acc;                // [rows of the pass]
};

__device__ __forceinline__ long dp_row(const DispRows& g, long row) {       // the row's first position in the partial arrays
    if (g.per_user) {
        const long u = row / g.R;
        return u * g.T + (row - u * g.R) * g.stride;
    }
    return row * (long)g.stride * g.U;
}

// k_dispersion_chunk — workgroup (x, y) = chunk x (16 blocks) of row r0 + y: the block totals of the five sums by the rule, the
// integers by wave_sum and one integer atomic per wave.
__global__ __launch_bounds__(DP_THREADS) void k_dispersion_chunk(const DispChunkParams p) {
    __shared__ double s_w[DP_CHUNK_BLOCKS][DP_SUMS][4];
    const DispRows& g = p.g;
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const long y = blockIdx.y, row = p.r0 + y;
    const long q0 = (long)blockIdx.x * (DP_CHUNK_BLOCKS * DP_BLOCK);
    const int m = (int)min((long)(DP_CHUNK_BLOCKS * DP_BLOCK), g.W - q0), nblk = (m + DP_BLOCK - 1) / DP_BLOCK;
    const long at0 = dp_row(g, row) + q0;
    unsigned long long cnt = 0ull, same = 0ull, slots = 0ull, present = 0ull, mx = 0ull;
    for (int b = 0; b < nblk; ++b) {
        double t[DP_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = b * DP_BLOCK + k * DP_THREADS + tid;
            if (q < m) {
                const long at = at0 + q;
                const int id = g.pid[at];
                if (id >= 0) {
                    ++present;
                    const double* V = g.unit + 3L * id;
                    const double x = V[0], yy = V[1], z = V[2];
                    if (x == x && yy == yy && z == z) { t[2] += x; t[3] += yy; t[4] += z; }
                    const int c = g.pcnt[at];
                    if (c > 0) {
                        t[0] += g.psum[at];
                        t[1] += g.pmin[at];
                        ++slots;
                        cnt += (unsigned long long)c;
                        same += (unsigned long long)g.psame[at];
                        mx = max(mx, (unsigned long long)__double_as_longlong(g.pmax[at]));
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < DP_SUMS; ++k) {
            const double s = wave_sum(t[k]);
            if (lane == 0) s_w[b][k][wv] = s;
        }
    }
    cnt = wave_sum(cnt); same = wave_sum(same); slots = wave_sum(slots); present = wave_sum(present);
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned long long)__shfl_xor((long long)mx, o, WAVE));
    DispAcc* acc = p.acc + y;
    if (lane == 0 && present) {
        atomicAdd(&acc->present, present);
        if (slots) {
            atomicAdd(&acc->cnt, cnt); atomicAdd(&acc->same, same); atomicAdd(&acc->slots, slots);
            atomicMax(&acc->maxbits, mx);
        }
    }
    __syncthreads();
    if (tid < nblk * DP_SUMS) {
        const int b = tid / DP_SUMS, k = tid - b * DP_SUMS;
        p.part[(y * DP_SUMS + k) * (long)p.nblk_row + (long)blockIdx.x * DP_CHUNK_BLOCKS + b] = mo_block_total(s_w[b][k]);
    }
}

// k_dispersion_finish — one wave per row, four rows per workgroup: lane k < 5 adds sum k's block totals in ascending order; lane
// b < B adds the histograms of the row's frames; lane 0 writes the row.
__global__ __launch_bounds__(DP_THREADS) void k_dispersion_finish(const DispChunkParams p, const long cr) {
    const DispRows& g = p.g;
    const int lane = lane_id();
    const long y = (long)blockIdx.x * (DP_THREADS / WAVE) + wave_id();
    if (y >= cr) return;                                         // uniform over the wave; no barrier below
    const long row = p.r0 + y;
    double total = 0.0;
    if (lane < DP_SUMS) {
        const double* ps = p.part + (y * DP_SUMS + lane) * (long)p.nblk_row;
        for (int b = 0; b < p.nblk_row; ++b) total += ps[b];
    }
    const double S = __shfl(total, 0, WAVE), M = __shfl(total, 1, WAVE);
    const DispAcc a = p.acc[y];
    if (g.hist && lane < g.B) {                                  // pooled layout only: row = r
        const unsigned* fh = g.fhist + row * (long)g.stride * g.B + lane;
        unsigned long long h = 0ull;
        for (int fi = 0; fi < g.window; ++fi) h += fh[(long)fi * g.B];
        g.hist[row * g.B + lane] = (long long)(h >> 1);          // every pair was counted from both sides
    }
    if (g.centroid && lane >= 2 && lane < DP_SUMS) g.centroid[row * 3 + (lane - 2)] = total;
    if (lane == 0) {
        const bool none = a.cnt == 0ull;
        const double nan = __builtin_nan("");
        if (g.stats) {
            g.stats[row] = none ? nan : S / (double)a.cnt;
            g.stats[g.rows + row] = none ? nan : __longlong_as_double((long long)a.maxbits);
            g.stats[2 * g.rows + row] = none ? nan : M / (double)a.slots;
        }
        if (g.counts) {
            const int sh = g.per_user ? 0 : 1;                   // pooled: a pair sample {u, v} was counted from both sides
            g.counts[row] = (long long)(a.cnt >> sh);
            g.counts[g.rows + row] = (long long)(a.same >> sh);
            g.counts[2 * g.rows + row] = (long long)a.slots;
            g.counts[3 * g.rows + row] = (long long)a.present;
        }
        if (none && g.status) atomicAdd(&g.status[1], 1);
    }
}

}  // namespace vet

namespace vh {

// What vet_dispersion* refuse about their arguments, before anything is staged, allocated or launched.
int check_dispersion_args(const vet_plan* pl, int U, int T, int window, int stride, int per_user, const double* edges, int B) {
    if (!pl) return fail(VET_ERR_INVALID, "plan is NULL");
    if (U <= 0 || T <= 0) return fail(VET_ERR_INVALID, "n_users and n_frames must be positive (got %d, %d)", U, T);
    if (window < 1) return fail(VET_ERR_INVALID, "window must be at least 1 frame (got %d)", window);
    if (stride < 1) return fail(VET_ERR_INVALID, "stride must be at least 1 frame (got %d)", stride);
    if (window > T) return fail(VET_ERR_INVALID, "window of %d frames is longer than the video's %d frames", window, T);
    if (B < 0 || B > vet::DP_MAX_BINS) return fail(VET_ERR_INVALID, "need 0 to %d histogram bins (got %d)", vet::DP_MAX_BINS, B);
    if (B && per_user) return fail(VET_ERR_INVALID, "the per-viewer layout has no histogram (B must be 0, got %d)", B);
    if (B && !edges) return fail(VET_ERR_INVALID, "edges is NULL");
    for (int i = 0; i <= B && B; ++i)
        if (!std::isfinite(edges[i]) || (i && !(edges[i] > edges[i - 1])))
            return fail(VET_ERR_INVALID, "histogram edges must be finite and strictly ascending (edge %d is %g)", i, edges[i]);
    if (U > 65535) return fail(VET_ERR_UNSUPPORTED, "dispersion: %d viewers (at most 65535: a frame's pairs must fit 31 bits)", U);
    const int64_t nchunk = (U + vet::DP_THREADS - 1) / vet::DP_THREADS;
    if ((int64_t)T * nchunk > (int64_t)0x7FFFFFFF)
        return fail(VET_ERR_UNSUPPORTED, "dispersion: %d frames of %d viewers in one call (at most 2^31 - 1 workgroups)", T, U);
    return VET_OK;
}

namespace {

constexpr size_t kDispersionPassBudget = (size_t)256 << 20;   // bytes of per-row workspace a pass of stage 2 may take

int launch_dispersion(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window, int stride,
                      int per_user, const double* edges, int B, double* d_stats, double* d_centroid, int64_t* d_hist,
                      int64_t* d_counts, int32_t* d_status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const long R = (long)vet_window_rows(T, window, stride);
    const long rows = per_user ? R * U : R, W = per_user ? window : (long)window * U;
    if (!d_hist) B = 0;
    if (!B) d_hist = nullptr;
    int tile = vet::DP_TILE;
    if (c->tune.dispersion_tile > 0) tile = std::min(tile, c->tune.dispersion_tile);
    const int nchunk = (U + vet::DP_THREADS - 1) / vet::DP_THREADS;
    const long nblk_row = (W + vet::DP_BLOCK - 1) / vet::DP_BLOCK;
    const long chunks = (nblk_row + vet::DP_CHUNK_BLOCKS - 1) / vet::DP_CHUNK_BLOCKS;
    const size_t per_row = (size_t)nblk_row * vet::DP_SUMS * 8 + sizeof(vet::DispAcc);
    const long CR = std::max(1L, std::min({(long)(kDispersionPassBudget / per_row), rows, 65535L}));
    // workspace: the six partials per (frame, viewer) | the frames' histograms | stage 2's block totals and integers of a pass
    const size_t S = (size_t)T * U;
    WsLayout lay;
    const size_t sum_o = lay.take<double>(S), min_o = lay.take<double>(S), max_o = lay.take<double>(S), cnt_o = lay.take<int32_t>(S),
                 same_o = lay.take<int32_t>(S), id_o = lay.take<int32_t>(S), fh_o = lay.take<uint32_t>((size_t)T * B),
                 part_o = lay.take<double>((size_t)CR * vet::DP_SUMS * nblk_row), acc_o = lay.take<vet::DispAcc>((size_t)CR);
    int rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    {   // stage 1
        vet::DispPairParams q{};
        q.src = vet::SampleSrc{d_mu, d_mv, d_ids, pl->W, pl->H, (long)pl->n_dirs};
        q.unit = pl->d_dir_unit; q.raw = pl->d_dir_raw;
        q.U = U; q.T = T; q.tile = tile; q.B = B; q.per_user = per_user ? 1 : 0; q.nchunk = nchunk;
        for (int i = 0; i <= B && B; ++i) q.edges[i] = edges[i];
        q.psum = (double*)(ws + sum_o); q.pmin = (double*)(ws + min_o); q.pmax = (double*)(ws + max_o);
        q.pcnt = (int32_t*)(ws + cnt_o); q.psame = (int32_t*)(ws + same_o); q.pid = (int32_t*)(ws + id_o);
        q.fhist = B ? (uint32_t*)(ws + fh_o) : nullptr;
        q.status = d_status;
        ProfScope ps(c, s, KID_SPATIAL);
        if (B) HIP_TRY(hipMemsetAsync(q.fhist, 0, (size_t)T * B * 4, s));
        const dim3 grid((unsigned)((long)T * nchunk));
        const bool reg = B >= 1 && B <= vet::DP_REG_BINS;
        const size_t lds = reg || !B ? 0 : vet::DP_EDGE_BYTES + (size_t)B * vet::DP_THREADS * 4;
        auto kernel = d_ids ? (reg ? vet::k_dispersion_pairs<true, true> : vet::k_dispersion_pairs<true, false>)
                            : (reg ? vet::k_dispersion_pairs<false, true> : vet::k_dispersion_pairs<false, false>);
        hipLaunchKernelGGL(kernel, grid, dim3(vet::DP_THREADS), lds, s, q);
        HIP_TRY(hipGetLastError());
    }
    vet::DispChunkParams q{};
    vet::DispRows& g = q.g;
    g.psum = (double*)(ws + sum_o); g.pmin = (double*)(ws + min_o); g.pmax = (double*)(ws + max_o);
    g.pcnt = (int32_t*)(ws + cnt_o); g.psame = (int32_t*)(ws + same_o); g.pid = (int32_t*)(ws + id_o);
    g.fhist = B ? (uint32_t*)(ws + fh_o) : nullptr;
    g.unit = pl->d_dir_unit;
    g.R = R; g.W = W; g.U = U; g.T = T; g.window = window; g.stride = stride; g.per_user = per_user ? 1 : 0; g.B = B; g.rows = rows;
    g.stats = d_stats; g.centroid = d_centroid; g.hist = (long long*)d_hist; g.counts = (long long*)d_counts; g.status = d_status;
    q.nblk_row = (int)nblk_row;
    q.part = (double*)(ws + part_o); q.acc = (vet::DispAcc*)(ws + acc_o);
    ProfScope ps(c, s, KID_TRANSITION);
    for (long r0 = 0; r0 < rows; r0 += CR) {
        const long cr = std::min(CR, rows - r0);
        q.r0 = r0;
        HIP_TRY(hipMemsetAsync(q.acc, 0, (size_t)cr * sizeof(vet::DispAcc), s));
        hipLaunchKernelGGL(vet::k_dispersion_chunk, dim3((unsigned)chunks, (unsigned)cr), dim3(vet::DP_THREADS), 0, s, q);
        HIP_TRY(hipGetLastError());
        const long wgs = (cr + vet::DP_THREADS / vet::WAVE - 1) / (vet::DP_THREADS / vet::WAVE);
        hipLaunchKernelGGL(vet::k_dispersion_finish, dim3((unsigned)wgs), dim3(vet::DP_THREADS), 0, s, q, cr);
        HIP_TRY(hipGetLastError());
    }
    return VET_OK;
}

}  // namespace

int dispersion_set_attrs(vet_ctx*) {
    const int lds = vet::DP_EDGE_BYTES + vet::DP_MAX_BINS * vet::DP_THREADS * 4;
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_dispersion_pairs<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_dispersion_pairs<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return VET_OK;
}

}  // namespace vh

using namespace vh;

extern "C" {

int vet_dispersion(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, int per_user,
                   const double* h_edges, int B, double* d_stats, double* d_centroid, int64_t* d_hist, int64_t* d_counts,
                   int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_dispersion_args(pl, U, T, window, stride, per_user, h_edges, B);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_dispersion_ids", stream, &s);
    return rc ? rc : launch_dispersion(pl, d_mu, d_mv, nullptr, U, T, window, stride, per_user, h_edges, B, d_stats, d_centroid, d_hist,
                                       d_counts, d_status, s);
}

int vet_dispersion_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, int per_user, const double* h_edges,
                       int B, double* d_stats, double* d_centroid, int64_t* d_hist, int64_t* d_counts, int32_t* d_status,
                       void* stream) {
    hipStream_t s;
    int rc = check_dispersion_args(pl, U, T, window, stride, per_user, h_edges, B);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_dispersion(pl, nullptr, nullptr, d_ids, U, T, window, stride, per_user, h_edges, B, d_stats, d_centroid,
                                       d_hist, d_counts, d_status, s);
}

}  // extern "C"
