// vet_fixation.hip — fixation and tile-dwell events behind vet_fixations* (include/vet.h): the kernels and their launch logic.  The
// pair (f, f + 1) of a viewer HOLDS when the viewer is present in both frames and the two directions are within a cone (mode 0:
// unit_near of vet_angle.hpp, the clusters' NEAR rule) or have the same nearest tile of lattice 0 (mode 1); a RUN is a maximal
// interval of present frames whose pairs all hold, an EVENT a run of at least min_frames frames; it belongs to the row of its START.
// Everything is an integer but the centroids.  The one unit that walks a viewer's frames in order with state carried along:
//   k_user_dirs (vet_user.hip)  dirs [U][T], for both layouts
//   k_fix_runs<MODE>    one 256-thread workgroup per viewer, persistent over the viewers, the frames in chunks of 1024 (four
//                       consecutive frames per thread).  The start of a frame's run is an inclusive max-scan of "f where a run starts
//                       at f": in the thread, across the lanes by shuffles, across the four waves through LDS words, the carry into
//                       the next chunk in a register — a run may span any number of chunks.  The thread that holds a run's END writes
//                       L to len[u][start]; the owner of every other frame writes 0.  The viewer's events are counted.
//   k_fix_offsets       one workgroup: the exclusive prefix of the viewers' event counts
//   k_fix_labels<MODE>  the same walk, scan and carry: label = len[u][start] >= min_frames ? len[u][start] : 0, -1 absent; with the
//                       event list, a second (sum) scan of the qualifying starts gives an event's rank inside its viewer
//   k_fix_frames        pooled layout: workgroup = 256 frames x 64 viewers, lane = frame (coalesced); the frame's totals by integer
//                       atomics, the histogram of a row by integer atomics for the rows that contain the event's start
//   k_fix_rows<POOLED, G>   a wave (G = 64) or a workgroup (G = 256) per row sums the row's frames: the labels and lengths of the
//                       viewer (per-viewer layout; its histogram in LDS) or the frame totals (pooled)
//   k_fix_centroids     one thread per listed event: the unit vectors of its frames in ascending order, plain adds
// Integer atomics only; no FP atomics.  No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_angle.hpp"

#include <algorithm>
#include <cmath>

namespace vet {

constexpr int FX_THREADS = 256;
constexpr int FX_FPT = 4;                       // consecutive frames of one thread
constexpr int FX_CHUNK = FX_THREADS * FX_FPT;   // frames of a chunk of the walk
constexpr int FX_WAVES = FX_THREADS / WAVE;
constexpr int FX_MAX_BINS = 64;
constexpr int FX_TILE_USERS = 64;               // k_fix_frames: viewers of one workgroup

struct FixWalk {
    const int32_t* dirs;         // [U][T]
    const double* unit;          // [n_dirs][3]
    const double* raw;           // [n_dirs][3]
    const uint16_t* nearest;     // [n_dirs], lattice 0 (mode 1)
    int n;                       // tiles of lattice 0
    double cos_thr;
    int U, T, chunk, min_frames;
    int32_t* len;                // [U][T]: L at the start of a run, 0 elsewhere
    int32_t* evcount;            // [U]
    int32_t* labels;             // [U][T]
    const long long* offsets;    // [U + 1]
    int32_t* events;             // [max_events][4] or null
    long long max_events;
};

template <int MODE>
__device__ __forceinline__ bool fx_hold(const FixWalk& p, int ia, int ib) {
    if (ia < 0 || ib < 0) return false;
    if (MODE == 1) {
        const int ta = (int)p.nearest[ia], tb = (int)p.nearest[ib];
        return ta == tb && ta < p.n;
    }
    if (ia == ib) return true;
    const double* A = p.unit + 3L * ia;
    const double* B = p.unit + 3L * ib;
    return unit_near(ia, ib, A[0], A[1], A[2], B[0], B[1], B[2], p.cos_thr, p.raw);
}

__device__ __forceinline__ int fx_wave_max(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, WAVE));
    return v;
}

// The thread's part of a chunk: frames f0 .. f0 + 3 (f0 = c0 + 4 tid; none for a thread beyond the chunk), whether a run starts
// (bit k of `starts`) or ends (`ends`) at frame f0 + k, and whether the viewer is present (`here`).  d = the viewer's ids.
template <int MODE>
__device__ __forceinline__ void fx_flags(const FixWalk& p, const int32_t* d, long f0, bool mine, unsigned& here, unsigned& starts,
                                         unsigned& ends) {
    here = starts = ends = 0u;
    if (!mine) return;
    int id[FX_FPT + 2];
#pragma unroll
    for (int k = 0; k < FX_FPT + 2; ++k) {
        const long f = f0 - 1 + k;
        id[k] = f >= 0 && f < p.T ? d[f] : -1;
    }
    bool h[FX_FPT + 1];
#pragma unroll
    for (int k = 0; k <= FX_FPT; ++k) h[k] = fx_hold<MODE>(p, id[k], id[k + 1]);
#pragma unroll
    for (int k = 0; k < FX_FPT; ++k)
        if (id[k + 1] >= 0) {
            here |= 1u << k;
            if (!h[k]) starts |= 1u << k;
            if (!h[k + 1]) ends |= 1u << k;
        }
}

// The start of the run of each of the thread's frames: s[k] for frame f0 + k (meaningful where the viewer is present).  An inclusive
// max-scan of the starts over the chunk on top of `carry`, the last start before the chunk (-1: none), which is advanced to the
// chunk's end.  s_w = 4 LDS words of this chunk's parity; the caller's barrier per chunk separates their reuse.
__device__ __forceinline__ void fx_scan_starts(unsigned starts, long f0, int* s_w, int& carry, int s[FX_FPT]) {
    const int lane = lane_id(), wv = wave_id();
    int cur = -1;
#pragma unroll
    for (int k = 0; k < FX_FPT; ++k) {
        if (starts >> k & 1u) cur = (int)(f0 + k);
        s[k] = cur;
    }
    int v = cur;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int t = __shfl_up(v, o, WAVE);
        if (lane >= o) v = max(v, t);
    }
    int before = __shfl_up(v, 1, WAVE);
    if (lane == 0) before = -1;
    if (lane == WAVE - 1) s_w[wv] = v;
    __syncthreads();
    int total = carry;
    before = max(before, carry);
#pragma unroll
    for (int w = 0; w < FX_WAVES; ++w) {
        const int t = s_w[w];
        if (w < wv) before = max(before, t);
        total = max(total, t);
    }
    carry = total;
#pragma unroll
    for (int k = 0; k < FX_FPT; ++k) s[k] = max(s[k], before);
}

// ------------------------------------------------------------------------------------------
// k_fix_runs — the lengths of the runs.  LDS: 2 x 4 scan words, 4 count words.
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(FX_THREADS) void k_fix_runs(const FixWalk p) {
    __shared__ int s_w[2][FX_WAVES];
    __shared__ int s_n[FX_WAVES];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const bool mine = tid * FX_FPT < p.chunk;
    int par = 0;                                                 // alternates with every chunk, across the viewers too
    for (int u = blockIdx.x; u < p.U; u += gridDim.x) {
        const int32_t* d = p.dirs + (long)u * p.T;
        int32_t* len = p.len + (long)u * p.T;
        int carry = -1, nev = 0;
        for (long c0 = 0; c0 < p.T; c0 += p.chunk, par ^= 1) {
            const long f0 = c0 + (long)tid * FX_FPT;
            unsigned here, starts, ends;
            fx_flags<MODE>(p, d, f0, mine, here, starts, ends);
            int s[FX_FPT];
            fx_scan_starts(starts, f0, s_w[par], carry, s);
#pragma unroll
            for (int k = 0; k < FX_FPT; ++k) {
                const long f = f0 + k;
                if (!mine || f >= p.T) continue;
                if (!(starts >> k & 1u)) len[f] = 0;             // a start's slot belongs to the thread that holds the run's end
                if (ends >> k & 1u) {
                    const int st = max(s[k], 0);                     // a present frame has a start at or before it
                    const int L = (int)(f - st) + 1;
                    len[st] = L;
                    nev += L >= p.min_frames ? 1 : 0;
                }
            }
        }
        nev = wave_sum(nev);
        __syncthreads();
        if (lane == 0) s_n[wv] = nev;
        __syncthreads();
        if (tid == 0) p.evcount[u] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    }
}

// ------------------------------------------------------------------------------------------
// k_fix_offsets — offsets [U + 1] = the exclusive prefix of evcount, into the workspace copy and the caller's array.  One workgroup.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FX_THREADS) void k_fix_offsets(const int32_t* evcount, const int U, long long* ws_off, long long* out) {
    __shared__ long long s_w[FX_WAVES];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    long long carry = 0;
    for (int u0 = 0; u0 < U; u0 += FX_THREADS) {
        const int u = u0 + tid;
        const long long mine = u < U ? (long long)evcount[u] : 0;
        long long v = mine;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const long long t = __shfl_up(v, o, WAVE);
            if (lane >= o) v += t;
        }
        __syncthreads();
        if (lane == WAVE - 1) s_w[wv] = v;
        __syncthreads();
        long long before = carry, total = carry;
        for (int w = 0; w < FX_WAVES; ++w) {
            if (w < wv) before += s_w[w];
            total += s_w[w];
        }
        if (u < U) {
            const long long o = before + v - mine;
            ws_off[u] = o;
            if (out) out[u] = o;
        }
        carry = total;
    }
    if (tid == 0) {
        ws_off[U] = carry;
        if (out) out[U] = carry;
    }
}

// ------------------------------------------------------------------------------------------
// k_fix_labels — the label of every sample, and the event list.  LDS: 2 x 4 scan words, 2 x 4 rank words.
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(FX_THREADS) void k_fix_labels(const FixWalk p) {
    __shared__ int s_w[2][FX_WAVES];
    __shared__ int s_q[2][FX_WAVES];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const bool mine = tid * FX_FPT < p.chunk;
    int par = 0;                                                 // alternates with every chunk, across the viewers too
    for (int u = blockIdx.x; u < p.U; u += gridDim.x) {
        const int32_t* d = p.dirs + (long)u * p.T;
        const int32_t* len = p.len + (long)u * p.T;
        int32_t* labels = p.labels + (long)u * p.T;
        const long long off = p.events ? p.offsets[u] : 0;
        int carry = -1;
        long long seen = 0;                                      // events of the viewer before the chunk
        for (long c0 = 0; c0 < p.T; c0 += p.chunk, par ^= 1) {
            const long f0 = c0 + (long)tid * FX_FPT;
            unsigned here, starts, ends;
            fx_flags<MODE>(p, d, f0, mine, here, starts, ends);
            int own[FX_FPT], q = 0;                              // the lengths at the thread's starts; its events
#pragma unroll
            for (int k = 0; k < FX_FPT; ++k) {
                own[k] = starts >> k & 1u ? len[f0 + k] : 0;
                q += own[k] >= p.min_frames ? 1 : 0;
            }
            int before_q = 0;
            if (p.events) {                                      // uniform over the launch
                int v = q;
#pragma unroll
                for (int o = 1; o < WAVE; o <<= 1) {
                    const int t = __shfl_up(v, o, WAVE);
                    if (lane >= o) v += t;
                }
                before_q = v - q;
                if (lane == WAVE - 1) s_q[par][wv] = v;
            }
            int s[FX_FPT];
            fx_scan_starts(starts, f0, s_w[par], carry, s);      // its barrier publishes s_q too
            if (p.events) {
                int total = 0;
#pragma unroll
                for (int w = 0; w < FX_WAVES; ++w) {
                    const int t = s_q[par][w];
                    if (w < wv) before_q += t;
                    total += t;
                }
                long long e = off + seen + before_q;
                seen += total;
#pragma unroll
                for (int k = 0; k < FX_FPT; ++k)
                    if (own[k] >= p.min_frames) {
                        if (e < p.max_events) {
                            const long f = f0 + k;
                            int32_t* ev = p.events + 4 * e;
                            ev[0] = u; ev[1] = (int32_t)f; ev[2] = own[k]; ev[3] = d[f + (own[k] - 1) / 2];
                        }
                        ++e;
                    }
            }
#pragma unroll
            for (int k = 0; k < FX_FPT; ++k) {
                const long f = f0 + k;
                if (!mine || f >= p.T) continue;
                int label = -1;
                if (here >> k & 1u) {
                    const int L = s[k] == (int)f ? own[k] : len[max(s[k], 0)];
                    label = L >= p.min_frames ? L : 0;
                }
                labels[f] = label;
            }
        }
    }
}

// bin b with e[b] <= L < e[b + 1], -1 outside the edges
__device__ __forceinline__ int fx_bin(const int* e, int B, int L) {
    if (B <= 0 || L < e[0] || L >= e[B]) return -1;
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (L >= e[mid]) lo = mid; else hi = mid;
    }
    return lo;
}

struct FixRows {
    const int32_t* labels;       // [U][T]
    const int32_t* len;          // [U][T]
    int U, T, window, stride, min_frames, B;
    long R, rows;                // rows per viewer (or of the call); R, or U * R
    int edges[FX_MAX_BINS + 1];
    // the frame totals of the pooled layout
    int* f_samples;              // [T]
    int* f_fix;                  // [T]
    int* f_events;               // [T]
    unsigned long long* f_sum;   // [T]
    int* f_max;                  // [T]
    long long* counts;           // [5][rows] or null
    int32_t* hist;               // [rows][B] or null
    int32_t* status;             // [2] or null
};

// ------------------------------------------------------------------------------------------
// k_fix_frames — the pooled layout's frame totals.  Workgroup (x, y) = frames [256 x, + 256) x viewers [64 y, + 64); lane = frame.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FX_THREADS) void k_fix_frames(const FixRows g) {
    __shared__ int s_edges[FX_MAX_BINS + 1];
    const int tid = threadIdx.x;
    const bool hist = g.hist != nullptr && g.B > 0;
    if (hist) {
        for (int i = tid; i <= g.B; i += FX_THREADS) s_edges[i] = g.edges[i];
        __syncthreads();
    }
    const long f = (long)blockIdx.x * FX_THREADS + tid;
    if (f >= g.T) return;
    const int u0 = blockIdx.y * FX_TILE_USERS, u1 = min(g.U, u0 + FX_TILE_USERS);
    // the rows that hold frame f: r * stride <= f < r * stride + window, r < R
    const long r_hi = min(g.R - 1, f / g.stride);
    const long r_lo = f < g.window ? 0 : (f - g.window) / g.stride + 1;
    int samples = 0, fix = 0, events = 0, mx = 0;
    unsigned long long sum = 0ull;
    for (int u = u0; u < u1; ++u) {
        const long i = (long)u * g.T + f;
        const int lab = g.labels[i], L = g.len[i];
        samples += lab >= 0 ? 1 : 0;
        fix += lab > 0 ? 1 : 0;
        if (L >= g.min_frames) {
            ++events; sum += (unsigned long long)L; mx = max(mx, L);
            if (hist) {
                const int b = fx_bin(s_edges, g.B, L);
                if (b >= 0)
                    for (long r = r_lo; r <= r_hi; ++r) atomicAdd(&g.hist[r * g.B + b], 1);
            }
        }
    }
    if (samples) atomicAdd(&g.f_samples[f], samples);
    if (fix) atomicAdd(&g.f_fix[f], fix);
    if (events) {
        atomicAdd(&g.f_events[f], events);
        atomicAdd(&g.f_sum[f], sum);
        atomicMax(&g.f_max[f], mx);
    }
}

// ------------------------------------------------------------------------------------------
// k_fix_rows — the counts of a row from its frames.  G threads per row (a wave, or the workgroup), 256 / G rows per workgroup,
// persistent over the rows with the same trip count in every wave.  POOLED: the frame totals; else viewer v's labels and lengths,
// and the row's histogram in LDS.
// ------------------------------------------------------------------------------------------
template <bool POOLED, int G>
__global__ __launch_bounds__(FX_THREADS) void k_fix_rows(const FixRows g) {
    constexpr int RPB = FX_THREADS / G;
    __shared__ int s_edges[FX_MAX_BINS + 1];
    __shared__ int s_hist[RPB][FX_MAX_BINS];
    __shared__ unsigned long long s_red[FX_WAVES][5];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int grp = tid / G, t = tid % G;
    const bool hist = !POOLED && g.hist != nullptr && g.B > 0;
    if (hist) for (int i = tid; i <= g.B; i += FX_THREADS) s_edges[i] = g.edges[i];
    for (long base = (long)blockIdx.x * RPB; base < g.rows; base += (long)gridDim.x * RPB) {
        const long row = base + grp;
        const bool live = row < g.rows;
        if (hist) {
            __syncthreads();                                     // the edges; the last row's histogram has been written
            for (int i = t; i < g.B; i += G) s_hist[grp][i] = 0;
            __syncthreads();
        }
        unsigned long long samples = 0ull, fix = 0ull, events = 0ull, sum = 0ull;
        int mx = 0;
        if (live) {
            const long v = POOLED ? 0 : row / g.R, r = POOLED ? row : row - v * g.R;
            const long fa = r * g.stride, fb = fa + g.window;
            for (long f = fa + t; f < fb; f += G) {
                if (POOLED) {
                    samples += (unsigned long long)g.f_samples[f]; fix += (unsigned long long)g.f_fix[f];
                    events += (unsigned long long)g.f_events[f]; sum += g.f_sum[f]; mx = max(mx, g.f_max[f]);
                } else {
                    const long i = v * g.T + f;
                    const int lab = g.labels[i], L = g.len[i];
                    samples += lab >= 0 ? 1ull : 0ull;
                    fix += lab > 0 ? 1ull : 0ull;
                    if (L >= g.min_frames) {
                        ++events; sum += (unsigned long long)L; mx = max(mx, L);
                        if (hist) {
                            const int b = fx_bin(s_edges, g.B, L);
                            if (b >= 0) atomicAdd(&s_hist[grp][b], 1);
                        }
                    }
                }
            }
        }
        samples = wave_sum(samples); fix = wave_sum(fix); events = wave_sum(events); sum = wave_sum(sum); mx = fx_wave_max(mx);
        if (G > WAVE) {
            __syncthreads();
            if (lane == 0) {
                s_red[wv][0] = samples; s_red[wv][1] = fix; s_red[wv][2] = events; s_red[wv][3] = sum;
                s_red[wv][4] = (unsigned long long)mx;
            }
            __syncthreads();
            samples = fix = events = sum = 0ull; mx = 0;
            for (int w = 0; w < FX_WAVES; ++w) {
                samples += s_red[w][0]; fix += s_red[w][1]; events += s_red[w][2]; sum += s_red[w][3];
                mx = max(mx, (int)s_red[w][4]);
            }
        }
        if (live && t == 0) {
            if (g.counts) {
                g.counts[row] = (long long)samples;
                g.counts[g.rows + row] = (long long)fix;
                g.counts[2 * g.rows + row] = (long long)events;
                g.counts[3 * g.rows + row] = (long long)sum;
                g.counts[4 * g.rows + row] = (long long)mx;
            }
            if (g.status && samples == 0ull) atomicAdd(&g.status[1], 1);
        }
        if (hist) {
            __syncthreads();
            if (live) for (int i = t; i < g.B; i += G) g.hist[row * g.B + i] = s_hist[grp][i];
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_fix_centroids — one thread per listed event: the sum of the unit vectors of its frames in ascending frame order, one accumulator
// per component from +0.0, plain adds.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FX_THREADS) void k_fix_centroids(const int32_t* dirs, const double* unit, const int T,
                                                              const long long* offsets, const int U, const int32_t* events,
                                                              const long long max_events, double* centroids) {
    const long long n = min(max_events, offsets[U]);
    for (long long e = (long long)blockIdx.x * FX_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * FX_THREADS) {
        const int32_t* ev = events + 4 * e;
        const int32_t* d = dirs + (long)ev[0] * T + ev[1];
        const int L = ev[2];
        double x = 0.0, y = 0.0, z = 0.0;
        for (int k = 0; k < L; ++k) {
            const double* A = unit + 3L * d[k];
            x += A[0]; y += A[1]; z += A[2];
        }
        centroids[3 * e] = x; centroids[3 * e + 1] = y; centroids[3 * e + 2] = z;
    }
}

}  // namespace vet

namespace vh {

// What vet_fixations* refuse about their arguments, before anything is staged, allocated or launched.
int check_fixation_args(const vet_plan* pl, int U, int T, int window, int stride, int mode, double cos_threshold, int min_frames,
                        const int32_t* edges, int B, int64_t max_events, const void* events, const void* centroids) {
    if (!pl) return fail(VET_ERR_INVALID, "plan is NULL");
    if (U <= 0 || T <= 0) return fail(VET_ERR_INVALID, "n_users and n_frames must be positive (got %d, %d)", U, T);
    if (window < 1) return fail(VET_ERR_INVALID, "window must be at least 1 frame (got %d)", window);
    if (stride < 1) return fail(VET_ERR_INVALID, "stride must be at least 1 frame (got %d)", stride);
    if (window > T) return fail(VET_ERR_INVALID, "window of %d frames is longer than the video's %d frames", window, T);
    if (min_frames < 1) return fail(VET_ERR_INVALID, "min_frames must be at least 1 (got %d)", min_frames);
    if (mode != 0 && mode != 1) return fail(VET_ERR_INVALID, "mode must be 0 (angle) or 1 (tile) (got %d)", mode);
    if (cos_threshold != cos_threshold) return fail(VET_ERR_INVALID, "cos_threshold is NaN");
    if (B < 0 || B > vet::FX_MAX_BINS) return fail(VET_ERR_INVALID, "need 0 to %d histogram bins (got %d)", vet::FX_MAX_BINS, B);
    if (B && !edges) return fail(VET_ERR_INVALID, "edges is NULL");
    for (int i = 0; i <= B && B; ++i)
        if (edges[i] < 1 || (i && edges[i] <= edges[i - 1]))
            return fail(VET_ERR_INVALID, "histogram edges must be at least 1 frame and strictly ascending (edge %d is %d)", i, edges[i]);
    if (max_events < 0) return fail(VET_ERR_INVALID, "max_events must not be negative (got %lld)", (long long)max_events);
    if (centroids && !events) return fail(VET_ERR_INVALID, "centroids need the event list (events is NULL)");
    if ((int64_t)window * U > (int64_t)0x7FFFFFFF)
        return fail(VET_ERR_UNSUPPORTED, "fixations: window * n_users = %lld positions per row (at most 2^31 - 1)", (long long)window * U);
    int rc = check_user_dirs_frames(T, "fixations");
    if (rc) return rc;
    if (mode == 1 && (pl->lat.empty() || (size_t)pl->lat[0].n * 4 > pl->ctx->lds_max))
        return fail(VET_ERR_UNSUPPORTED, "fixations: the per-viewer count path does not take lattice 0 of this plan (%d tiles)",
                    pl->lat.empty() ? 0 : pl->lat[0].n);
    return VET_OK;
}

namespace {

int launch_fixations(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window, int stride,
                     int mode, double cos_threshold, int min_frames, int per_user, const int32_t* edges, int B, int64_t max_events,
                     int64_t* d_counts, int32_t* d_hist, int32_t* d_labels, int64_t* d_offsets, int32_t* d_events,
                     double* d_centroids, int32_t* d_status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const long R = (long)vet_window_rows(T, window, stride), rows = per_user ? R * U : R;
    if (!d_hist) B = 0;
    if (!B) d_hist = nullptr;
    if (!d_events) max_events = 0;
    int chunk = vet::FX_CHUNK;
    if (c->tune.fixation_chunk > 0) chunk = std::min(chunk, std::max(vet::FX_FPT, c->tune.fixation_chunk / vet::FX_FPT * vet::FX_FPT));
    const size_t S = (size_t)U * T, Tp = per_user ? 0 : (size_t)T;
    // workspace: the transposed ids | the run lengths | the labels (where d_labels does not take them) | the viewers' event counts
    // and their prefix | the pooled layout's frame totals
    WsLayout lay;
    const size_t dirs_o = lay.take<int32_t>(S), len_o = lay.take<int32_t>(S), lab_o = lay.take<int32_t>(d_labels ? 0 : S),
                 evc_o = lay.take<int32_t>((size_t)U), off_o = lay.take<long long>((size_t)U + 1), ftot_o = lay.take<int32_t>(4 * Tp),
                 fsum_o = lay.take<unsigned long long>(Tp);
    int rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    int32_t* dirs = (int32_t*)(ws + dirs_o);
    rc = user_dirs_run(pl, d_mu, d_mv, d_ids, U, T, dirs, d_status, "fixations", s);
    if (rc) return rc;
    vet::FixWalk q{};
    q.dirs = dirs; q.unit = pl->d_dir_unit; q.raw = pl->d_dir_raw;
    q.nearest = pl->lat.empty() ? nullptr : pl->lat[0].d_nearest; q.n = pl->lat.empty() ? 0 : pl->lat[0].n;
    q.cos_thr = cos_threshold; q.U = U; q.T = T; q.chunk = chunk; q.min_frames = min_frames;
    q.len = (int32_t*)(ws + len_o); q.evcount = (int32_t*)(ws + evc_o);
    q.labels = d_labels ? d_labels : (int32_t*)(ws + lab_o);
    q.offsets = (const long long*)(ws + off_o); q.events = max_events > 0 ? d_events : nullptr; q.max_events = max_events;
    const dim3 walk_grid((unsigned)std::min<long>(U, 8L * c->n_cu)), block(vet::FX_THREADS);
    {
        ProfScope ps(c, s, KID_TRANSITION);
        if (mode) hipLaunchKernelGGL(vet::k_fix_runs<1>, walk_grid, block, 0, s, q);
        else hipLaunchKernelGGL(vet::k_fix_runs<0>, walk_grid, block, 0, s, q);
        HIP_TRY(hipGetLastError());
        if (d_offsets || q.events) {
            hipLaunchKernelGGL(vet::k_fix_offsets, dim3(1), block, 0, s, (const int32_t*)q.evcount, U, (long long*)(ws + off_o),
                               (long long*)d_offsets);
            HIP_TRY(hipGetLastError());
        }
        if (mode) hipLaunchKernelGGL(vet::k_fix_labels<1>, walk_grid, block, 0, s, q);
        else hipLaunchKernelGGL(vet::k_fix_labels<0>, walk_grid, block, 0, s, q);
        HIP_TRY(hipGetLastError());
        if (q.events && d_centroids) {
            const dim3 grid((unsigned)grid_for((long)std::min<int64_t>(max_events, (int64_t)S), vet::FX_THREADS, c->n_cu));
            hipLaunchKernelGGL(vet::k_fix_centroids, grid, block, 0, s, (const int32_t*)dirs, (const double*)pl->d_dir_unit, T,
                               q.offsets, U, (const int32_t*)d_events, (long long)max_events, d_centroids);
            HIP_TRY(hipGetLastError());
        }
    }
    if (!d_counts && !d_hist && !d_status) return VET_OK;
    vet::FixRows g{};
    g.labels = q.labels; g.len = q.len; g.U = U; g.T = T; g.window = window; g.stride = stride; g.min_frames = min_frames; g.B = B;
    g.R = R; g.rows = rows;
    for (int i = 0; i <= B && B; ++i) g.edges[i] = edges[i];
    g.counts = (long long*)d_counts; g.hist = d_hist; g.status = d_status;
    ProfScope ps(c, s, KID_FINALIZE);
    if (!per_user) {
        int* ftot = (int*)(ws + ftot_o);
        g.f_samples = ftot; g.f_fix = ftot + T; g.f_events = ftot + 2 * (size_t)T; g.f_max = ftot + 3 * (size_t)T;
        g.f_sum = (unsigned long long*)(ws + fsum_o);
        HIP_TRY(hipMemsetAsync(ftot, 0, 4 * Tp * 4, s));
        HIP_TRY(hipMemsetAsync(g.f_sum, 0, Tp * 8, s));
        if (d_hist) HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)rows * B * 4, s));
        const dim3 grid((unsigned)((T + vet::FX_THREADS - 1) / vet::FX_THREADS),
                        (unsigned)((U + vet::FX_TILE_USERS - 1) / vet::FX_TILE_USERS));
        hipLaunchKernelGGL(vet::k_fix_frames, grid, block, 0, s, g);
        HIP_TRY(hipGetLastError());
    }
    const bool wide = window > 8 * vet::WAVE;
    const long rpb = wide ? 1 : vet::FX_WAVES;
    const dim3 grid((unsigned)std::max<long>(1, std::min<long>((rows + rpb - 1) / rpb, 16L * c->n_cu)));
    if (per_user) {
        if (wide) hipLaunchKernelGGL((vet::k_fix_rows<false, vet::FX_THREADS>), grid, block, 0, s, g);
        else hipLaunchKernelGGL((vet::k_fix_rows<false, vet::WAVE>), grid, block, 0, s, g);
    } else {
        if (wide) hipLaunchKernelGGL((vet::k_fix_rows<true, vet::FX_THREADS>), grid, block, 0, s, g);
        else hipLaunchKernelGGL((vet::k_fix_rows<true, vet::WAVE>), grid, block, 0, s, g);
    }
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

}  // namespace

}  // namespace vh

using namespace vh;

extern "C" {

int vet_fixations(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, int mode,
                  double cos_threshold, int min_frames, int per_user, const int32_t* h_edges, int B, int64_t max_events,
                  int64_t* d_counts, int32_t* d_hist, int32_t* d_labels, int64_t* d_offsets, int32_t* d_events, double* d_centroids,
                  int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_fixation_args(pl, U, T, window, stride, mode, cos_threshold, min_frames, h_edges, B, max_events, d_events,
                                 d_centroids);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_fixations_ids", stream, &s);
    return rc ? rc : launch_fixations(pl, d_mu, d_mv, nullptr, U, T, window, stride, mode, cos_threshold, min_frames, per_user, h_edges,
                                      B, max_events, d_counts, d_hist, d_labels, d_offsets, d_events, d_centroids, d_status, s);
}

int vet_fixations_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, int mode, double cos_threshold,
                      int min_frames, int per_user, const int32_t* h_edges, int B, int64_t max_events, int64_t* d_counts,
                      int32_t* d_hist, int32_t* d_labels, int64_t* d_offsets, int32_t* d_events, double* d_centroids,
                      int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_fixation_args(pl, U, T, window, stride, mode, cos_threshold, min_frames, h_edges, B, max_events, d_events,
                                 d_centroids);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_fixations(pl, nullptr, nullptr, d_ids, U, T, window, stride, mode, cos_threshold, min_frames, per_user,
                                      h_edges, B, max_events, d_counts, d_hist, d_labels, d_offsets, d_events, d_centroids, d_status, s);
}

}  // extern "C"
