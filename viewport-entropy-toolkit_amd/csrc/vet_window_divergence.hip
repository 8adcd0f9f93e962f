// vet_window_divergence.hip — window-to-window attention divergence behind vet_window_divergence* (include/vet.h): the kernels
// and their launch logic.  Rows are vet_spatial_entropy_windowed's (row r pools frames [r * stride, r * stride + window) into
// one histogram P_r per lattice, its d_weights); for every row r and lag l = 1 .. L the mass-weighted Jensen-Shannon
// divergence, in bits, of the rows r and r + l:
//     D_k(r, l) = S(P_r + P_{r+l}) - (W_r S(P_r) + W_{r+l} S(P_{r+l})) / (W_r + W_{r+l}),   S(h) = -sum_keys (h_t / W) log2(h_t / W),
// S being the reference's `entropy` before the normaliser (compute_spatial_entropy, utilities/entropy_utils.py:194-198; naive
// plans: compute_naive_spatial_entropy), then the mean over the lattices.  Output d_div[R][L], NaN where r + l >= R.
// Three stages, pair rows in chunks so that the workspace stays bounded whatever R is:
//   1  vet_spatial_entropy_windowed's stage 1, unchanged (vet_window.hip: window_frames_run): every frame's histogram once;
//   2  per lattice and chunk of pair rows [r0, r0 + CR): the row histograms [r0, min(R, r0 + CR + L)) — the chunk's rows and
//      the halo of L rows their lags reach — as [rows][n] f64 (+0.0 = no key) with the total W and a flag:
//        weighted Fibonacci lattices   k_window_hist_w: window_row_w (vet_window_hist.hpp), the sums and total
//                                      k_window_entropy_w takes (window_tile_sum: ascending frame order);
//        unweighted / binned lattices  k_window_hist_c: window_count over the row's frames, every row afresh, counts as f64;
//      the flag is raised by a row without a sample and by one whose own S is NaN under the reference's q * log2 q arithmetic;
//   3  k_window_divergence: the pair stage in k_user_divergence's overlap form.  With f(x) = x log2 x,
//        D_k = ( f(W_a + W_b) - (f(W_a) + f(W_b)) - sum_t [ f(a_t + b_t) - (f(a_t) + f(b_t)) ] ) / (W_a + W_b),
//      one FP64 log2 per tile on which BOTH rows have weight; f(a_t) is taken once per staged entry.
// Several lattices: the pair stage of lattice k ADDS D_k / K to the output in lattice order (lattice 0 stores, and writes the
// structural NaN); a NaN of any lattice stays.
// D(r, l) is a pure function of the plan, the window and the frames of rows r and r + l: the histograms are pure, one thread
// owns one pair, and its accumulator runs over the tiles in ascending order whatever the block shape, the chunk or the launch.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_window_hist.hpp"
#include "vet_row_hist.hpp"
#include "vet_divergence.hpp"

#include <algorithm>

namespace vet {

// ------------------------------------------------------------------------------------------
// k_window_hist_w — stage 2 of a weighted Fibonacci lattice for histogram rows [h0, h_end).  One wave per row, NW rows per
// workgroup, no barriers: window_row_w as in k_window_entropy_w; instead of the entropy it leaves the histogram, W and the
// flag (row_own_nan, vet_row_hist.hpp).  Lattice 0's launch writes samples[r] and
// status[1] for rows >= r_new (the rows no earlier chunk has written: halo rows are rebuilt by the next chunk).
// LDS: f64 [NW][n] (a wave reads back only what its own lanes wrote).
// ------------------------------------------------------------------------------------------
struct WindowHistWParams {
    const double* frames;        // [T][n] stage 1's frame sums
    const int32_t* present;      // [T]
    int n, window, stride;
    long h0, h_end, r_new;
    RowStats out;
    int32_t* samples;            // [R] or null
    int32_t* status;             // [2] or null
};

__global__ __launch_bounds__(256) void k_window_hist_w(const WindowHistWParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int NW = blockDim.x >> 6, lane = lane_id(), wv = wave_id();
    const long r = p.h0 + (long)blockIdx.x * NW + wv;
    if (r >= p.h_end) return;
    double* h = (double*)smem + (size_t)wv * p.n;
    const long f0 = r * (long)p.stride, slot = r - p.h0;
    double tot;
    const int np = window_row_w(h, p.frames, p.present, p.n, p.window, f0, tot, [&](int t, double acc, bool key) {
        p.out.hist[slot * (long)p.n + t] = key ? acc : 0.0;
    });
    const bool any_nan = row_own_nan(p.n, tot, KeyedHist{h, WIN_NO_KEY_BITS});
    if (lane == 0) {
        p.out.tot[slot] = tot;
        p.out.flag[slot] = (np == 0 || any_nan) ? 1 : 0;
        if (r >= p.r_new) {
            if (p.samples) p.samples[r] = np;
            if (p.status && np == 0) atomicAdd(&p.status[1], 1);
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_window_hist_c — stage 2 of an integer-count lattice (unweighted nearest tile, naive lat/lon bins) for histogram rows
// [h0, h_end).  One wave per row, blockIdx = r - h0: window_count over the row's frames, every row counted afresh; the counts
// leave as f64 (exact), W = the row's samples.  Counts never make the reference's q * log2 q NaN (q >= 1 / N), so the flag is
// "no sample".
// LDS: u32 [n].
// ------------------------------------------------------------------------------------------
struct WindowHistCParams {
    const int32_t* tiles;        // [T][U]
    int U, n, window, stride;
    long h0, r_new;
    RowStats out;
    int32_t* samples;            // [R] or null
    int32_t* status;             // [2] or null
};

__global__ __launch_bounds__(64) void k_window_hist_c(const WindowHistCParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* cnt = (unsigned*)smem;
    const int lane = lane_id();
    for (int t = lane; t < p.n; t += WAVE) cnt[t] = 0u;
    __syncthreads();
    const long slot = blockIdx.x, r = p.h0 + slot, f0 = r * (long)p.stride;
    window_count(cnt, p.n, p.tiles, p.U, f0, f0 + p.window, 1u);
    __syncthreads();
    int np = 0;
    for (int t = lane; t < p.n; t += WAVE) {
        const unsigned v = cnt[t];
        np += (int)v;
        p.out.hist[slot * (long)p.n + t] = (double)v;
    }
    np = wave_sum(np);
    if (lane == 0) {
        p.out.tot[slot] = (double)np;
        p.out.flag[slot] = np == 0 ? 1 : 0;
        if (r >= p.r_new) {
            if (p.samples) p.samples[r] = np;
            if (p.status && np == 0) atomicAdd(&p.status[1], 1);
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_window_divergence<RB, LB, TC> — stage 3.  Workgroup (x, y): pair rows [ra0, ra0 + RB), ra0 = r0 + x * RB, and lags
// [l0, l0 + LB), l0 = y * LB + 1; 256 = RB * LB threads; thread (ri = tid % RB, li = tid / RB) owns the ONE pair
// (r, l) = (ra0 + ri, l0 + li), one accumulator.
// The RB "a" histograms (rows ra0 ..) and the RB + LB - 1 consecutive "b" histograms the block's pairs reach (rows ra0 + l0 ..)
// are staged through LDS TC tiles at a time: lanes read TC consecutive tiles of one row, the entry and its f(x) = x log2 x
// (taken once per staged entry) go to arrays of leading dimension TC + 1 doubles (odd), so that the compute loop's reads
// a[ri][t] and b[ri + li][t] — consecutive rows of one column along the lanes — fall on distinct banks.  Tiles in ascending
// order, stage after stage: a pair's accumulator sees the same sequence of additions in every block shape and launch.
// Per tile and pair, k_user_divergence's statements: s = a + b; ONE unsigned compare of s's bits sends
// 0 < s < thr = (W_a + W_b) * 2^-1000 to the slow path, which performs the reference's division s / (W_a + W_b) and marks the
// pair NaN where the quotient is 0 (the pooled term's 0 * log2 0); overlap tiles (a > 0 and b > 0) add f(s) - (f(a) + f(b)).
// Output: D = ((f(W) - (f(W_a) + f(W_b))) - acc) / W, NaN where either flag or the slow path says so and where r + l >= R;
// `first` stores D / K, later lattices add.  LB = 1: the lanes run along r, contiguous in d_div when L = 1; LB > 1: the block's
// results are transposed through LDS so that the lanes run along l, contiguous in d_div[r][.].  Non-temporal stores.
// The host picks the shape from max_lag alone (window_div_shape).  LDS, static, 2 (entry, f) * (2 RB + LB - 1) * (TC + 1) * 8:
//   <256, 1, 8>   73 728 bytes (2 workgroups per CU)    max_lag = 1
//   <32, 8, 32>   37 488 bytes (4 workgroups per CU)    max_lag <= 8
//   <8, 32, 32>   24 816 bytes (6 workgroups per CU)    longer bands
// ------------------------------------------------------------------------------------------
struct WindowDivParams {
    RowStats in;
    int n;
    long h0, h_end;              // histogram rows of the chunk: [h0, h_end)
    long r0, r_end;              // pair rows of the chunk: [r0, r_end)
    long R, L;                   // rows of the call, max_lag
    int first;                   // lattice 0: store; later lattices: add
    double K;                    // lattices of the plan
    double* out;                 // [R][L]
};

template <int RB, int LB, int TC>
__global__ __launch_bounds__(256) void k_window_divergence(const WindowDivParams p) {
    static_assert(RB * LB == 256 && (TC & (TC - 1)) == 0 && RB * (TC + 1) >= RB * (LB + 1), "block shape");
    constexpr int LD = TC + 1, NB = RB + LB - 1;
    __shared__ double sa[RB * LD], sfa[RB * LD], sb[NB * LD], sfb[NB * LD];
    const int tid = threadIdx.x, ri = tid % RB, li = tid / RB;
    const long ra0 = p.r0 + (long)blockIdx.x * RB, l0 = (long)blockIdx.y * LB + 1, rb0 = ra0 + l0;
    const long r = ra0 + ri, l = l0 + li, rb = r + l;
    const bool mine = r < p.r_end && l <= p.L;                     // an element of d_div
    const bool pair = mine && rb < p.R;                            // ... that has a partner row
    const double Wa = pair ? p.in.tot[r - p.h0] : 0.0, Wb = pair ? p.in.tot[rb - p.h0] : 0.0, W = Wa + Wb;
    // bits(thr) - 1: 0 < s < thr  <=>  bits(s) - 1 < bits(thr) - 1 as unsigned (s = +0.0 wraps to the largest value; so does
    // thr = 0, which sends every s > 0 to the slow path)
    const unsigned long long thr_m1 = (unsigned long long)__double_as_longlong(ldexp(W, -1000)) - 1ull;
    double acc = 0.0;
    bool bad = false;
    for (int t0 = 0; t0 < p.n; t0 += TC) {
        __syncthreads();                                           // the previous stage has been read
        for (int i = tid; i < (RB + NB) * TC; i += 256) {
            const int row = i / TC, t = i & (TC - 1);
            const bool isb = row >= RB;
            const long hr = isb ? rb0 + (row - RB) : ra0 + row;    // rows beyond the chunk's pairs / halo hold 0.0: no key
            const double a = (hr < (isb ? p.h_end : p.r_end) && t0 + t < p.n) ? p.in.hist[(hr - p.h0) * (long)p.n + t0 + t] : 0.0;
            const int o = (isb ? row - RB : row) * LD + t;
            (isb ? sb : sa)[o] = a;
            (isb ? sfb : sfa)[o] = a > 0.0 ? xlog2x(a) : 0.0;
        }
        __syncthreads();
        if (pair) {
            for (int t = 0; t < TC; ++t) {                         // tiles beyond n hold 0.0
                const int oa = ri * LD + t, ob = (ri + li) * LD + t;
                const double a = sa[oa], b = sb[ob], s = a + b;
                if ((unsigned long long)__double_as_longlong(s) - 1ull < thr_m1) bad |= s / W == 0.0;
                if (a > 0.0 && b > 0.0) acc += xlog2x(s) - (sfa[oa] + sfb[ob]);
            }
        }
    }
    double d = __builtin_nan("");
    if (pair && !(p.in.flag[r - p.h0] || p.in.flag[rb - p.h0] || bad)) d = ((xlog2x(W) - (xlog2x(Wa) + xlog2x(Wb))) - acc) / W;
    d = d / p.K;
    if (LB == 1) {
        if (mine) {
            double* o = p.out + r * p.L + (l - 1);
            __builtin_nontemporal_store(p.first ? d : *o + d, o);
        }
        return;
    }
    __syncthreads();
    double* tile = sa;                                             // [row of the block][lag of the block], LB + 1 doubles apart
    tile[ri * (LB + 1) + li] = d;
    __syncthreads();
    const int j = tid % LB, i = tid / LB;
    const long r2 = ra0 + i, l2 = l0 + j;
    if (r2 < p.r_end && l2 <= p.L) {
        double* o = p.out + r2 * p.L + (l2 - 1);
        const double d2 = tile[i * (LB + 1) + j];
        __builtin_nontemporal_store(p.first ? d2 : *o + d2, o);
    }
}

}  // namespace vet

namespace vh {

// ---- stage 2, shared with vet_crowd.hip (vet_host.hpp): lattice k's pooled histograms of rows [h0, h_end) from stage 1's arrays
int window_hist_run(vet_plan* pl, int k, int U, const WindowFrames& wf, int window, int stride, long h0, long h_end, long r_new,
                    double* hist, double* tot, int32_t* flag, int32_t* samples, int32_t* status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const Lattice& Lk = pl->lat[k];
    const char* ws = (const char*)c->ws;
    const long hr = h_end - h0;
    const vet::RowStats st{hist, tot, flag};
    ProfScope ps(c, s, KID_FINALIZE);
    if (counts_lattice(pl, k)) {
        vet::WindowHistCParams q{};
        q.tiles = (const int32_t*)(ws + wf.off[k]); q.U = U; q.n = Lk.n; q.window = window; q.stride = stride;
        q.h0 = h0; q.r_new = r_new; q.out = st; q.samples = samples; q.status = status;
        hipLaunchKernelGGL(vet::k_window_hist_c, dim3((unsigned)hr), dim3(vet::WAVE), (size_t)Lk.n * 4, s, q);
    } else {
        vet::WindowHistWParams q{};
        q.frames = (const double*)(ws + wf.off[k]); q.present = (const int32_t*)(ws + wf.present_off);
        q.n = Lk.n; q.window = window; q.stride = stride;
        q.h0 = h0; q.h_end = h_end; q.r_new = r_new; q.out = st; q.samples = samples; q.status = status;
        int nw = 4;                                    // k_window_entropy_w's launch shape
        while (nw > 1 && (size_t)nw * Lk.n * 8 > 32 * 1024) nw /= 2;
        hipLaunchKernelGGL(vet::k_window_hist_w, dim3((unsigned)((hr + nw - 1) / nw)), dim3(nw * vet::WAVE),
                           (size_t)nw * Lk.n * 8, s, q);
    }
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

namespace {

constexpr size_t kWinDivHistBudget = (size_t)256 << 20;   // bytes of row histograms a chunk may take in the workspace

// the pair kernel's block shape: a function of max_lag alone (the kernel's header)
struct WindowDivShape { int rb, lb; const void* fn; };
WindowDivShape window_div_shape(long L) {
    if (L <= 1) return {256, 1, (const void*)vet::k_window_divergence<256, 1, 8>};
    if (L <= 8) return {32, 8, (const void*)vet::k_window_divergence<32, 8, 32>};
    return {8, 32, (const void*)vet::k_window_divergence<8, 32, 32>};
}

int check_window_div_args(const vet_plan* pl, int U, int T, int window, int stride, int max_lag, const void* out) {
    int rc = check_window_args(pl, U, T, window, stride, out);
    if (rc) return rc;
    const long R = (long)vet_window_rows(T, window, stride);
    if (R < 2) return fail(VET_ERR_INVALID, "window divergence needs at least two rows (window %d, stride %d, %d frames give %ld)",
                           window, stride, T, R);
    if (max_lag < 1 || max_lag > R - 1)
        return fail(VET_ERR_INVALID, "max_lag must be between 1 and rows - 1 = %ld (got %d)", R - 1, max_lag);
    return VET_OK;
}

int launch_window_divergence(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window,
                             int stride, int max_lag, double* d_div, int32_t* d_samples, int32_t* d_status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const int K = (int)pl->lat.size();
    const long R = (long)vet_window_rows(T, window, stride), L = max_lag;
    const WindowDivShape g = window_div_shape(L);
    // ---- what the call refuses, before anything is launched or allocated
    const long gy = (L + g.lb - 1) / g.lb;
    if (gy > 65535) return fail(VET_ERR_UNSUPPORTED, "window divergence: max_lag %ld (at most %d)", L, 65535 * g.lb);
    if (R >= (1L << 31) - 256) return fail(VET_ERR_UNSUPPORTED, "window divergence: %ld rows in one call (fewer than 2^31 - 256)", R);
    int n_max = 0;
    for (int k = 0; k < K; ++k) {
        n_max = std::max(n_max, pl->lat[k].n);
        if (!counts_lattice(pl, k) && (size_t)pl->lat[k].n * 8 > c->lds_max)
            return fail(VET_ERR_UNSUPPORTED, "window divergence: lattice of %d tiles does not fit the LDS", pl->lat[k].n);
    }
    WindowFrames wf;
    int rc = window_frames_layout(pl, U, T, 0, wf, s);
    if (rc) return rc;
    // pair rows per chunk: the histogram budget pays for the chunk's rows and the halo of L rows
    const long budget_rows = (long)(kWinDivHistBudget / ((size_t)n_max * sizeof(double)));
    long CR = c->tune.window_divergence_chunk_rows > 0 ? c->tune.window_divergence_chunk_rows : budget_rows - L;
    CR = std::max(1L, std::min(CR, R));
    const long HR = std::min(R, CR + L);
    // workspace: stage 1's arrays | hist [HR][n_max] | tot [HR] | flag [HR]
    WsLayout lay{wf.bytes};
    const size_t hist_o = lay.take<double>((size_t)HR * n_max), tot_o = lay.take<double>((size_t)HR), flag_o = lay.take<int32_t>((size_t)HR);
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
        for (int k = 0; k < K; ++k) {
            const Lattice& Lk = pl->lat[k];
            int32_t *samples = k == 0 ? d_samples : nullptr, *status = k == 0 ? d_status : nullptr;
            // ---- stage 2, charged to k_finalize
            rc = window_hist_run(pl, k, U, wf, window, stride, r0, h_end, r_new, st.hist, st.tot, st.flag, samples, status, s);
            if (rc) return rc;
            {   // ---- stage 3, charged to k_transition: the one profile id the call does not use otherwise
                vet::WindowDivParams q{};
                q.in = st; q.n = Lk.n; q.h0 = r0; q.h_end = h_end; q.r0 = r0; q.r_end = r_end; q.R = R; q.L = L;
                q.first = k == 0; q.K = (double)K; q.out = d_div;
                void* args[] = {(void*)&q};
                ProfScope ps(c, s, KID_TRANSITION);
                HIP_TRY(hipLaunchKernel(g.fn, dim3((unsigned)((r_end - r0 + g.rb - 1) / g.rb), (unsigned)gy), dim3(256), args, 0, s));
                HIP_TRY(hipGetLastError());
            }
        }
    }
    return VET_OK;
}

}  // namespace

int window_divergence_set_attrs(vet_ctx* c) {
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_window_hist_w, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_max));
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_window_hist_c, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_max));
    return VET_OK;
}

}  // namespace vh

using namespace vh;

extern "C" {

int vet_window_divergence(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, int max_lag,
                          double* d_div, int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_div_args(pl, U, T, window, stride, max_lag, d_div);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_window_divergence_ids", stream, &s);
    return rc ? rc : launch_window_divergence(pl, d_mu, d_mv, nullptr, U, T, window, stride, max_lag, d_div, d_samples, d_status, s);
}

int vet_window_divergence_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, int max_lag, double* d_div,
                              int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_div_args(pl, U, T, window, stride, max_lag, d_div);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_window_divergence(pl, nullptr, nullptr, d_ids, U, T, window, stride, max_lag, d_div, d_samples, d_status, s);
}

}  // extern "C"
