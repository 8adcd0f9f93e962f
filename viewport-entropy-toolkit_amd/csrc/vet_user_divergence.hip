// vet_user_divergence.hip — pairwise viewer divergence behind vet_user_divergence* (include/vet.h): the kernels and their launch
// logic.  For every row r (frames [r * stride, r * stride + window)) a U x U matrix: D(u, v) is the Jensen-Shannon divergence, in
// bits, of the two viewers' row histograms h_u and h_v — vet_user_entropy's d_weights — each viewer weighted by their mass:
//     D_k(u, v) = S(h_u + h_v) - (W_u S(h_u) + W_v S(h_v)) / (W_u + W_v),   S(h) = -sum_keys (h_t / W) log2(h_t / W),
// S being the reference's `entropy` before the normaliser (compute_spatial_entropy, utilities/entropy_utils.py:194-198; naive
// plans: compute_naive_spatial_entropy), then the mean over the lattices.
// Three stages, rows in chunks so that the workspace stays bounded whatever R is:
//   1  k_user_dirs (vet_user_dirs.hpp, unchanged): direction ids transposed once, dirs[U][T];
//   2  per lattice and chunk of rows, every viewer's histogram [rows of the chunk][U][n] f64 with its total W and a flag:
//        weighted Fibonacci lattices   k_user_hist_w: user_walk_w (vet_user_dirs.hpp), the walk k_user_entropy_w runs, at
//                                      the wave split user_nw() gives vet_user_entropy, and row_total in wave 0;
//        unweighted / binned lattices  k_user_hist_c: user_count over the row's frames, counts as f64;
//      the flag is raised by a viewer without a sample in the row and by one whose own S is NaN under the reference's
//      q * log2 q arithmetic (a key whose value is 0.0, or whose h_t / W underflows to 0);
//   3  k_user_divergence: the pair stage, in the overlap form.  With f(x) = x log2 x,
//        W S(h) = f(W) - sum_t f(h_t), so
//        D_k = ( f(W_u + W_v) - (f(W_u) + f(W_v)) - sum_t [ f(a_t + b_t) - (f(a_t) + f(b_t)) ] ) / (W_u + W_v),
//      and the bracket is zero unless both viewers have weight on tile t: a pair costs one FP64 log2 per tile of the OVERLAP of
//      the two supports (the viewers' own sum_t f(h_t) cancel: nothing of them is kept).  f(a_t) is taken once per staged
//      histogram entry, not per pair.
// Several lattices: the pair stage of lattice k ADDS D_k / K to the output in lattice order (lattice 0 stores), the same for
// every pair; a NaN of any lattice stays.
// What bounds k_user_divergence: the FP64 log2 (a software routine of ~40 FP64 VALU operations on the quarter-rate-or-slower
// FP64 pipe) of the overlap tiles; per tile and thread the rest is 1 + 4 LDS reads (the 4 are wave-uniform broadcasts), 4 adds
// and 8 compares.  Global traffic is 2 * 32 * n * 8 bytes read per 32 x 32 block of pairs against 16 KB written, so HBM is not
// the limit; LDS is 33 KB per workgroup (4 workgroups = 16 waves per CU of the 160 KB).
// D(u, v) is a pure function of the plan, the window and the two viewers' own samples of the row: the histograms are
// vet_user_entropy's (pure), and the pair's accumulator runs over the tiles in ascending order whatever the blocking.  Every
// operation on (a, b) is commutative, and the lower triangle is copied from the upper: the matrix is symmetric bit for bit.
// No CPU compute path; nothing here reads the environment.
#include "vet_host.hpp"
#include "vet_common.hpp"
#include "vet_spatial_dtable.hpp"
#include "vet_user_dirs.hpp"
#include "vet_row_hist.hpp"
#include "vet_divergence.hpp"

#include <algorithm>

namespace vet {

// ------------------------------------------------------------------------------------------
// k_user_hist_w — stage 2 of a weighted Fibonacci lattice for rows [r0, r0 + CR).  One workgroup per (row, user),
// blockIdx = (r - r0) * U + u.  user_walk_w and row_total as in k_user_entropy_w (same NW from the host); instead of the
// normalised entropy it leaves the histogram, W and the flag (row_own_nan).  Lattice 0's launch also writes samples[u][r] and
// status[1] as vet_user_entropy does.
// LDS: dtable_lds_bytes(NW, n).
// ------------------------------------------------------------------------------------------
struct UserHistWParams {
    const int32_t* dirs;         // [U][T]
    int T, U;
    const uint32_t* alias;       // [n_dirs] direction -> row | mirrored << 31
    ExactRows X;
    int window, stride;
    long R, r0;                  // rows per user, first row of the chunk
    RowStats out;
    int32_t* samples;            // [U][R] or null
    int32_t* status;             // [2] or null
};

template <int S>
__global__ __launch_bounds__(256) void k_user_hist_w(const UserHistWParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* hist = (double*)smem;                                  // [NW][n]
    const int n = p.X.n;
    const long slot = blockIdx.x, rc = slot / p.U, u = slot - rc * p.U, r = p.r0 + rc;
    const int n_present = user_walk_w<S>(hist, p.dirs + u * (long)p.T + r * (long)p.stride, p.alias, p.X, p.window, [&](int t, double v) {
        const bool key = (unsigned long long)__double_as_longlong(v) != NO_KEY_BITS;
        p.out.hist[slot * (long)n + t] = key ? v : 0.0;
    });
    if (wave_id() != 0) return;
    const KeyedHist keys{hist, NO_KEY_BITS};
    const double tot = row_total(n, keys);
    const bool any_nan = row_own_nan(n, tot, keys);
    if (lane_id() == 0) {
        p.out.tot[slot] = tot;
        p.out.flag[slot] = (n_present == 0 || any_nan) ? 1 : 0;
        if (p.samples) p.samples[u * p.R + r] = n_present;
        if (p.status && n_present == 0) atomicAdd(&p.status[1], 1);
    }
}

// ------------------------------------------------------------------------------------------
// k_user_hist_c — stage 2 of an integer-count lattice (unweighted nearest tile, naive lat/lon bins) for rows [r0, r0 + CR).
// One wave per (row, user), blockIdx = (r - r0) * U + u: user_row_count (vet_user_dirs.hpp) over the row's frames, every row
// counted afresh; the counts leave as f64 (exact), W = the row's samples.  Counts of present viewers never make the
// reference's q * log2 q NaN (q >= 1 / N), so the flag is "no sample".
// LDS: u32 [n].
// ------------------------------------------------------------------------------------------
struct UserHistCParams {
    const int32_t* dirs;         // [U][T]
    int T, U;
    const uint16_t* nearest;     // [n_dirs] direction -> tile / bin
    int n;
    int window, stride;
    long R, r0;
    RowStats out;
    int32_t* samples;            // [U][R] or null
    int32_t* status;             // [2] or null
};

__global__ __launch_bounds__(64) void k_user_hist_c(const UserHistCParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* cnt = (unsigned*)smem;
    const int lane = lane_id();
    const long slot = blockIdx.x, rc = slot / p.U, u = slot - rc * p.U, r = p.r0 + rc;
    const int np = user_row_count(cnt, p.n, p.dirs + u * (long)p.T, p.nearest, r * (long)p.stride, p.window, [&](int t, unsigned v) {
        p.out.hist[slot * (long)p.n + t] = (double)v;
    });
    if (lane == 0) {
        p.out.tot[slot] = (double)np;
        p.out.flag[slot] = np == 0 ? 1 : 0;
        if (p.samples) p.samples[u * p.R + r] = np;
        if (p.status && np == 0) atomicAdd(&p.status[1], 1);
    }
}

// ------------------------------------------------------------------------------------------
// k_user_divergence — stage 3.  Workgroup (x, y): row r0 + y of the chunk, the x-th DIV_B x DIV_B block of pairs of the upper
// triangle (block row bi <= block column bj, numbered row by row); 256 threads.  Thread (ti = tid % 32, tj = tid / 32) owns
// the pairs (u, v) = (bi * 32 + ti, bj * 32 + tj + 8 q), q = 0..3, one accumulator each.
// The two groups of 32 histograms are staged through LDS DIV_TC tiles at a time: lanes read 32 consecutive tiles of one
// viewer (256 contiguous bytes), the entry and its f(a) = a log2 a go to two arrays of leading dimension DIV_TC + 1 doubles,
// so that the compute loop's read a[ti][t] (32 rows, one column) covers all 64 banks once; b[tj + 8 q][t] is the same
// address for every lane of a half-wave (broadcast).  Tiles in ascending order, chunk after chunk: the accumulator of a pair
// sees the same sequence of additions wherever the pair lies in the launch.
// Per tile and pair: s = a + b; ONE unsigned compare of s's bits sends 0 < s < thr = (W_u + W_v) * 2^-1000 to the slow path,
// which performs the reference's division s / (W_u + W_v) and marks the pair NaN where the quotient is 0 (the pooled term's
// 0 * log2 0); overlap tiles (a > 0 and b > 0) add f(s) - (f(a) + f(b)).
// Output: D = ((f(W) - (f(W_u) + f(W_v))) - acc) / W, NaN where either flag or the slow path says so, +0.0 / NaN on the
// diagonal; `first` stores D / K, later lattices add.  The mirrored element D(v, u) leaves from the registers (lanes run along
// u: contiguous); D(u, v) is transposed through LDS first so that its lanes run along v.  Diagonal blocks take the lower
// triangle from the upper.  Non-temporal stores: the matrix is not read again by this call (later lattices excepted).
// LDS: 4 arrays f64 [32][33] = 33 792 bytes, static.
// ------------------------------------------------------------------------------------------
constexpr int DIV_B = 32;             // viewers per side of a pair block
constexpr int DIV_TC = 32;            // tiles per LDS stage
constexpr int DIV_LD = DIV_TC + 1;    // leading dimension in doubles

struct UserDivParams {
    RowStats in;
    int U, n, nblk;              // nblk = ceil(U / DIV_B)
    int first;                   // lattice 0: store; later lattices: add
    double K;                    // lattices of the plan
    double* out;                 // [CR][U][U], the chunk's first row
};

__global__ __launch_bounds__(256) void k_user_divergence(const UserDivParams p) {
    __shared__ double sa[2][DIV_B * DIV_LD], sf[2][DIV_B * DIV_LD];
    const int tid = threadIdx.x, ti = tid & (DIV_B - 1), tj = tid >> 5;
    int bi = 0, rest = (int)blockIdx.x;
    while (rest >= p.nblk - bi) { rest -= p.nblk - bi; ++bi; }
    const int bj = bi + rest;
    const long rc = blockIdx.y;
    const double* H = p.in.hist + rc * (long)p.U * p.n;
    const double* tot = p.in.tot + rc * (long)p.U;
    const int32_t* flag = p.in.flag + rc * (long)p.U;
    const int u = bi * DIV_B + ti;
    const double Wu = u < p.U ? tot[u] : 0.0;
    double Wv[4], W[4], acc[4];
    unsigned long long thr_m1[4];
    bool bad[4];
    for (int q = 0; q < 4; ++q) {
        const int v = bj * DIV_B + tj + 8 * q;
        Wv[q] = v < p.U ? tot[v] : 0.0;
        W[q] = Wu + Wv[q];
        // bits(thr) - 1: 0 < s < thr  <=>  bits(s) - 1 < bits(thr) - 1 as unsigned (s = +0.0 wraps to the largest value; so
        // does thr = 0, which sends every s > 0 to the slow path)
        thr_m1[q] = (unsigned long long)__double_as_longlong(ldexp(W[q], -1000)) - 1ull;
        acc[q] = 0.0;
        bad[q] = false;
    }
    for (int t0 = 0; t0 < p.n; t0 += DIV_TC) {
        __syncthreads();                                           // the previous stage has been read
        for (int i = tid; i < 2 * DIV_B * DIV_TC; i += 256) {
            const int g = i / (DIV_B * DIV_TC), row = (i / DIV_TC) & (DIV_B - 1), t = i & (DIV_TC - 1);
            const int usr = (g ? bj : bi) * DIV_B + row;
            const double a = (usr < p.U && t0 + t < p.n) ? H[usr * (long)p.n + t0 + t] : 0.0;
            sa[g][row * DIV_LD + t] = a;
            sf[g][row * DIV_LD + t] = a > 0.0 ? xlog2x(a) : 0.0;
        }
        __syncthreads();
        for (int t = 0; t < DIV_TC; ++t) {                         // tiles beyond n hold 0.0: no key for anyone
            const double a = sa[0][ti * DIV_LD + t];
            for (int q = 0; q < 4; ++q) {
                const int o = (tj + 8 * q) * DIV_LD + t;
                const double b = sa[1][o], s = a + b;
                if ((unsigned long long)__double_as_longlong(s) - 1ull < thr_m1[q]) bad[q] |= s / W[q] == 0.0;
                if (a > 0.0 && b > 0.0) acc[q] += xlog2x(s) - (sf[0][ti * DIV_LD + t] + sf[1][o]);
            }
        }
    }
    __syncthreads();
    const int fu = u < p.U ? flag[u] : 1;
    double dq[4];
    double* tile = sa[0];                                          // [u of the block][v of the block]
    for (int q = 0; q < 4; ++q) {
        const int vl = tj + 8 * q, v = bj * DIV_B + vl;
        const int fv = v < p.U ? flag[v] : 1;
        double d;
        if (u == v) d = fu ? __builtin_nan("") : 0.0;
        else if (fu || fv || bad[q]) d = __builtin_nan("");
        else d = ((xlog2x(W[q]) - (xlog2x(Wu) + xlog2x(Wv[q]))) - acc[q]) / W[q];
        dq[q] = d / p.K;
        tile[ti * DIV_LD + vl] = dq[q];
    }
    __syncthreads();
    const bool diag = bi == bj;
    for (int q = 0; q < 4; ++q) {
        // D(u', v'): u' = block row tj + 8 q, v' = lane ti — lanes run along v
        const int ul = tj + 8 * q, uu = bi * DIV_B + ul, vv = bj * DIV_B + ti;
        if (uu < p.U && vv < p.U) {
            const double d = (diag && ul > ti) ? tile[ti * DIV_LD + ul] : tile[ul * DIV_LD + ti];
            double* o = p.out + (rc * (long)p.U + uu) * p.U + vv;
            __builtin_nontemporal_store(p.first ? d : *o + d, o);
        }
        // D(v, u), mirrored, of this thread's own pairs — lanes run along u; a diagonal block is complete without it
        const int v = bj * DIV_B + tj + 8 * q;
        if (!diag && u < p.U && v < p.U) {
            double* o = p.out + (rc * (long)p.U + v) * p.U + u;
            __builtin_nontemporal_store(p.first ? dq[q] : *o + dq[q], o);
        }
    }
}

}  // namespace vet

namespace vh {

static const void* hist_w_kernel(int stride) { return VET_KERNEL_BY_S(vet::k_user_hist_w, row_chunk_class(stride)); }

// stage 2 of lattice k for rows [r0, r0 + cr), charged as vet_user_entropy's (declared in vet_host.hpp: vet_bootstrap.hip builds the
// same histograms)
int user_hist_run(vet_plan* pl, int k, const int32_t* dirs, int U, int T, int window, int stride, long R, long r0, long cr,
                  double* hist, double* tot, int32_t* flag, int32_t* samples, int32_t* status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const Lattice& L = pl->lat[k];
    const vet::RowStats st{hist, tot, flag};
    if (counts_lattice(pl, k)) {
        vet::UserHistCParams q{};
        q.dirs = dirs; q.T = T; q.U = U; q.nearest = L.d_nearest; q.n = L.n; q.window = window; q.stride = stride;
        q.R = R; q.r0 = r0; q.out = st; q.samples = samples; q.status = status;
        ProfScope ps(c, s, KID_FINALIZE);
        hipLaunchKernelGGL(vet::k_user_hist_c, dim3((unsigned)(cr * U)), dim3(vet::WAVE), (size_t)L.n * 4, s, q);
    } else {
        vet::UserHistWParams q{};
        q.dirs = dirs; q.T = T; q.U = U; q.alias = pl->d_alias; q.X = exact_rows_arg(pl, k);
        q.window = window; q.stride = stride; q.R = R; q.r0 = r0; q.out = st; q.samples = samples; q.status = status;
        const int nw = user_nw(c->lds_max, L.n, window);
        void* args[] = {(void*)&q};
        ProfScope ps(c, s, KID_WEIGHTS);
        HIP_TRY(hipLaunchKernel(hist_w_kernel(q.X.stride), dim3((unsigned)(cr * U)), dim3(nw * vet::WAVE), args,
                                vet::dtable_lds_bytes(nw, L.n), s));
    }
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

namespace {

constexpr size_t kDivHistBudget = (size_t)256 << 20;      // bytes of histograms a chunk of rows may take in the workspace

int launch_divergence(vet_plan* pl, const double* d_mu, const double* d_mv, const int32_t* d_ids, int U, int T, int window,
                      int stride, double* d_div, int32_t* d_samples, int32_t* d_status, hipStream_t s) {
    vet_ctx* c = pl->ctx;
    const int K = (int)pl->lat.size();
    const long R = (long)vet_window_rows(T, window, stride);
    // ---- what the call refuses, before anything is launched or allocated
    if (R * (long)U >= (1L << 31))
        return fail(VET_ERR_UNSUPPORTED, "viewer divergence: %ld rows x users in one call (fewer than 2^31)", R * (long)U);
    const long nblk = ((long)U + vet::DIV_B - 1) / vet::DIV_B, pair_blocks = nblk * (nblk + 1) / 2;
    if (pair_blocks >= (1L << 31))
        return fail(VET_ERR_UNSUPPORTED, "viewer divergence: %d users give %ld pair blocks in one launch (fewer than 2^31)", U,
                    pair_blocks);
    int rc = check_user_dirs_frames(T, "viewer divergence");
    if (rc) return rc;
    rc = check_user_plan(pl, "viewer divergence", s);
    if (rc) return rc;
    int n_max = 0;
    for (int k = 0; k < K; ++k) n_max = std::max(n_max, pl->lat[k].n);
    // rows per chunk: the histogram budget, the y extent of the pair launch and the x extent of the histogram launch
    long CR = c->tune.divergence_chunk_rows > 0 ? c->tune.divergence_chunk_rows
                                                : (long)(kDivHistBudget / ((size_t)U * n_max * sizeof(double)));
    CR = std::max(1L, std::min({CR, R, 65535L, ((1L << 31) - 1) / U}));
    // workspace: dirs [U][T] | hist [CR][U][n_max] | tot [CR][U] | flag [CR][U]
    WsLayout lay;
    const size_t dirs_o = lay.take<int32_t>((size_t)U * T), hist_o = lay.take<double>((size_t)CR * U * n_max),
                 tot_o = lay.take<double>((size_t)CR * U), flag_o = lay.take<int32_t>((size_t)CR * U);
    rc = ensure_ws(c, lay.at);
    if (rc) return rc;
    char* ws = (char*)c->ws;
    int32_t* dirs = (int32_t*)(ws + dirs_o);
    const vet::RowStats st{(double*)(ws + hist_o), (double*)(ws + tot_o), (int32_t*)(ws + flag_o)};
    // ---- stage 1
    rc = user_dirs_run(pl, d_mu, d_mv, d_ids, U, T, dirs, d_status, "viewer divergence", s);
    if (rc) return rc;
    for (long r0 = 0; r0 < R; r0 += CR) {
        const long cr = std::min(CR, R - r0);
        for (int k = 0; k < K; ++k) {
            const Lattice& L = pl->lat[k];
            rc = user_hist_run(pl, k, dirs, U, T, window, stride, R, r0, cr, st.hist, st.tot, st.flag, k == 0 ? d_samples : nullptr,
                               k == 0 ? d_status : nullptr, s);
            if (rc) return rc;
            {   // ---- stage 3, charged to k_finalize
                vet::UserDivParams q{};
                q.in = st; q.U = U; q.n = L.n; q.nblk = (int)nblk; q.first = k == 0; q.K = (double)K;
                q.out = d_div + (size_t)r0 * U * U;
                ProfScope ps(c, s, KID_FINALIZE);
                hipLaunchKernelGGL(vet::k_user_divergence, dim3((unsigned)pair_blocks, (unsigned)cr), dim3(256), 0, s, q);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    return VET_OK;
}

}  // namespace

int user_divergence_set_attrs(vet_ctx* c) {
    for (int stride : {64, 128, 256, 512})
        HIP_TRY(hipFuncSetAttribute(hist_w_kernel(stride), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_max));
    HIP_TRY(hipFuncSetAttribute((const void*)vet::k_user_hist_c, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_max));
    return VET_OK;
}

}  // namespace vh

using namespace vh;

extern "C" {

int vet_user_divergence(vet_plan* pl, const double* d_mu, const double* d_mv, int U, int T, int window, int stride, double* d_div,
                        int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_args(pl, U, T, window, stride, d_div);
    if (!rc) rc = entry_samples(pl, d_mu, d_mv, nullptr, "vet_user_divergence_ids", stream, &s);
    return rc ? rc : launch_divergence(pl, d_mu, d_mv, nullptr, U, T, window, stride, d_div, d_samples, d_status, s);
}

int vet_user_divergence_ids(vet_plan* pl, const int32_t* d_ids, int U, int T, int window, int stride, double* d_div,
                            int32_t* d_samples, int32_t* d_status, void* stream) {
    hipStream_t s;
    int rc = check_window_args(pl, U, T, window, stride, d_div);
    if (!rc) rc = entry_samples(pl, nullptr, nullptr, d_ids, nullptr, stream, &s);
    return rc ? rc : launch_divergence(pl, nullptr, nullptr, d_ids, U, T, window, stride, d_div, d_samples, d_status, s);
}

}  // extern "C"
