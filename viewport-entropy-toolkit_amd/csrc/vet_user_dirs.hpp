// vet_user_dirs.hpp — k_user_dirs: stage 1 of the per-viewer entry points (vet_user.hip: vet_user_entropy*,
// vet_user_transition.hip: vet_user_transition_entropy*, vet_user_divergence.hip: vet_user_divergence*, vet_crowd.hip:
// vet_crowd_divergence*): every sample quantised once, its direction id written transposed.  Also the two walks over one user's
// ids that build a row's histogram in LDS, each written once for the kernels of those units: user_walk_w (weighted lattices:
// k_user_entropy_w, k_user_hist_w, k_crowd_w) and user_count / user_row_count (integer counts: k_user_entropy_c, k_user_hist_c,
// k_crowd_c).
// Part of the gfx950 device code of the viewport -> tile -> entropy path (see vet_kernels.hpp for the map).
#pragma once
#include "vet_common.hpp"
#include "vet_weights_pass.hpp"

namespace vet {

constexpr int UT = 64;           // k_user_dirs: the tile is UT frames x UT users
constexpr int UT_LD = UT + 1;    // leading dimension in dwords: a row write and a column read both hit 32 distinct banks per half-wave

// ------------------------------------------------------------------------------------------
// k_user_dirs — stage 1.  Workgroup (bx, by) owns users [bx * 64, + 64) x frames [by * 64, + 64); 4 waves.
// In: wave w reads frames w, w + 4, ... of the tile, lane = user: 64 consecutive samples of one frame (coalesced), quantised
// (sample_dir) and stored as a row of the LDS tile.  Out: wave w writes users w, w + 4, ..., lane = frame: a column of the
// LDS tile, 64 consecutive ids of dirs[u] (coalesced).  Edge tiles are predicated: nothing is loaded or stored outside
// [0, T) x [0, U).  status[0] is raised by samples outside [0, 1] (ids: at or beyond the direction table) as k_window_tiles
// raises it.
// LDS: i32 [64][65].
// ------------------------------------------------------------------------------------------
struct UserDirsParams {
    SampleSrc src;
    int U, T;
    int32_t* dirs;               // [U][T]
    int32_t* status;             // [2] or null
};

template <bool FROM_IDS>
__global__ __launch_bounds__(256) void k_user_dirs(const UserDirsParams p) {
    __shared__ int32_t tile[UT * UT_LD];
    const int lane = lane_id(), wv = wave_id();
    const long u0 = (long)blockIdx.x * UT, f0 = (long)blockIdx.y * UT;
    bool bad = false;
    {
        const long u = u0 + lane;
        for (int i = wv; i < UT; i += 4) {
            const long f = f0 + i;
            int id = -1;
            if (f < p.T && u < p.U) id = sample_dir<FROM_IDS>(p.src, f * (long)p.U + u, bad);
            tile[i * UT_LD + lane] = id;
        }
    }
    __syncthreads();
    {
        const long f = f0 + lane;
        for (int j = wv; j < UT; j += 4) {
            const long u = u0 + j;
            if (u < p.U && f < p.T) p.dirs[u * (long)p.T + f] = tile[lane * UT_LD + j];
        }
    }
    if (p.status) {
        const unsigned long long anybad = __ballot(bad);
        if (anybad && lane == 0) atomicAdd(&p.status[0], (int)__popcll(anybad));
    }
}

// Counts the nearest tiles / bins of frames [fa, fb) of one user's ids d into the wave's LDS histogram cnt (delta = 1, or
// ~0u = -1 mod 2^32 for frames that leave a sliding row).  Integers, exact in any order.
__device__ __forceinline__ void user_count(unsigned* cnt, int n, const int32_t* d, const uint16_t* nearest, long fa, long fb,
                                           unsigned delta) {
    for (long f = fa + lane_id(); f < fb; f += WAVE) {
        const int id = d[f];
        if (id >= 0) {
            const int t = (int)nearest[id];
            if (t < n) atomicAdd(&cnt[t], delta);
        }
    }
}

// One row counted afresh by a one-wave workgroup (k_user_hist_c, k_crowd_c): the counts zeroed, user_count over the row's
// frames [f0, f0 + window) of the user's ids d, then each(t, count) for every tile t from the lane that owns it.  Returns the
// row's samples.
template <class Each>
__device__ __forceinline__ int user_row_count(unsigned* cnt, int n, const int32_t* d, const uint16_t* nearest, long f0, int window,
                                              Each each) {
    const int lane = lane_id();
    for (int t = lane; t < n; t += WAVE) cnt[t] = 0u;
    __syncthreads();
    user_count(cnt, n, d, nearest, f0, f0 + window, 1u);
    __syncthreads();
    int np = 0;
    for (int t = lane; t < n; t += WAVE) {
        const unsigned v = cnt[t];
        np += (int)v;
        each(t, v);
    }
    return wave_sum(np);
}

// The weighted walk of one (user, row) by a workgroup of NW = blockDim.x / 64 waves (NW is chosen by the host from `window` and
// the lattice's LDS footprint alone: user_nw): hist is the dynamic LDS, dtable_lds_bytes(NW, X.n) = f64 [NW][n] and the present
// counts i32 [NW]; d = &dirs[u][r * stride].  Wave w takes the w-th contiguous share of the row's `window` frames in ascending
// order; a 64-frame chunk is one coalesced load of 64 consecutive ids, alias[id], and add_exact_rows into the wave's own
// histogram (initialised to "no key", NO_KEY_BITS): the frames of a chunk are added in lane = frame order, the waves' histograms
// in wave order (waves_in_order).  Every row is summed from scratch.  Tile t's value v is left in hist[t] (wave 0's share) and
// handed to each(t, v) by the one thread that owns the tile; behind the closing barrier every wave may read hist[0 .. n).
// Returns the row's present samples.
template <int S, class Each>
__device__ __forceinline__ int user_walk_w(double* hist, const int32_t* d, const uint32_t* alias, const ExactRows& X, int window,
                                           Each each) {
    const int NW = blockDim.x >> 6, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int n = X.n;
    int* cnt_w = (int*)(hist + (size_t)NW * n);                    // [NW] present samples per wave
    double* h = hist + (size_t)wv * n;
    for (int t = lane; t < n; t += WAVE) ((unsigned long long*)h)[t] = NO_KEY_BITS;
    const int per = (window + NW - 1) / NW;
    const int j_begin = min(window, wv * per), j_end = min(window, j_begin + per);
    int np = 0;
    for (int j0 = j_begin; j0 < j_end; j0 += WAVE) {
        const int j = j0 + lane;
        const int id = j < j_end ? d[j] : -1;
        const uint32_t a = id >= 0 ? alias[id] : 0u;
        add_exact_rows<S>(h, X, (int)(a & 0x7FFFFFFFu), (int)(a >> 31), id >= 0, min(WAVE, j_end - j0));
        np += id >= 0 ? 1 : 0;
    }
    np = wave_sum(np);
    if (lane == 0) cnt_w[wv] = np;
    __syncthreads();
    // tile values, wave order, into wave 0's share (every slot is read and written by one thread only)
    for (int t = tid; t < n; t += blockDim.x) {
        const double v = waves_in_order(hist, NW, n, t);
        hist[t] = v;
        each(t, v);
    }
    int n_present = 0;
    for (int w2 = 0; w2 < NW; ++w2) n_present += cnt_w[w2];
    __syncthreads();
    return n_present;
}

}  // namespace vet
