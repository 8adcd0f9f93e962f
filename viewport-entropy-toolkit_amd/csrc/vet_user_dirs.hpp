// vet_user_dirs.hpp — k_user_dirs: stage 1 of the per-viewer entry points (vet_user.hip: vet_user_entropy*,
// vet_user_transition.hip: vet_user_transition_entropy*, vet_user_divergence.hip: vet_user_divergence*): every sample quantised
// once, its direction id written transposed.  Also user_count, the counting walk over one user's ids.
// Part of the gfx950 device code of the viewport -> tile -> entropy path (see vet_kernels.hpp for the map).
#pragma once
#include "vet_common.hpp"

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
// ~0u = -1 mod 2^32 for frames that leave a sliding row): k_user_entropy_c and k_user_hist_c.  Integers, exact in any order.
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

}  // namespace vet
