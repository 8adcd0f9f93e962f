// vet_window_hist.hpp — how a window's pooled histogram is built from stage 1's per-frame arrays: the device helpers shared by
// k_window_entropy_w/_c (vet_window.hip: vet_spatial_entropy_windowed*) and k_window_hist_w/_c (vet_window_divergence.hip:
// vet_window_divergence*), so that the two give the same bits.
// Part of the gfx950 device code of the viewport -> tile -> entropy path (see vet_kernels.hpp for the map).
#pragma once
#include "vet_common.hpp"

namespace vet {

// -0.0 = "no key" in an FP64 histogram (vet_spatial_sweep.hpp: NO_KEY_BITS; the window units do not include the sweep kernels)
constexpr unsigned long long WIN_NO_KEY_BITS = 0x8000000000000000ull;

__device__ __forceinline__ double window_term(double v) { return v == 0.0 ? -v : v; }   // dense encoding -> histogram value

// Tile t of a weighted row: col = &hist[f0][t] of stage 1's [T][n] frame sums in the dense tile_weights encoding; the window's
// frames added in ascending frame order onto "no key" (-0.0), four loads in flight.
__device__ __forceinline__ double window_tile_sum(const double* col, int n, int window) {
    double acc = __longlong_as_double((long long)WIN_NO_KEY_BITS);
    int j = 0;
    for (; j + 4 <= window; j += 4) {
        const double v0 = col[(long)j * n], v1 = col[(long)(j + 1) * n], v2 = col[(long)(j + 2) * n], v3 = col[(long)(j + 3) * n];
        acc += window_term(v0); acc += window_term(v1); acc += window_term(v2); acc += window_term(v3);
    }
    for (; j < window; ++j) acc += window_term(col[(long)j * n]);
    return acc;
}

// A weighted row in one wave (k_window_entropy_w, k_window_hist_w): the present samples of frames [f0, f0 + window), and per tile
// (lane l owns tiles l, l + 64, ...) window_tile_sum over stage 1's frames[T][n], left in the wave's LDS histogram h[n] and
// handed to each(t, acc, key) — key: the tile is a key of the row.  tot = the keys' values added in lane order, wave_sum's
// butterfly.  Returns the row's samples.
template <class Each>
__device__ __forceinline__ int window_row_w(double* h, const double* frames, const int32_t* present, int n, int window, long f0,
                                            double& tot, Each each) {
    const int lane = lane_id();
    int np = 0;
    for (int j = lane; j < window; j += WAVE) np += present[f0 + j];
    np = wave_sum(np);
    double part = 0.0;
    for (int t = lane; t < n; t += WAVE) {
        const double acc = window_tile_sum(frames + f0 * (long)n + t, n, window);
        h[t] = acc;
        const bool key = (unsigned long long)__double_as_longlong(acc) != WIN_NO_KEY_BITS;
        if (key) part += acc;
        each(t, acc, key);
    }
    tot = wave_sum(part);
    return np;
}

// Counts the tiles / bins of frames [fa, fb) of stage 1's tiles[T][U] into the wave's LDS histogram cnt (delta = 1, or
// ~0u = -1 mod 2^32 for frames that leave a sliding run of rows).  Integers, exact in any order.
__device__ __forceinline__ void window_count(unsigned* cnt, int n, const int32_t* tiles, int U, long fa, long fb, unsigned delta) {
    const int32_t* q = tiles + fa * (long)U;
    const long m = (fb - fa) * (long)U;
    for (long i = lane_id(); i < m; i += WAVE) {
        const int t = q[i];
        if ((unsigned)t < (unsigned)n) atomicAdd(&cnt[t], delta);      // -1 = absent
    }
}

}  // namespace vet
