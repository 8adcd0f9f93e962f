// vet_rank.hpp — ordering values in LDS, written once for the units that summarise a row's replicates (vet_bootstrap.hip,
// vet_group.hip) and for the permutation draw of vet_group.hip: the bitonic sort of a power-of-two array by one 256-thread
// workgroup, and the quantile by linear interpolation between order statistics.
// Part of the gfx950 device code of the viewport -> tile -> entropy path (see vet_kernels.hpp for the map).
#pragma once
#include "vet_common.hpp"

namespace vet {

// x[0 .. P) in LDS, P a power of two, ascending; every thread of the 256-thread workgroup calls it.  Begins and ends with a
// barrier: what the threads wrote to x before the call is seen, and the sorted array is complete on return.
template <class T>
__device__ __forceinline__ void lds_bitonic_sort(T* x, int P) {
    const int tid = threadIdx.x;
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = tid; i < P; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const T a = x[i], b = x[l];
                    if ((a > b) == ((i & k) == 0)) { x[i] = b; x[l] = a; }
                }
            }
        }
    __syncthreads();
}

// the quantile q of the ascending x[0 .. m), m >= 1: linear interpolation between the order statistics at position q (m - 1)
__device__ __forceinline__ double lerp_quantile(const double* x, int m, double q) {
    const double pos = q * (double)(m - 1);
    const int i = (int)floor(pos);
    if (i >= m - 1) return x[m - 1];
    return x[i] + (x[i + 1] - x[i]) * (pos - (double)i);
}

}  // namespace vet
