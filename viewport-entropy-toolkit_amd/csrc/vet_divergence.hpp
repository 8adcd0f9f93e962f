// vet_divergence.hpp — the two scalar pieces of the Jensen-Shannon pair stages (vet_user_divergence.hip: k_user_divergence,
// vet_window_divergence.hip: k_window_divergence) and of the histogram kernels that feed them.
// Part of the gfx950 device code of the viewport -> tile -> entropy path (see vet_kernels.hpp for the map).
#pragma once
#include "vet_common.hpp"

namespace vet {

// the reference's -q log2 q is NaN for this key (0 * -inf: the value is 0.0 or underflows against the total)
__device__ __forceinline__ bool own_term_is_nan(double v, double tot) {
    const double q = v / tot;
    return isnan(q * log2(q));
}

__device__ __forceinline__ double xlog2x(double x) { return x * log2(x); }

}  // namespace vet
