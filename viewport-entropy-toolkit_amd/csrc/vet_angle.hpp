// vet_angle.hpp — the angle between two directions of the plan's direction table and the small rules that the angle statistics
// share: vet_motion.hip (vet_head_motion*: a viewer's two directions `lag` frames apart) and vet_dispersion.hip (vet_dispersion*:
// two viewers' directions in one frame).  One definition of the angle, of the edge histogram's bin and of a block's total.
// Part of the gfx950 device code of the viewport -> tile -> entropy path (see vet_kernels.hpp for the map).
#pragma once
#include "vet_common.hpp"

namespace vet {

// The reference's vector_angle_distance of two Vectors given by their rows of the unit table (ax.. and bx..) and their direction
// ids: c = fma(A.z, B.z, fma(A.y, B.y, A.x * B.x)), acos(clip(c)); +0.0 exactly for the same id and for the same Vector under
// another id (the pole rows of a grid; the raw Vectors are compared only when the cosine is near 1).  Symmetric in (a, b): the
// products commute and the fused dot adds them in one order.  ia, ib >= 0.
__device__ __forceinline__ double unit_angle(int ia, int ib, double ax, double ay, double az, double bx, double by, double bz,
                                             const double* raw) {
    if (ia == ib) return 0.0;
    const double c = fma(az, bz, fma(ay, by, ax * bx));
    if (c > 0.999999) {          // the same Vector under another id (the pole rows of a grid): still
        const double* ra = raw + 3L * ia;
        const double* rb = raw + 3L * ib;
        if (ra[0] == rb[0] && ra[1] == rb[1] && ra[2] == rb[2]) return 0.0;
    }
    return acos(clip_unit(c));
}

// Whether the two directions are within a cone given by its cosine (vet_viewer_clusters*): the same id, the same Vector under
// another id (unit_angle's rule), or c >= cos_thr for unit_angle's fused dot c.  No acos; a NaN c is not near.  Symmetric in (a, b).
__device__ __forceinline__ bool unit_near(int ia, int ib, double ax, double ay, double az, double bx, double by, double bz,
                                          double cos_thr, const double* raw) {
    if (ia == ib) return true;
    const double c = fma(az, bz, fma(ay, by, ax * bx));
    if (c >= cos_thr) return true;
    if (c > 0.999999) {          // only a threshold above that leaves the same Vector to be found
        const double* ra = raw + 3L * ia;
        const double* rb = raw + 3L * ib;
        return ra[0] == rb[0] && ra[1] == rb[1] && ra[2] == rb[2];
    }
    return false;
}

// the same of two direction ids, the unit vectors gathered from the table; NaN where either is absent
__device__ __forceinline__ double motion_angle(int ia, int ib, const double* unit, const double* raw) {
    if (ia < 0 || ib < 0) return __builtin_nan("");
    const double* A = unit + 3L * ia;
    const double* B = unit + 3L * ib;
    return unit_angle(ia, ib, A[0], A[1], A[2], B[0], B[1], B[2], raw);
}

// bin b with e[b] <= a < e[b + 1], -1 outside the edges
__device__ __forceinline__ int mo_bin(const double* e, int B, double a) {
    if (B <= 0 || !(a >= e[0]) || !(a < e[B])) return -1;
    int lo = 0, hi = B;                                          // e[lo] <= a < e[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a >= e[mid]) lo = mid; else hi = mid;
    }
    return lo;
}

// the four waves' sums of a block in order
__device__ __forceinline__ double mo_block_total(const double* w) { return ((w[0] + w[1]) + w[2]) + w[3]; }

}  // namespace vet
