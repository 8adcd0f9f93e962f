// vet_row_hist.hpp — what one wave does with a finished row histogram, written once for the row calls: the per-viewer units
// (vet_user.hip, vet_user_divergence.hip, vet_crowd.hip, vet_bootstrap.hip) and the windowed units (vet_window.hip, vet_window_divergence.hip).
// A row histogram is seen through a functor value(t, v): whether tile t is a key of the row, and its value v — KeyedHist for an
// FP64 histogram in LDS with a "no key" bit pattern (the caller says which: NO_KEY_BITS and WIN_NO_KEY_BITS stay two names), a
// lambda over u32 counts in vet_crowd.hip, over a replicate's FP64 sums in vet_bootstrap.hip.  Every loop runs over the tiles in lane order and ends in wave_sum's butterfly (or
// a ballot), so a value does not depend on which kernel asked for it.  Also RowStats, what the histogram kernels of the
// divergence calls leave per row, and the reference's epilogue over integer counts.
// Part of the gfx950 device code of the viewport -> tile -> entropy path (see vet_kernels.hpp for the map).
#pragma once
#include "vet_common.hpp"
#include "vet_divergence.hpp"

namespace vet {

// what a histogram kernel leaves per row of a chunk (k_user_hist_w/_c: row = (row of the chunk, viewer); k_window_hist_w/_c:
// row = histogram row of the chunk), next to the histogram
struct RowStats {
    double* hist;                // [rows][n]  h_t (+0.0 where the row has no key)
    double* tot;                 // [rows]     W
    int32_t* flag;               // [rows]     1: no sample in the row, or the row's own S is NaN
};

// an FP64 histogram h[n] in LDS whose tiles without a key hold the bit pattern no_key
struct KeyedHist {
    const double* h;
    unsigned long long no_key;
    __device__ __forceinline__ bool operator()(int t, double& v) const {
        v = h[t];
        return (unsigned long long)__double_as_longlong(v) != no_key;
    }
};

// W: the keys' values added in lane order
template <class V>
__device__ __forceinline__ double row_total(int n, V value) {
    double tot = 0.0;
    for (int t = lane_id(); t < n; t += WAVE) {
        double v;
        if (value(t, v)) tot += v;
    }
    return wave_sum(tot);
}

// S: -sum q log2 q over the keys in lane order, q = v / tot (the reference's term: NaN for q = 0)
template <class V>
__device__ __forceinline__ double row_entropy(int n, double tot, V value) {
    double hh = 0.0;
    for (int t = lane_id(); t < n; t += WAVE) {
        double v;
        if (value(t, v)) {
            const double q = v / tot;
            hh -= q * log2(q);
        }
    }
    return wave_sum(hh);
}

// whether the reference's S of the row is NaN: some key's own term is (own_term_is_nan)
template <class V>
__device__ __forceinline__ bool row_own_nan(int n, double tot, V value) {
    bool nan_key = false;
    for (int t = lane_id(); t < n; t += WAVE) {
        double v;
        if (value(t, v)) nan_key |= own_term_is_nan(v, tot);
    }
    return __ballot(nan_key) != 0ull;
}

// The reference's epilogue over the integer counts cnt[p.n] of one row, in one wave (k_user_entropy_c, k_window_entropy_c; P is
// the kernel's parameter block): samples N = histogram total, h -= (v / N) * (log2 v - log2 N) in lane order, the normaliser
// log2(n) if full_norm or N > norm_n, else log2(N) (entropy_utils.py:201-206; one sample gives the reference's 0 / 0), NaN and
// status[1] += 1 for an empty row.  k_spatial_u_lds's operations (log2 taken directly where that kernel reads its log2 table:
// the same ocml values).  Writes ent[row], weights[row][.] and samples[row].
template <class P>
__device__ __forceinline__ void count_row_entropy(const unsigned* cnt, const P& p, long row) {
    const int lane = lane_id();
    int np = 0;
    for (int t = lane; t < p.n; t += WAVE) np += (int)cnt[t];
    np = wave_sum(np);
    const double tw = (double)np, lgn = np ? log2(tw) : 0.0, inv_tw = 1.0 / tw;
    double h = 0.0;
    for (int t = lane; t < p.n; t += WAVE) {
        const unsigned v = cnt[t];
        if (v) h -= ((double)v * inv_tw) * (log2((double)v) - lgn);
        if (p.weights) __builtin_nontemporal_store((double)v, p.weights + row * (long)p.n + t);
    }
    h = wave_sum(h);
    if (lane == 0) {
        double hmax = p.hmax;
        if (!(tw > (double)p.norm_n) && !p.full_norm) hmax = -tw * (1.0 / tw) * -lgn;
        double e = h / hmax;
        if (np == 0) {
            e = __builtin_nan("");
            if (p.status) atomicAdd(&p.status[1], 1);
        }
        p.ent[row] = e;
        if (p.samples) p.samples[row] = np;
    }
}

}  // namespace vet
