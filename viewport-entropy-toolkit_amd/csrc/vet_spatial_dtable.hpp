// vet_spatial_dtable.hpp — k_spatial_dtable: FoV-weighted spatial entropy in FP64 from start to end ('dtable')
// Part of the gfx950 device code of the viewport -> tile -> entropy path (see vet_kernels.hpp for the map).
// Reference citations are relative to /root/reference/src/viewport_entropy_toolkit/.
#pragma once
#include "vet_weights_pass.hpp"

namespace vet {

// ------------------------------------------------------------------------------------------
// k_spatial_dtable — compute_spatial_entropy (entropy_utils.py:147-211) with the reference's arithmetic: exact FP64
// weights (calculate_tile_weights, :124-137; the k_wexact rows of every lattice of the launch) summed in FP64, then
// -sum q log2 q over the keys of the frame's dict.  The weights pass (k_weights_gather) with an entropy epilogue:
// one workgroup per frame, wave w takes the w-th contiguous share of the frame's users in column order and adds each
// user's row of EVERY lattice of the launch into its own LDS histograms (add_exact_rows: the same adds in the same order
// as the weights pass, so lattice 0's tile sums — and the weights output — are the weights pass's bits when NW is the
// weights pass's NW, which the host guarantees).  The alias (row | mirrored) is plan-wide: read once per sample.
// Epilogue: tile value = the waves' histograms added in wave order; a tile is a key iff it is not NO_KEY_BITS (a key
// whose weights are all 0.0 reads +0.0 and then gives q = 0 -> 0 * log2 0 = NaN, as the reference does, :194-198);
// lattice j is reduced by wave j % NW in fixed lane order + butterfly, divided by hmax_j; the launch's lattices are
// added in lattice order and divided by K (k_finalize's operations) where the launch holds every lattice of the plan.
// LDS: hist f64 [NW][n_sum] (lattice j at off[j] of every wave's share), present counts i32 [NW] (8-byte padded).
// S: 64-entry chunks of the longest row of the launch (1, 2, 4; 0 = any number).  Each lattice walks its rows with the
// variant of its own row length (chunk[j] <= S): the short rows of small lattices keep 8 users per step when a large lattice
// of the same launch needs the generic loop.  None of this changes the sums (users in order per tile for every variant).
// ------------------------------------------------------------------------------------------
struct DtableParams {
    SampleSrc src;
    int U, T;
    const uint32_t* alias;           // [n_dirs] direction -> row | mirrored << 31 (every lattice's rows use this numbering)
    const uint16_t* nearest;         // [n_dirs] nearest tile of lattice 0 (for assign)
    int K;                           // lattices of this launch
    int n_sum;                       // tiles of the launch's lattices: one wave's histogram
    int off[MAX_LATTICES];           // lattice j's tile 0 in a wave's histogram
    double hmax[MAX_LATTICES];
    int chunk[MAX_LATTICES];         // row-walk variant of lattice j: 1, 2, 4 (64-entry chunks of its longest row), 0 = generic
    ExactRows lat[MAX_LATTICES];
    double* entropy;                 // [T] mean over the launch's lattices, or null
    double* ent_k;                   // [K][T] per-lattice values (row j = lattice j of the launch), or null
    int32_t* assign;                 // [T*U] nearest tile of lattice 0, -1 absent, or null
    double* weights;                 // [T*n_0] tile weight sums of lattice j = 0 (the launch starts at lattice 0), or null
    int32_t* present;                // [T] or null
    int32_t* status;                 // [2] or null: {non-zero iff a sample is outside [0,1], frames without a user}
};

__host__ __device__ constexpr size_t dtable_lds_bytes(int NW, int n_sum) {
    return (size_t)NW * n_sum * 8 + (((size_t)NW * 4 + 7) & ~(size_t)7);
}

template <bool FROM_IDS, int S>
__global__ __launch_bounds__(256) void k_spatial_dtable(const DtableParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* hist = (double*)smem;                                  // [NW][n_sum]
    const int NW = blockDim.x >> 6, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    int* cnt_w = (int*)(hist + (size_t)NW * p.n_sum);              // [NW] present users per wave
    const long f = blockIdx.x;
    double* h = hist + (size_t)wv * p.n_sum;
    for (int t = lane; t < p.n_sum; t += WAVE) ((unsigned long long*)h)[t] = NO_KEY_BITS;
    const int per = (p.U + NW - 1) / NW;
    const int u_begin = wv * per, u_end = min(p.U, u_begin + per);
    bool bad = false;
    int np = 0;
    for (int u0 = u_begin; u0 < u_end; u0 += WAVE) {
        const int u = u0 + lane;
        const long idx = f * (long)p.U + u;
        const int id = u < u_end ? sample_dir<FROM_IDS>(p.src, idx, bad) : -1;
        const uint32_t a = id >= 0 ? p.alias[id] : 0u;
        const int row = (int)(a & 0x7FFFFFFFu), mir = (int)(a >> 31), cnt = min(WAVE, u_end - u0);
        for (int j = 0; j < p.K; ++j) {
            // only the variants up to the launch's S are compiled into this instance (the conditions fold)
            const int sj = p.chunk[j];
            if (S == 1 || sj == 1) add_exact_rows<1>(h + p.off[j], p.lat[j], row, mir, id >= 0, cnt);
            else if (S == 2 || sj == 2) add_exact_rows<2>(h + p.off[j], p.lat[j], row, mir, id >= 0, cnt);
            else if (S == 4 || sj == 4) add_exact_rows<4>(h + p.off[j], p.lat[j], row, mir, id >= 0, cnt);
            else add_exact_rows<0>(h + p.off[j], p.lat[j], row, mir, id >= 0, cnt);
        }
        if (p.assign && u < u_end) __builtin_nontemporal_store(id >= 0 ? (int)p.nearest[id] : -1, p.assign + idx);
        np += id >= 0 ? 1 : 0;
    }
    np = wave_sum(np);
    if (lane == 0) cnt_w[wv] = np;
    __syncthreads();
    // tile values, wave order, into wave 0's share (every slot is read and written by one thread only)
    for (int t = tid; t < p.n_sum; t += blockDim.x) {
        const double v = waves_in_order(hist, NW, p.n_sum, t);
        hist[t] = v;
        if (p.weights && t < p.lat[0].n) __builtin_nontemporal_store(weights_out(v), p.weights + f * (long)p.lat[0].n + t);
    }
    int n_present = 0;
    for (int w2 = 0; w2 < NW; ++w2) n_present += cnt_w[w2];
    __syncthreads();
    for (int j = wv; j < p.K; j += NW) {
        double* hr = hist + p.off[j];
        const int n = p.lat[j].n;
        double tot = 0.0;
        for (int t = lane; t < n; t += WAVE) {
            const double v = hr[t];
            if ((unsigned long long)__double_as_longlong(v) != NO_KEY_BITS) tot += v;
        }
        tot = wave_sum(tot);
        double hh = 0.0;
        for (int t = lane; t < n; t += WAVE) {
            const double v = hr[t];
            if ((unsigned long long)__double_as_longlong(v) != NO_KEY_BITS) {
                const double q = v / tot;
                hh -= q * log2(q);
            }
        }
        hh = wave_sum(hh);
        if (lane == 0) {
            const double e = n_present == 0 ? __builtin_nan("") : hh / p.hmax[j];
            hr[0] = e;                                             // this wave has read lattice j's values (wave_sum)
            if (p.ent_k) p.ent_k[(long)j * p.T + f] = e;
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (p.entropy) {
            double s = 0.0;
            for (int j = 0; j < p.K; ++j) s += hist[p.off[j]];
            p.entropy[f] = s / (double)p.K;
        }
        if (p.present) p.present[f] = n_present;
        if (p.status && n_present == 0) atomicAdd(&p.status[1], 1);
    }
    if (p.status) {
        const unsigned long long anybad = __ballot(bad);
        if (anybad && lane == 0) atomicAdd(&p.status[0], (int)__popcll(anybad));
    }
}

}  // namespace vet
