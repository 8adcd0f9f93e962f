// vet_heatmap.hip — per-frame tile-attention heatmaps (the reference's tile-attention animation,
// utilities/visualization_utils.py:99-204, as an equirectangular RGB raster): the kernels and their launch logic.
// The C-ABI entry points (vet_heatmap_*) and the render pipeline of a device-resident result live in vet_hostapi.hip.
//
//   k_heatmap_map      pixel -> nearest tile of the lattice (find_nearest_tile over the pixel centre's direction)
//   k_heatmap_map_latlon  pixel -> lat/lon cell of a naive tiling (find_naive_tile_index over the pixel centre)
//   k_heatmap_palette  per frame and tile: _get_color_from_intensity(tile_weights / users present) as packed RGB
//                      (f64 spatial weights, or the i32 source-tile counts of a transition result)
//   k_heatmap_bin_palette  per frame: the lat/lon cell histogram of its samples in LDS, then its palette row (naive plans)
//   k_heatmap_fill     the hot path: RGB[t][q] = palette[t][map[q]], a streamed store of n x H x W x 3 bytes
//   k_heatmap_markers  per (frame, user): a black square centred on the user's viewport pixel
// Reference citations are relative to /root/reference/src/viewport_entropy_toolkit/.
#include "vet_host.hpp"
#include "vet_common.hpp"

namespace vet {

// ------------------------------------------------------------------------------------------
// k_heatmap_map: pixel (r, c) of a W x H equirectangular frame -> nearest tile.  The pixel centre's direction is
// Vector.from_spherical (data_types.py:204-216) in FP64 without its 6-decimal rounding, at
//   lon = (c + 0.5) / W * 360 - 180,   lat = 90 - (r + 0.5) / H * 180   (row 0 = lat +90, as pixel_to_spherical),
// normalised as vector_angle_distance does (entropy_utils.py:55-58); the tile is nearest_tile's first minimum over the
// lattice's unit centres in LDS — k_nearest_lut's arithmetic.  One thread per pixel.
// ------------------------------------------------------------------------------------------
__global__ void k_heatmap_map(const double* __restrict__ tiles, int n, int W, int H, uint16_t* __restrict__ map) {
    extern __shared__ double s_tiles[];
    for (int i = threadIdx.x; i < 3 * n; i += blockDim.x) s_tiles[i] = tiles[i];
    __syncthreads();
    const long HW = (long)W * H;
    constexpr double kRad = 3.141592653589793 / 180.0;             // np.radians: x * (pi / 180)
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < HW; q += (long)gridDim.x * blockDim.x) {
        const int r = (int)(q / W), c = (int)(q - (long)r * W);
        const double lon = ((double)c + 0.5) / (double)W * 360.0 - 180.0;
        const double lat = 90.0 - ((double)r + 0.5) / (double)H * 180.0;
        const double theta = lon * kRad, phi = (90.0 - lat) * kRad;
        const double sp = sin(phi);
        const double x = sp * cos(theta), y = sp * sin(theta), z = cos(phi);
        const double len = sqrt(x * x + y * y + z * z);
        map[q] = (uint16_t)nearest_tile(x / len, y / len, z / len, s_tiles, n);
    }
}

// ------------------------------------------------------------------------------------------
// k_heatmap_palette: PlotManager._get_color_from_intensity (utilities/visualization_utils.py:187-204) of every tile of
// every frame, in FP64 and in the reference's operation order (the library builds with -ffp-contract=off: no FMA here):
//   i = w / n (0 when no user is present), clip to [0, 1], red = i * (1 - 0.8) + 0.8, green = blue = 0.8 - i * 0.8,
//   byte = floor(v * 255 + 0.5);  packed R | G << 8 | B << 16.
// w = tile_weights[t][tile] (a non-key is +0.0, a zero-valued key -0.0: both give grey).  A NaN intensity clips to 0.
// Wt = double: spatial tile_weights.  Wt = int32_t: a transition result's srccount rows (the users counted per source tile,
// weight_per_tile, utilities/entropy_utils.py:289-292), converted exactly to double before the same arithmetic.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t colour_byte(double v) { return (uint32_t)floor(v * 255.0 + 0.5); }

// the packed colour of weight w over `users` present (the palette arithmetic of every heatmap kind)
__device__ __forceinline__ uint32_t heatmap_colour(double w, int users) {
    double v = users > 0 ? w / (double)users : 0.0;
    v = fmin(fmax(v, 0.0), 1.0);
    const double red = v * 0.19999999999999996 + 0.8;
    const double gb = 0.8 - v * 0.8;
    const uint32_t g = colour_byte(gb);
    return colour_byte(red) | g << 8 | g << 16;
}

template <typename Wt>
__global__ void k_heatmap_palette(const Wt* __restrict__ weights, const int32_t* __restrict__ present, long T, int n,
                                  uint32_t* __restrict__ pal) {
    const long total = T * (long)n;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
        pal[i] = heatmap_colour((double)weights[i], present[i / n]);
}

// ------------------------------------------------------------------------------------------
// k_heatmap_map_latlon: pixel (r, c) -> lat/lon cell, find_naive_tile_index (utilities/entropy_utils.py:362-381) of the
// pixel centre in FP64 with C truncation:
//   lon = (c + 0.5) / W * 360 - 180,   lat = 90 - (r + 0.5) / H * 180,
//   li = (int)((lon + 180) / tile_width),  lj = (int)((lat + 90) / tile_height)
// — cell li * n_lat + lj in the numbering of the naive plan's direction -> bin LUT.  The map holds the cell's SLOT
// lj * n_lon + li instead (the palette rows of lat/lon heatmaps are slot-ordered): a pixel row then reads consecutive
// palette entries, where the cell numbering would put neighbouring columns n_lat entries apart (1x1-degree cells: 724 B,
// one cache line per pixel of the fill).  vet_heatmap_read_map turns slots back into cells.  One thread per pixel.
// ------------------------------------------------------------------------------------------
__global__ void k_heatmap_map_latlon(int W, int H, double tw, double th, int n_lon, uint16_t* __restrict__ map) {
    const long HW = (long)W * H;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < HW; q += (long)gridDim.x * blockDim.x) {
        const int r = (int)(q / W), c = (int)(q - (long)r * W);
        const double lon = ((double)c + 0.5) / (double)W * 360.0 - 180.0;
        const double lat = 90.0 - ((double)r + 0.5) / (double)H * 180.0;
        map[q] = (uint16_t)((int)((lat + 90.0) / th) * n_lon + (int)((lon + 180.0) / tw));
    }
}

// ------------------------------------------------------------------------------------------
// k_heatmap_bin_palette: the palette rows of a block of frames straight from their samples, for a binned (lat/lon) plan.
// Workgroup g takes frames [g * FPW, g * FPW + FPW).  Pass 1: every sample (16 B in: mu, mv, non-temporal) goes through
// the plan's own quantiser (grid_dir) and direction -> bin LUT into the frame's LDS histogram (ds_add), and every present
// user into the frame's LDS `present` counter; a NaN is absent, a sample outside [0, 1] counts in neither.  The histogram
// and the palette rows are slot-ordered (bin li * n_lat + lj -> slot lj * n_lon + li, as k_heatmap_map_latlon).  Pass 2:
// palette[t][slot] = heatmap_colour(count, present) over the flat (frame, slot) range of the workgroup, which is
// contiguous in the [T][n] palette; zero counts take the grey of heatmap_colour(0, 0) without the FP64 division.
// PACK: two 16-bit counts per LDS word (slot b adds 1 << 16 (b & 1) to word b >> 1; exact while U <= 65535, so no carry
// reaches the neighbour): 1x1-degree cells, 65 341 bins, take 128 KiB.  !PACK: one u32 per bin, for U > 65535 on grids
// whose bins fit the LDS as u32 (the host refuses the rest).
// LDS: present u32 [FPW rounded up to 4] | cnt u32 [FPW][words] (rounded up to 4)
// ------------------------------------------------------------------------------------------
struct BinParams {
    const double* mu;      // [T][U]
    const double* mv;
    const uint16_t* lut;   // the plan's direction -> bin table of lattice 0
    int U, T, VW, VH;      // users, frames, video size (the plan's pixel grid)
    int n, words, FPW;     // bins, LDS words per frame, frames per workgroup
    int n_lat, n_lon;      // bins per lon column, per lat row
    uint32_t* pal;         // [T][n]
};

template <bool PACK>
__global__ __launch_bounds__(1024) void k_heatmap_bin_palette(const BinParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* present = (uint32_t*)smem;
    uint32_t* cnt = present + ((p.FPW + 3) & ~3);
    const long f0 = (long)blockIdx.x * p.FPW;
    const int nf = (int)min((long)p.FPW, (long)p.T - f0);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int zq = (nf * p.words + 3) >> 2;                      // 16-byte stores (the layout rounds the counts up to 4)
    for (int i = tid; i < zq; i += nt) ((uint4*)cnt)[i] = make_uint4(0u, 0u, 0u, 0u);
    for (int i = tid; i < nf; i += nt) present[i] = 0u;
    __syncthreads();
    const double* mu = p.mu + f0 * (long)p.U;
    const double* mv = p.mv + f0 * (long)p.U;
    const int total = nf * p.U;                                  // < 2^31 (host)
    for (int i = tid; i < total; i += nt) {
        bool bad = false;
        const int id = grid_dir(__builtin_nontemporal_load(mu + i), __builtin_nontemporal_load(mv + i), p.VW, p.VH, bad);
        if (id < 0) continue;
        const int fl = nf == 1 ? 0 : (int)((unsigned)i / (unsigned)p.U);
        const unsigned bin = p.lut[id], li = bin / (unsigned)p.n_lat;
        const int slot = (int)((bin - li * p.n_lat) * p.n_lon + li);
        atomicAdd(&present[fl], 1u);
        if (PACK) atomicAdd(&cnt[fl * p.words + (slot >> 1)], 1u << ((slot & 1) << 4));
        else atomicAdd(&cnt[fl * p.words + slot], 1u);
    }
    __syncthreads();
    // the workgroup's span of the palette, [f0 * n, (f0 + nf) * n): a head up to 16-byte alignment (the palette itself is
    // 16-byte aligned), 16-byte stores of 4 entries per thread, a tail
    const uint32_t grey = heatmap_colour(0.0, 0);
    uint32_t* out = p.pal + f0 * (long)p.n;
    const int span = nf * p.n;
    const int head = min((int)((4 - ((f0 * p.n) & 3)) & 3), span);
    const int body = head + ((span - head) & ~3);
    auto colour_at = [&](int fl, int b) {
        const uint32_t* row = cnt + fl * p.words;
        const uint32_t c = PACK ? (row[b >> 1] >> ((b & 1) << 4)) & 0xffffu : row[b];
        return c ? heatmap_colour((double)c, (int)present[fl]) : grey;
    };
    auto single = [&](int j) {
        const int fl = nf == 1 ? 0 : (int)((unsigned)j / (unsigned)p.n);
        out[j] = colour_at(fl, j - fl * p.n);
    };
    if (tid < head) single(tid);
    for (int j = head + 4 * tid; j < body; j += 4 * nt) {
        int fl = nf == 1 ? 0 : (int)((unsigned)j / (unsigned)p.n), b = j - fl * p.n;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = colour_at(fl, b);
            if (++b == p.n) { b = 0; ++fl; }
        }
        *(uint4*)(out + j) = make_uint4(v[0], v[1], v[2], v[3]);
    }
    if (tid < span - body) single(body + tid);
}

// ------------------------------------------------------------------------------------------
// k_heatmap_fill: RGB[p] = palette[t][map[q]] over the flat pixel space p = t * HW + q of the block's n frames.  Thread i
// takes pixels 4i .. 4i+3: its 12 bytes start at a multiple of 4 whatever HW is and leave as ONE non-temporal dwordx3
// store (the frames are streamed once and not reread; cdna_hip_programming.md, stores).  The map (HW u16, L2-resident)
// and the palette rows (n_tiles u32 per frame) are the only loads.  QUAD: HW % 4 == 0, so the four pixels share a frame
// and their map entries are one 8-byte load.  Grid-stride; (t, q) of the first quad from one division, then stepped by
// the stride's (frames, pixels).  The last N % 4 pixels of the block are written byte-wise by the first threads.
// ------------------------------------------------------------------------------------------
struct FillParams {
    const uint16_t* map;   // [HW]
    const uint32_t* pal;   // [T][n]
    int n;
    long HW, N;            // pixels per frame, pixels of the block (T * HW)
    long step_t, step_q;   // the grid stride (4 * threads) as whole frames + pixels
    uint8_t* out;          // [N][3], 4-byte aligned
};

template <bool QUAD>
__global__ __launch_bounds__(256) void k_heatmap_fill(const FillParams p) {
    const long quads = p.N >> 2;
    long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    long t = (i << 2) / p.HW, q = (i << 2) - t * p.HW;
    const long istep = (long)gridDim.x * blockDim.x;
    for (; i < quads; i += istep) {
        uint32_t c[4];
        if (QUAD) {
            const ushort4 m = *(const ushort4*)(p.map + q);
            const uint32_t* row = p.pal + t * p.n;
            c[0] = row[m.x]; c[1] = row[m.y]; c[2] = row[m.z]; c[3] = row[m.w];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                long tk = t, qk = q + k;
                while (qk >= p.HW) { qk -= p.HW; ++tk; }
                c[k] = p.pal[tk * p.n + p.map[qk]];
            }
        }
        const u32x3 v = {c[0] | c[1] << 24, c[1] >> 8 | c[2] << 16, c[2] >> 16 | c[3] << 8};
        __builtin_nontemporal_store(v, (u32x3_a4*)(p.out + 12 * i));
        t += p.step_t; q += p.step_q;
        if (q >= p.HW) { q -= p.HW; ++t; }
    }
    const int tail = (int)(p.N & 3);
    if (blockIdx.x == 0 && (int)threadIdx.x < tail) {
        const long px = (quads << 2) + threadIdx.x;
        const long tk = px / p.HW, qk = px - tk * p.HW;
        const uint32_t c = p.pal[tk * p.n + p.map[qk]];
        uint8_t* o = p.out + 3 * px;
        o[0] = (uint8_t)c; o[1] = (uint8_t)(c >> 8); o[2] = (uint8_t)(c >> 16);
    }
}

// ------------------------------------------------------------------------------------------
// k_heatmap_markers: one thread per (frame, user) of the block, after the fill on the same stream.  The viewport pixel
// is the engine's own quantiser (grid_dir: normalize_to_pixel, data_utils.py:243-261, px = int(mu * video_width)); a
// NaN sample is absent and a sample outside [0, 1] draws nothing (the run that produced the weights reported it).
//   col = min(px * W / video_width, W - 1), row = min(py * H / video_height, H - 1)   (integer division)
// A (2 radius + 1)^2 black square around (row, col): columns wrap modulo W (longitude is periodic), rows clamp to
// [0, H).  Overlapping squares write the same bytes, so the result does not depend on the order.
// ------------------------------------------------------------------------------------------
__global__ void k_heatmap_markers(const double* __restrict__ mu, const double* __restrict__ mv, int U, long T, int VW,
                                  int VH, int W, int H, int radius, uint8_t* __restrict__ out) {
    const long total = T * (long)U;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        bool bad = false;
        const int id = grid_dir(mu[i], mv[i], VW, VH, bad);
        if (id < 0) continue;
        const long f = i / U;
        const long py = id / (VW + 1), px = id - py * (VW + 1);
        const long col = min(px * W / VW, (long)W - 1), row = min(py * H / VH, (long)H - 1);
        for (long rr = max(row - radius, 0L); rr <= min(row + radius, (long)H - 1); ++rr) {
            uint8_t* line = out + (f * H + rr) * (long)W * 3;
            for (long dc = -radius; dc <= radius; ++dc) {
                long cc = (col + dc) % W;
                if (cc < 0) cc += W;
                uint8_t* o = line + 3 * cc;
                o[0] = 0; o[1] = 0; o[2] = 0;
            }
        }
    }
}

}  // namespace vet

namespace vh {

int heatmap_map(vet_ctx* c, const double* d_unit_tiles, int n, int W, int H, uint16_t* d_map, hipStream_t s) {
    const size_t lds = (size_t)n * 3 * sizeof(double);
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void*)vet::k_heatmap_map, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(vet::k_heatmap_map, dim3(grid_for((long)W * H, 256, c->n_cu)), dim3(256), lds, s, d_unit_tiles, n,
                       W, H, d_map);
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

int heatmap_map_latlon(vet_ctx* c, int tile_width, int tile_height, int W, int H, uint16_t* d_map, hipStream_t s) {
    hipLaunchKernelGGL(vet::k_heatmap_map_latlon, dim3(grid_for((long)W * H, 256, c->n_cu)), dim3(256), 0, s, W, H,
                       (double)tile_width, (double)tile_height, 360 / tile_width + 1, d_map);
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

// The fill of frames [0, T) from their palette rows, then the markers when d_mu / d_mv are given.
static int heatmap_fill(vet_ctx* c, const HeatmapGeom& g, const double* d_mu, const double* d_mv, int U, int T,
                        const uint32_t* d_pal, uint8_t* d_rgb, hipStream_t s) {
    const long HW = (long)g.W * g.H, N = HW * T;
    const long quads = N >> 2;
    const int grid = grid_for(quads > 0 ? quads : 1, 256, c->n_cu);
    const long stride = 4L * grid * 256;
    const vet::FillParams fp{g.d_map, d_pal, g.n, HW, N, stride / HW, stride % HW, d_rgb};
    if (HW % 4 == 0) hipLaunchKernelGGL(vet::k_heatmap_fill<true>, dim3(grid), dim3(256), 0, s, fp);
    else hipLaunchKernelGGL(vet::k_heatmap_fill<false>, dim3(grid), dim3(256), 0, s, fp);
    HIP_TRY(hipGetLastError());
    if (d_mu && d_mv && U > 0) {
        hipLaunchKernelGGL(vet::k_heatmap_markers, dim3(grid_for((long)T * U, 256, c->n_cu)), dim3(256), 0, s, d_mu, d_mv,
                           U, (long)T, g.VW, g.VH, g.W, g.H, g.radius, d_rgb);
        HIP_TRY(hipGetLastError());
    }
    return VET_OK;
}

template <typename Wt>
int heatmap_render(vet_ctx* c, const HeatmapGeom& g, const Wt* d_weights, const int32_t* d_present, const double* d_mu,
                   const double* d_mv, int U, int T, uint32_t* d_pal, uint8_t* d_rgb, hipStream_t s) {
    hipLaunchKernelGGL(vet::k_heatmap_palette<Wt>, dim3(grid_for((long)T * g.n, 256, c->n_cu)), dim3(256), 0, s, d_weights,
                       d_present, (long)T, g.n, d_pal);
    HIP_TRY(hipGetLastError());
    return heatmap_fill(c, g, d_mu, d_mv, U, T, d_pal, d_rgb, s);
}

BinLayout heatmap_bin_layout(int n, int U) {
    BinLayout L;
    if (U <= 0 || (long)U > (1L << 30)) return L;
    L.pack = U <= 65535;
    L.words = L.pack ? (n + 1) / 2 : n;
    const size_t frame = (size_t)L.words * 4;
    if (16 + ((frame + 15) & ~(size_t)15) > kWholeLds) return L;   // u32 counts of this many bins do not fit
    // frames per workgroup: about 4096 samples each (small U), within 32 KiB of counts so that several workgroups share
    // a CU; one frame when a frame's counts alone are larger
    long fpw = std::max(1, 4096 / U);
    fpw = std::min<long>(fpw, std::max<size_t>(1, ((size_t)32 << 10) / frame));
    fpw = std::min<long>(fpw, ((1L << 31) - 1024) / U);
    L.FPW = (int)std::max(1L, fpw);
    L.lds = (size_t)((L.FPW + 3) & ~3) * 4 + (((size_t)L.FPW * frame + 15) & ~(size_t)15);
    L.ok = true;
    return L;
}

// Frames per bin-palette + fill launch pair: at most 64 MiB of palette, so that the fill gathers a chunk's rows from the
// Infinity Cache right after k_heatmap_bin_palette wrote them.  1x1-degree cells (261 KB per frame, 535 MB for 2 048
// frames) would otherwise leave the fill gathering from HBM.  Measured on one MI355X, 2 048 frames of 1 024 users at
// 1200 x 600 (bin-palette + fill): 1.95 / 1.51 / 1.30 / 1.31 ms in chunks of 16 / 32 / 64 / 128 MiB, 2.2 ms in one
// (tools/naive_heatmap_timing.py).  Grids up to 10x10-degree cells (703 bins) run in one chunk.
int heatmap_bin_chunk(int n) { return (int)std::max<size_t>(1, ((size_t)64 << 20) / ((size_t)n * 4)); }

int heatmap_render_binned(vet_ctx* c, const HeatmapGeom& g, int n_lat, const uint16_t* d_lut, const double* d_mu,
                          const double* d_mv, int U, int T, bool markers, uint32_t* d_pal, uint8_t* d_rgb, hipStream_t s) {
    const BinLayout L = heatmap_bin_layout(g.n, U);
    if (!L.ok) return fail(VET_ERR_UNSUPPORTED, "%d users over %d cells exceed the LDS histogram of k_heatmap_bin_palette", U, g.n);
    const void* fn = L.pack ? (const void*)vet::k_heatmap_bin_palette<true> : (const void*)vet::k_heatmap_bin_palette<false>;
    if (L.lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
    const int C = heatmap_bin_chunk(g.n);
    const size_t frame = (size_t)g.W * g.H * 3;
    for (int f0 = 0; f0 < T; f0 += C) {
        const int b = std::min(C, T - f0);
        const size_t off = (size_t)f0 * U;
        const vet::BinParams bp{d_mu + off, d_mv + off, d_lut, U, b, g.VW, g.VH, g.n, L.words, L.FPW, n_lat, g.n / n_lat, d_pal};
        const dim3 grid((unsigned)((b + (long)L.FPW - 1) / L.FPW));
        if (L.pack) hipLaunchKernelGGL(vet::k_heatmap_bin_palette<true>, grid, dim3(1024), L.lds, s, bp);
        else hipLaunchKernelGGL(vet::k_heatmap_bin_palette<false>, grid, dim3(1024), L.lds, s, bp);
        HIP_TRY(hipGetLastError());
        int rc = heatmap_fill(c, g, markers ? d_mu + off : nullptr, markers ? d_mv + off : nullptr, U, b, d_pal,
                              d_rgb + (size_t)f0 * frame, s);
        if (rc) return rc;
    }
    return VET_OK;
}

template int heatmap_render<double>(vet_ctx*, const HeatmapGeom&, const double*, const int32_t*, const double*,
                                    const double*, int, int, uint32_t*, uint8_t*, hipStream_t);
template int heatmap_render<int32_t>(vet_ctx*, const HeatmapGeom&, const int32_t*, const int32_t*, const double*,
                                     const double*, int, int, uint32_t*, uint8_t*, hipStream_t);

}  // namespace vh
