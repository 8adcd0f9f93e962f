// vet_tiling.hip — a tiling drawn on the unit sphere (the reference's pyvista tiling renders,
// utilities/visualization_utils.py:306-674, as a small rasteriser with a fixed frame definition): the kernels and their
// launch logic.  The C-ABI entry points (vet_tiling_*), the cameras and the block loop live in vet_hostapi.hip.
//
//   k_tiling_chords   arc -> 50 slerp points (spherical_interpolation at np.linspace(0, 1, 50)), once per scene
//   k_tiling_splat    per (frame, chord) and (frame, centre): set the pixels' line / point flag bytes
//   k_tiling_compose  the hot path: flags + sphere disc -> RGB, a streamed store of n x H x W x 3 bytes
// The frame definition is include/vet.h's; tests/_tiling_oracle.py implements it in numpy.  All arithmetic is FP64 and the
// library builds with -ffp-contract=off, so only sin / acos may differ from numpy (in the last bit).
// Reference citations are relative to /root/reference/src/viewport_entropy_toolkit/.
#include "vet_host.hpp"
#include "vet_common.hpp"

namespace vet {

using vh::TilingCam;

constexpr int kArcPoints = 50;                                     // num_points of the reference's arcs: 49 chords each

// ------------------------------------------------------------------------------------------
// k_tiling_chords: point i of arc a (one thread each) — spherical_interpolation (data_utils.py:503-518):
//   â = a / |a|, b̂ = b / |b|, theta = arccos(clip(â . b̂, -1, 1)), t_i = i * (1 / 49) (t_49 = 1, as np.linspace),
//   P_i = (sin((1 - t_i) theta) â + sin(t_i theta) b̂) / sin(theta).
// Coincident or antipodal ends (sin(theta) == 0, or a clipped cosine of -1: sin(pi) is 1.2e-16 in FP64, and the reference's
// points there are rounding noise scaled by 1 / sin(pi)) give NaN points: the splat skips them, the arc draws nothing.
// ------------------------------------------------------------------------------------------
__global__ void k_tiling_chords(const double* __restrict__ arcs, long n_arcs, double* __restrict__ pts) {
    const long total = n_arcs * kArcPoints;
    for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < total; k += (long)gridDim.x * blockDim.x) {
        const long a = k / kArcPoints;
        const int i = (int)(k - a * kArcPoints);
        const double* e = arcs + 6 * a;
        const double la = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        const double lb = sqrt(e[3] * e[3] + e[4] * e[4] + e[5] * e[5]);
        const double ax = e[0] / la, ay = e[1] / la, az = e[2] / la;
        const double bx = e[3] / lb, by = e[4] / lb, bz = e[5] / lb;
        const double cosine = clip_unit(ax * bx + ay * by + az * bz);
        const double theta = acos(cosine), st = sin(theta);
        const double t = i == kArcPoints - 1 ? 1.0 : (double)i * (1.0 / (kArcPoints - 1));
        const double s1 = sin((1.0 - t) * theta), s2 = sin(t * theta);
        double* p = pts + 3 * k;
        if (st == 0.0 || cosine == -1.0) {
            p[0] = p[1] = p[2] = __builtin_nan("");
        } else {
            p[0] = (s1 * ax + s2 * bx) / st;
            p[1] = (s1 * ay + s2 * by) / st;
            p[2] = (s1 * az + s2 * bz) / st;
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_tiling_splat: one thread per (frame, chord) and per (frame, centre) of the block.  A pixel's flags are one uint32 of
// four bytes: 0 front-line, 1 back-line, 2 front-point, 3 back-point.  Each is set with a plain byte store of the constant
// 1: threads that cover the same pixel store the same value, so no atomics are needed and the result does not depend on
// the order (the guide: global atomics execute at the memory side).  The block's flags are cleared before, by memset.
//   project:  X(p) = W/2 + (p - F).r / s,  Y(p) = H/2 - (p - F).u / s;  pixel (row, col) has its centre at (col + .5, row + .5)
//   line:     dist(q, chord AB) <= 1: tau = clamp((q - A).(B - A) / |B - A|^2, 0, 1) (0 when A == B), front iff the
//             chord point P_i + tau (P_i+1 - P_i) has p.(-d) > 0
//   point:    |X(c) - X_q| < 5 and |Y(c) - Y_q| < 5, front iff c.(-d) > 0
// The candidate pixels of a chord are walked along its major axis: per major-axis pixel, the minor-axis pixels near the
// chord's span there (with a margin of one pixel each way beyond the exact test's), so a chord costs O(its length) even
// when the camera is close; the exact test above decides.
// ------------------------------------------------------------------------------------------
struct SplatParams {
    const double* pts;       // [n_arcs][50][3]
    const double* centres;   // [n_centres][3]
    const TilingCam* cam;    // [T]
    long n_chords, n_centres;
    long T;
    int W, H;
    uint8_t* flags;          // [T][H][W][4]
};

__device__ __forceinline__ void project(const double* p, const TilingCam& c, int W, int H, double& X, double& Y) {
    const double vx = p[0] - c.F[0], vy = p[1] - c.F[1], vz = p[2] - c.F[2];
    X = (double)W / 2.0 + (vx * c.r[0] + vy * c.r[1] + vz * c.r[2]) / c.s;
    Y = (double)H / 2.0 - (vx * c.u[0] + vy * c.u[1] + vz * c.u[2]) / c.s;
}

__device__ __forceinline__ int clamp_index(double v, int n) {       // v in [-1, n], as an int (v may be huge)
    return (int)fmin(fmax(v, -1.0), (double)n);
}

__device__ void splat_chord(const double* P0, const double* P1, const TilingCam& c, int W, int H, uint8_t* fl) {
    double Ax, Ay, Bx, By;
    project(P0, c, W, H, Ax, Ay);
    project(P1, c, W, H, Bx, By);
    if (!isfinite(Ax) || !isfinite(Ay) || !isfinite(Bx) || !isfinite(By)) return;
    const double ex = Bx - Ax, ey = By - Ay, len2 = ex * ex + ey * ey;
    const bool xmaj = fabs(ex) >= fabs(ey);
    double a0 = xmaj ? Ax : Ay, a1 = xmaj ? Bx : By, b0 = xmaj ? Ay : Ax, b1 = xmaj ? By : Bx;
    if (a1 < a0) {
        double t = a0; a0 = a1; a1 = t;
        t = b0; b0 = b1; b1 = t;
    }
    const int nmaj = xmaj ? W : H, nmin = xmaj ? H : W;
    const double slope = a1 > a0 ? (b1 - b0) / (a1 - a0) : 0.0;
    const int m_lo = max(clamp_index(floor(a0 - 2.5), nmaj), 0), m_hi = min(clamp_index(ceil(a1 + 1.5), nmaj), nmaj - 1);
    for (int m = m_lo; m <= m_hi; ++m) {
        const double cm = (double)m + 0.5;
        const double v0 = b0 + (fmin(fmax(cm - 1.0, a0), a1) - a0) * slope;
        const double v1 = b0 + (fmin(fmax(cm + 1.0, a0), a1) - a0) * slope;
        const int n_lo = max(clamp_index(floor(fmin(v0, v1) - 2.5), nmin), 0);
        const int n_hi = min(clamp_index(ceil(fmax(v0, v1) + 1.5), nmin), nmin - 1);
        for (int n = n_lo; n <= n_hi; ++n) {
            const int row = xmaj ? n : m, col = xmaj ? m : n;
            const double qx = (double)col + 0.5, qy = (double)row + 0.5;
            double tau = len2 > 0.0 ? ((qx - Ax) * ex + (qy - Ay) * ey) / len2 : 0.0;
            tau = fmin(fmax(tau, 0.0), 1.0);
            const double dx = qx - (Ax + tau * ex), dy = qy - (Ay + tau * ey);
            if (dx * dx + dy * dy <= 1.0) {
                const double px = P0[0] + tau * (P1[0] - P0[0]), py = P0[1] + tau * (P1[1] - P0[1]),
                             pz = P0[2] + tau * (P1[2] - P0[2]);
                const double depth = px * c.nd[0] + py * c.nd[1] + pz * c.nd[2];
                fl[((long)row * W + col) * 4 + (depth > 0.0 ? 0 : 1)] = 1;
            }
        }
    }
}

__device__ void splat_point(const double* p, const TilingCam& c, int W, int H, uint8_t* fl) {
    double X, Y;
    project(p, c, W, H, X, Y);
    if (!isfinite(X) || !isfinite(Y)) return;
    const int flag = p[0] * c.nd[0] + p[1] * c.nd[1] + p[2] * c.nd[2] > 0.0 ? 2 : 3;
    const int c_lo = max(clamp_index(floor(X - 6.5), W), 0), c_hi = min(clamp_index(ceil(X + 5.5), W), W - 1);
    const int r_lo = max(clamp_index(floor(Y - 6.5), H), 0), r_hi = min(clamp_index(ceil(Y + 5.5), H), H - 1);
    for (int row = r_lo; row <= r_hi; ++row) {
        if (!(fabs(Y - ((double)row + 0.5)) < 5.0)) continue;
        for (int col = c_lo; col <= c_hi; ++col)
            if (fabs(X - ((double)col + 0.5)) < 5.0) fl[((long)row * W + col) * 4 + flag] = 1;
    }
}

__global__ __launch_bounds__(256) void k_tiling_splat(const SplatParams p) {
    const long per = p.n_chords + p.n_centres, total = p.T * per;
    const long HW = (long)p.W * p.H;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long f = i / per, j = i - f * per;
        const TilingCam c = p.cam[f];
        uint8_t* fl = p.flags + f * HW * 4;
        if (j < p.n_chords) {
            const long a = j / (kArcPoints - 1);
            const double* P0 = p.pts + 3 * (a * kArcPoints + (j - a * (kArcPoints - 1)));
            const double* P1 = P0 + 3;
            if (isfinite(P0[0]) && isfinite(P0[1]) && isfinite(P0[2]) && isfinite(P1[0]) && isfinite(P1[1]) && isfinite(P1[2]))
                splat_chord(P0, P1, c, p.W, p.H, fl);
        } else {
            const double* q = p.centres + 3 * (j - p.n_chords);
            if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2])) splat_point(q, c, p.W, p.H, fl);
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_tiling_compose: the colour of every pixel of the block from its flags and the sphere's disc
//   under = back-point ? red : back-line ? black : background
//   pixel = front-point ? red : front-line ? black : disc ? blend(under) : under
//   disc: ((X_q - X0)^2 + (Y_q - Y0)^2) s^2 <= 1;  blend(x) = floor(0.3 * 128 + 0.7 x + 0.5) per channel (host-computed)
// k_heatmap_fill's store pattern: thread i takes pixels 4i .. 4i+3 of the flat pixel space p = t * HW + q and stores their
// 12 bytes as ONE non-temporal dwordx3 (4-byte aligned whatever HW is); QUAD: HW % 4 == 0, so the four pixels share a
// frame and their flags are one 16-byte load.  The last N % 4 pixels are written byte-wise by the first threads.
// ------------------------------------------------------------------------------------------
struct ComposeParams {
    const uint32_t* flags;   // [N]
    const TilingCam* cam;    // [T]
    int W;
    long HW, N;              // pixels per frame, pixels of the block
    long step_t, step_q;     // the grid stride (4 * threads) as whole frames + pixels
    uint32_t colour[6];      // background, red, black, blend(background), blend(red), blend(black)
    uint8_t* out;            // [N][3], 4-byte aligned
};

__device__ __forceinline__ uint32_t tiling_pixel(const ComposeParams& p, uint32_t f, const TilingCam& c, long q) {
    if (f & 0x00FF0000u) return p.colour[1];
    if (f & 0x000000FFu) return p.colour[2];
    const int under = (f & 0xFF000000u) ? 1 : (f & 0x0000FF00u) ? 2 : 0;
    const int qi = (int)q, row = qi / p.W, col = qi - row * p.W;     // HW < 2^31 (vet_tiling_create)
    const double dx = ((double)col + 0.5) - c.X0, dy = ((double)row + 0.5) - c.Y0;
    return (dx * dx + dy * dy) * (c.s * c.s) <= 1.0 ? p.colour[3 + under] : p.colour[under];
}

template <bool QUAD>
__global__ __launch_bounds__(256) void k_tiling_compose(const ComposeParams p) {
    const long quads = p.N >> 2;
    long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    long t = (i << 2) / p.HW, q = (i << 2) - t * p.HW;
    const long istep = (long)gridDim.x * blockDim.x;
    for (; i < quads; i += istep) {
        uint32_t c[4];
        if (QUAD) {
            const uint4 f = *(const uint4*)(p.flags + (i << 2));
            const TilingCam& cam = p.cam[t];
            c[0] = tiling_pixel(p, f.x, cam, q); c[1] = tiling_pixel(p, f.y, cam, q + 1);
            c[2] = tiling_pixel(p, f.z, cam, q + 2); c[3] = tiling_pixel(p, f.w, cam, q + 3);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                long tk = t, qk = q + k;
                while (qk >= p.HW) { qk -= p.HW; ++tk; }
                c[k] = tiling_pixel(p, p.flags[(i << 2) + k], p.cam[tk], qk);
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
        const uint32_t c = tiling_pixel(p, p.flags[px], p.cam[tk], qk);
        uint8_t* o = p.out + 3 * px;
        o[0] = (uint8_t)c; o[1] = (uint8_t)(c >> 8); o[2] = (uint8_t)(c >> 16);
    }
}

}  // namespace vet

namespace vh {

int tiling_chords(vet_ctx* c, const double* d_arcs, long n_arcs, double* d_pts, hipStream_t s) {
    hipLaunchKernelGGL(vet::k_tiling_chords, dim3(grid_for(n_arcs * vet::kArcPoints, 256, c->n_cu)), dim3(256), 0, s, d_arcs,
                       n_arcs, d_pts);
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

int tiling_render(vet_ctx* c, const TilingGeom& g, const TilingCam* d_cam, int T, uint32_t* d_flags, uint8_t* d_rgb,
                  hipStream_t s) {
    const long HW = (long)g.W * g.H, N = HW * T;
    HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)N * 4, s));
    const long n_chords = g.n_arcs * (vet::kArcPoints - 1);
    const vet::SplatParams sp{g.d_pts, g.d_centres, d_cam, n_chords, g.n_centres, (long)T, g.W, g.H, (uint8_t*)d_flags};
    hipLaunchKernelGGL(vet::k_tiling_splat, dim3(grid_for((long)T * (n_chords + g.n_centres), 256, c->n_cu)), dim3(256), 0, s,
                       sp);
    HIP_TRY(hipGetLastError());
    const long quads = N >> 2;
    const int grid = grid_for(quads > 0 ? quads : 1, 256, c->n_cu);
    const long stride = 4L * grid * 256;
    vet::ComposeParams cp{d_flags, d_cam, g.W, HW, N, stride / HW, stride % HW, {}, d_rgb};
    for (int k = 0; k < 6; ++k) cp.colour[k] = g.colour[k];
    if (HW % 4 == 0) hipLaunchKernelGGL(vet::k_tiling_compose<true>, dim3(grid), dim3(256), 0, s, cp);
    else hipLaunchKernelGGL(vet::k_tiling_compose<false>, dim3(grid), dim3(256), 0, s, cp);
    HIP_TRY(hipGetLastError());
    return VET_OK;
}

}  // namespace vh
