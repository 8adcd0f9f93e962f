"""Time of the windowed Markov transition statistics (vet_transition_markov), one-lattice plans:
  config 5's shape (512 viewers x 10 000 frames, [200]): the whole video, window = stride = 20, and window 20 at stride 1, each at
      lag 1 and lag 10;
  config 3's shape (1024 x 30 000, [500]): window = stride = 20 and the whole video, lag 1.
Per shape the device call alone (inputs resident, hipEvents on the launch stream), without and with the matrix output, its
per-kernel split from the engine's profile scopes (stage 1 k_window_tiles = k_spatial; k_markov_rows or k_markov_count with the
zeroing of the matrices = k_transition; k_markov_cells = k_wtab), and today's route to the same numbers alternating with the new
call in the same run — existing calls only, so it is the same code before and after this call existed:
  today   vet_transition_entropy with the per-pair tile pairs resident (the reference returns them for lattice 0 only, hence the
          one-lattice plans), then torch on the device: the keys p * n + c, a scatter_add into [rows][n^2] in chunks of rows under
          256 MB, and the xlogy sums.  At lag > 1 the source is pair f's first tile and the destination pair f + lag - 1's second
          tile: the same samples as long as every viewer is present in every frame, which holds for the synthetic video.
After a warm-up; per side the median and the min..max spread of REPS single calls.  Nothing gates on a speed ratio: the JSON holds
the numbers, also where the new call does not win.  Also recorded: whether the two routes agree (samples and matrix exactly, the
statistics to 1e-12).
usage: python tools/markov_timing.py [out.json]      (default: profiles/markov/markov_timing.json)"""
import json
import math
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'viewport-entropy-toolkit_amd'))
import numpy as np
import torch
from viewport_entropy_toolkit import _native, _quantiser
import bench

VW, VH = 100, 200
WARMUP, REPS = 1, 5
CHUNK_BYTES = 256 << 20
# (workload, users, frames, tile count, window (None = whole video), stride, lag)
SHAPES = [("config5_shape", 512, 10000, 200, None, 1, 1), ("config5_shape", 512, 10000, 200, None, 1, 10),
          ("config5_shape", 512, 10000, 200, 20, 20, 1), ("config5_shape", 512, 10000, 200, 20, 20, 10),
          ("config5_shape", 512, 10000, 200, 20, 1, 1), ("config5_shape", 512, 10000, 200, 20, 1, 10),
          ("config3", 1024, 30000, 500, 20, 20, 1), ("config3", 1024, 30000, 500, None, 1, 1)]


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def f(k):
    """k log2 k on a float64 tensor of counts"""
    return torch.xlogy(k, k) / math.log(2.0)


def run_shape(eng, dev, stream, name, U, T, tc, window, stride, lag, video):
    mu = torch.from_numpy(video[0]).to(dev); mv = torch.from_numpy(video[1]).to(dev)
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(tc)], 120.0, 2.0, True, VW, VH)
    n = plan.n_tiles[0]
    window = T - lag if window is None else window
    R = (T - lag - window) // stride + 1
    with_matrix = R * n * n < 2**31
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.empty((5, R), dtype=torch.float64, device=dev)
    samples = torch.empty(R, dtype=torch.int32, device=dev)
    matrix = torch.empty((R, n, n), dtype=torch.int32, device=dev) if with_matrix else None
    ent = torch.empty(T - 1, dtype=torch.float64, device=dev)
    pairs = torch.empty((T - 1, U, 2), dtype=torch.int32, device=dev)
    t_out = torch.empty((5, R), dtype=torch.float64, device=dev)
    t_samples = torch.empty(R, dtype=torch.int64, device=dev)
    t_matrix = torch.empty((R, n * n), dtype=torch.int32, device=dev) if with_matrix else None
    rows_per_chunk = max(1, min(R, CHUNK_BYTES // (n * n * 4)))

    def call(want_matrix=False):
        plan.transition_markov_device(mu.data_ptr(), mv.data_ptr(), U, T, window, stride, lag, out.data_ptr(),
                                      d_matrix=matrix.data_ptr() if want_matrix else 0, d_samples=samples.data_ptr(),
                                      d_status=st.data_ptr(), stream=stream.cuda_stream)

    def today():
        plan.transition_device(mu.data_ptr(), mv.data_ptr(), U, T, ent.data_ptr(), d_pairs=pairs.data_ptr(), d_status=st.data_ptr(),
                               stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            P = T - lag
            p, c = pairs[:P, :, 0].long(), pairs[lag - 1:lag - 1 + P, :, 1].long()
            ok = (p >= 0) & (c >= 0)
            keys = torch.where(ok, p * n + c, torch.zeros_like(p))
            keys_w, ok_w = keys.unfold(0, window, stride), ok.unfold(0, window, stride)        # [R][U][window] views
            for r0 in range(0, R, rows_per_chunk):
                r1 = min(R, r0 + rows_per_chunk)
                M = torch.zeros((r1 - r0, n * n), dtype=torch.int32, device=dev)
                M.scatter_add_(1, keys_w[r0:r1].reshape(r1 - r0, -1), ok_w[r0:r1].reshape(r1 - r0, -1).to(torch.int32))
                if t_matrix is not None:
                    t_matrix[r0:r1] = M
                M3 = M.view(r1 - r0, n, n).double()
                n_p, m_c = M3.sum(dim=2), M3.sum(dim=1)
                N = n_p.sum(dim=1)
                several = (M3 > 0).sum(dim=2) >= 2
                A = (f(n_p) * several).sum(dim=1)
                B = (f(M3) * several[:, :, None]).sum(dim=(1, 2))
                rate = (A - B) / N
                dest = torch.log2(N) - f(m_c).sum(dim=1) / N
                t_out[0, r0:r1] = rate
                t_out[1, r0:r1] = torch.log2(N) - f(n_p).sum(dim=1) / N
                t_out[2, r0:r1] = dest
                t_out[3, r0:r1] = dest - rate
                t_out[4, r0:r1] = torch.diagonal(M3, dim1=1, dim2=2).sum(dim=1) / N
                t_samples[r0:r1] = N.long()

    run = {"workload": name, "users": U, "frames": T, "tile_count": tc, "tiles": n, "window": window, "stride": stride, "lag": lag,
           "rows": R, "candidate_samples_per_row": window * U, "shape": "lds" if window * U <= 32768 else "chunked",
           "today_rows_per_chunk": rows_per_chunk}
    for _ in range(WARMUP):
        call(); today()
        if with_matrix:
            call(True)
    torch.cuda.synchronize()
    ms_c, ms_m, ms_t = [], [], []
    for _ in range(REPS):
        ms_c.append(timed(stream, call))
        ms_t.append(timed(stream, today))
        if with_matrix:
            ms_m.append(timed(stream, lambda: call(True)))
    kernels = {}
    for label, want in (("stats_only", False),) + ((("with_matrix", True),) if with_matrix else ()):
        eng.profile_enable(True); eng.profile_reset()
        call(want)
        eng.synchronize(); torch.cuda.synchronize()
        k = {x: round(eng.profile_get(x)[0], 4) for x in ("k_spatial", "k_transition", "k_wtab", "k_finalize")}
        eng.profile_enable(False)
        kernels[label] = {"stage1_k_window_tiles": k["k_spatial"], "k_markov_rows_or_count_with_zeroing": k["k_transition"],
                          "k_markov_cells": k["k_wtab"], "k_finalize": k["k_finalize"]}
    c_s, t_s = stats(ms_c), stats(ms_t)
    a, b = out.cpu().numpy(), t_out.cpu().numpy()
    fin = ~np.isnan(a) & ~np.isnan(b)
    run.update({"device_call": c_s, "device_call_with_matrix": stats(ms_m) if with_matrix else None,
                "today_transition_pairs_plus_torch": t_s, "kernels_ms": kernels,
                "speedup_median": round(t_s["median_ms"] / c_s["median_ms"], 3),
                "speedup_median_with_matrix": round(t_s["median_ms"] / stats(ms_m)["median_ms"], 3) if with_matrix else None,
                "slower_than_today_by_more_than_its_spread": bool(c_s["median_ms"] - t_s["median_ms"] > t_s["max_ms"] - t_s["min_ms"]),
                "samples_equal_today": bool(torch.equal(samples.long(), t_samples)),
                "matrix_equal_today": bool(torch.equal(matrix.view(R, n * n), t_matrix)) if with_matrix else None,
                "nan_positions_agree_with_today": bool(np.array_equal(np.isnan(a), np.isnan(b))),
                "max_abs_diff_stats_vs_today": float(np.max(np.abs(a[fin] - b[fin]))) if fin.any() else 0.0})
    plan.close()
    del mu, mv, matrix, t_matrix, pairs
    torch.cuda.empty_cache()
    return run


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    record = {"tool": "tools/markov_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (tables built, workspace grown), the new "
                        "call, today's route and the new call with the matrix output alternating; median and min..max", "runs": []}
    videos = {}
    for name, U, T, tc, window, stride, lag in SHAPES:
        if (U, T) not in videos:
            videos[(U, T)] = bench.synth_video(U, T, 1234, 0)
        run = run_shape(eng, dev, stream, name, U, T, tc, window, stride, lag, videos[(U, T)])
        record["runs"].append(run)
        print(json.dumps(run), flush=True)
    record["device"] = torch.cuda.get_device_name(0)
    record["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f_out:
        json.dump(record, f_out, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "markov", "markov_timing.json"))
