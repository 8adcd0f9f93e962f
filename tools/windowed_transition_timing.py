"""Time of the windowed (pooled) transition entropy (vet_transition_entropy_windowed) against the capability it replaces: the
per-pair call (vet_transition_entropy) over the MATERIALISED device-resident [2R][window * U] input — row 2r holds frames
f0 .. f0 + w - 1 side by side, row 2r + 1 frames f0 + 1 .. f0 + w, f0 = r * stride — of which the even output rows are kept;
the materialisation is timed separately and not charged to the baseline.  Inputs resident, hipEvents on the launch stream after
a warm-up, the two sides ALTERNATING in the same run; per side the median and the min..max spread of REPS single calls.
Shapes: config 5 (512 users x 10 000 frames, [200]) at window 20, stride 20 / 5 / 1, and for the small-window regime config 2
(64 x 3 000, [50, 100, 200]) at the same.  Where the materialised input would exceed MAX_BASELINE_BYTES the baseline runs over
the first rows that fit and is scaled to R rows (recorded as such).  Also: the new call's per-kernel times from the engine's
profile scopes (stage 1 = k_spatial: k_window_tiles; stage 2 = k_transition: k_window_transition; k_finalize: the mean over
the lattices) and the pooled pair-samples per second.
usage: python tools/windowed_transition_timing.py [out.json]      (default: profiles/windowed/windowed_transition_timing.json)"""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'viewport-entropy-toolkit_amd'))
import numpy as np
import torch
from viewport_entropy_toolkit import _native, _quantiser
import bench

SHAPES = [("config5", 512, 10000, [200], (20, 5, 1)), ("config2", 64, 3000, [50, 100, 200], (20, 5, 1))]
WINDOW = 20
WARMUP, REPS = 2, 11
MAX_BASELINE_BYTES = 6 << 30


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms, scale=1.0):
    return {"median_ms": round(float(np.median(ms)) * scale, 4), "min_ms": round(min(ms) * scale, 4), "max_ms": round(max(ms) * scale, 4)}


def materialise(x, window, stride, rows):
    """[T][U] -> [2 rows][window * U]: rows 2r / 2r + 1 = frames f0 .. / f0 + 1 .., pair-major then user order"""
    U = x.shape[1]
    win = x.unfold(0, window, 1).permute(0, 2, 1).reshape(-1, window * U)         # [T - w + 1][w * U], a view chain
    f0 = torch.arange(rows, device=x.device) * stride
    return win[torch.stack([f0, f0 + 1], dim=1).reshape(-1)].contiguous()


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    record = {"tool": "tools/windowed_transition_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP,
              "reps": REPS, "window": WINDOW,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls; windowed and baseline alternate "
                        "in the same run; median and min..max of REPS calls; materialisation not timed into the baseline",
              "shapes": []}
    for name, U, T, tcs, strides in SHAPES:
        mu_h, mv_h = bench.synth_video(U, T, 1234, 0)
        mu = torch.from_numpy(mu_h).to(dev); mv = torch.from_numpy(mv_h).to(dev)
        plan = _native.Plan(eng, [_quantiser.lattice_xyz(tc) for tc in tcs], 120.0, 2.0, True, 100, 200)
        st = torch.zeros(2, dtype=torch.int32, device=dev)
        shape = {"workload": name, "users": U, "frames": T, "tile_counts": tcs, "runs": []}
        for stride in strides:
            window = WINDOW
            R = (T - 1 - window) // stride + 1
            rows_b = int(min(R, MAX_BASELINE_BYTES // (2 * 2 * window * U * 8)))
            ent_w = torch.empty(R, dtype=torch.float64, device=dev)
            ent_b = torch.empty(2 * rows_b - 1, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mu_m, mv_m = materialise(mu, window, stride, rows_b), materialise(mv, window, stride, rows_b)
            torch.cuda.synchronize()
            gather_ms = (time.perf_counter() - t0) * 1e3

            def windowed():
                plan.transition_windowed_device(mu.data_ptr(), mv.data_ptr(), U, T, window, stride, ent_w.data_ptr(),
                                                d_status=st.data_ptr(), stream=stream.cuda_stream)

            def baseline():
                plan.transition_device(mu_m.data_ptr(), mv_m.data_ptr(), window * U, 2 * rows_b, ent_b.data_ptr(),
                                       d_status=st.data_ptr(), stream=stream.cuda_stream)
            for _ in range(WARMUP):
                windowed(); baseline()
            torch.cuda.synchronize()
            ms_w, ms_b = [], []
            for _ in range(REPS):
                ms_w.append(timed(stream, windowed))
                ms_b.append(timed(stream, baseline))
            eng.profile_enable(True); eng.profile_reset()
            windowed()
            eng.synchronize(); torch.cuda.synchronize()
            kern = {k: round(eng.profile_get(k)[0], 4) for k in ("k_spatial", "k_transition", "k_finalize")}
            eng.profile_enable(False)
            a, b = ent_w.cpu().numpy()[:rows_b], ent_b.cpu().numpy()[::2]
            ok = np.isfinite(a) & np.isfinite(b) & (b != 0)
            w_s, b_s = stats(ms_w), stats(ms_b, R / rows_b)
            run = {"stride": stride, "window": window, "rows": R, "windowed": w_s, "baseline_materialised": b_s,
                   "baseline_rows_run": rows_b, "baseline_scaled_to_all_rows": bool(rows_b < R),
                   "materialise_ms_not_charged": round(gather_ms, 3), "materialised_bytes": int(mu_m.numel() * 16),
                   "windowed_kernels_ms": {"stage1_k_window_tiles": kern["k_spatial"], "stage2_k_window_transition": kern["k_transition"],
                                           "mean_over_lattices_k_finalize": kern["k_finalize"]},
                   "pooled_pair_samples_per_s": round(R * window * U * len(tcs) / (w_s["median_ms"] * 1e-3), 1),
                   "speedup_median": round(b_s["median_ms"] / w_s["median_ms"], 3),
                   "windowed_median_below_baseline_min": bool(w_s["median_ms"] < b_s["min_ms"]),
                   "faster_by_more_than_baseline_spread": bool(b_s["min_ms"] - w_s["median_ms"] > b_s["max_ms"] - b_s["min_ms"]),
                   "max_rel_diff_vs_baseline": float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) if ok.any() else 0.0}
            del mu_m, mv_m
            shape["runs"].append(run)
            print(json.dumps({"workload": name, **run}), flush=True)
        record["shapes"].append(shape)
        plan.close()
        del mu, mv
        torch.cuda.empty_cache()
    record["device"] = torch.cuda.get_device_name(0)
    record["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "windowed", "windowed_transition_timing.json"))
