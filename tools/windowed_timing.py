"""Time of the windowed (pooled) spatial entropy (vet_spatial_entropy_windowed) against the capability it replaces: the per-frame
call of an fp64 plan (same arithmetic) over the MATERIALISED [R][window * U] input — a reshape for stride = window, a device
gather copy otherwise (timed separately, not charged to the baseline).  Inputs resident, hipEvents on the launch stream after a
warm-up, the two sides alternating in the same run; per side the median and the min..max spread of REPS single calls.
Shapes: config 3 (1024 users x 30 000 frames, [500]) at window 20, stride 20 / 5 / 1; config 2 (64 x 3 000, [50, 100, 200]) and
a config-4-shaped video (256 x 10 000, the reference's default tile_counts) at window 20, stride 1.  Where the per-frame
kernels refuse window * U users per "frame" the refusal is recorded and the comparison uses window = 4.  Also: the per-frame
fp64 pass alone (`dtable`, the floor of stage 1) and the windowed call's per-kernel times from the engine's profile scopes
(stage 1 = k_weights + k_spatial (k_window_tiles), stage 2 = k_finalize: k_window_entropy and the mean over lattices).
usage: python tools/windowed_timing.py [out.json]      (default: profiles/windowed/windowed_timing.json)"""
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

SHAPES = [("config3", 1024, 30000, [500], (20, 5, 1)), ("config2", 64, 3000, [50, 100, 200], (1,)),
          ("config4_shape", 256, 10000, [20, 50, 100, 250, 1000], (1,))]
WINDOW, FALLBACK_WINDOW = 20, 4
WARMUP, REPS = 1, 5


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def materialise(x, window, stride):
    """[T][U] -> [R][window * U], frame-major then user order inside a row (a view when stride == window and window | T)."""
    T, U = x.shape
    if stride == window and T % window == 0:
        return x.reshape(T // window, window * U)
    return x.unfold(0, window, stride).permute(0, 2, 1).reshape(-1, window * U).contiguous()


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    record = {"tool": "tools/windowed_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (tables built, workspace grown); "
                        "windowed and baseline alternate in the same run; median and min..max of REPS calls", "shapes": []}
    for name, U, T, tcs, strides in SHAPES:
        mu_h, mv_h = bench.synth_video(U, T, 1234, 0)
        mu = torch.from_numpy(mu_h).to(dev); mv = torch.from_numpy(mv_h).to(dev)
        lattices = [_quantiser.lattice_xyz(tc) for tc in tcs]
        plan = _native.Plan(eng, lattices, 120.0, 2.0, True, 100, 200)
        base = _native.Plan(eng, lattices, 120.0, 2.0, True, 100, 200)
        base.set_fp64(True)
        st = torch.zeros(2, dtype=torch.int32, device=dev)
        ent_f = torch.empty(T, dtype=torch.float64, device=dev)

        def per_frame():
            base.spatial_device(mu.data_ptr(), mv.data_ptr(), U, T, ent_f.data_ptr(), d_status=st.data_ptr(), stream=stream.cuda_stream)
        for _ in range(WARMUP):
            per_frame()
        torch.cuda.synchronize()
        floor = [timed(stream, per_frame) for _ in range(REPS)]
        shape = {"workload": name, "users": U, "frames": T, "tile_counts": tcs,
                 "per_frame_fp64_pass": {**stats(floor), "formulation": [base.last_formulation(k) for k in range(len(tcs))]},
                 "runs": []}
        for stride in strides:
            run = {"stride": stride}
            for window in (WINDOW, FALLBACK_WINDOW):
                R = (T - window) // stride + 1
                ent_w = torch.empty(R, dtype=torch.float64, device=dev)
                ent_b = torch.empty(R, dtype=torch.float64, device=dev)

                def windowed():
                    plan.spatial_windowed_device(mu.data_ptr(), mv.data_ptr(), U, T, window, stride, ent_w.data_ptr(),
                                                 d_status=st.data_ptr(), stream=stream.cuda_stream)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mu_m, mv_m = materialise(mu, window, stride), materialise(mv, window, stride)
                torch.cuda.synchronize()
                gather_ms = (time.perf_counter() - t0) * 1e3

                def baseline():
                    base.spatial_device(mu_m.data_ptr(), mv_m.data_ptr(), window * U, R, ent_b.data_ptr(), d_status=st.data_ptr(),
                                        stream=stream.cuda_stream)
                try:
                    for _ in range(WARMUP):
                        windowed(); baseline()
                    torch.cuda.synchronize()
                except _native.NativeError as e:
                    run.setdefault("baseline_refused", []).append({"window": window, "users_per_frame": window * U, "error": str(e)})
                    del mu_m, mv_m
                    continue
                ms_w, ms_b = [], []
                for _ in range(REPS):
                    ms_w.append(timed(stream, windowed))
                    ms_b.append(timed(stream, baseline))
                eng.profile_enable(True); eng.profile_reset()
                windowed()
                eng.synchronize(); torch.cuda.synchronize()
                kern = {k: round(eng.profile_get(k)[0], 4) for k in ("k_weights", "k_spatial", "k_finalize")}
                eng.profile_enable(False)
                a, b = ent_w.cpu().numpy(), ent_b.cpu().numpy()
                ok = np.isfinite(a) & np.isfinite(b)
                w_s, b_s = stats(ms_w), stats(ms_b)
                run.update({"window": window, "rows": R, "windowed": w_s, "baseline_materialised": b_s,
                            "baseline_formulation": [base.last_formulation(k) for k in range(len(tcs))],
                            "materialise_ms_not_charged": round(gather_ms, 3), "materialised_bytes": int(mu_m.numel() * 16),
                            "windowed_kernels_ms": {"stage1_k_weights_gather": kern["k_weights"], "stage1_k_window_tiles": kern["k_spatial"],
                                                    "stage2_k_window_entropy_and_mean": kern["k_finalize"]},
                            "speedup_median": round(b_s["median_ms"] / w_s["median_ms"], 3),
                            "faster_by_more_than_baseline_spread": bool(b_s["min_ms"] - w_s["max_ms"] > b_s["max_ms"] - b_s["min_ms"]),
                            "stage2_cheaper_than_stage1": bool(kern["k_finalize"] < kern["k_weights"] + kern["k_spatial"]),
                            "max_rel_diff_vs_baseline": float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) if ok.any() else 0.0})
                del mu_m, mv_m
                break
            shape["runs"].append(run)
            print(json.dumps({"workload": name, **run}), flush=True)
        record["shapes"].append(shape)
        plan.close(); base.close()
        del mu, mv
        torch.cuda.empty_cache()
    record["device"] = torch.cuda.get_device_name(0)
    record["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "windowed", "windowed_timing.json"))
