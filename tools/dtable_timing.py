"""Time of the `dtable` formulation (vet_plan_set_fp64: exact FP64 weight rows of every lattice, FP64 histograms, one pass for
entropy + tile weights) against the default formulations, with hipEvents on the launch stream after a warm-up:
config 3 (1024 users x 30 000 frames, [500]), config 2 (64 x 3 000, [50, 100, 200]) and a config-4-shaped video with the
reference's default tile_counts.  Per run: mean ms per call, the formulation of every lattice, and the largest relative
difference of the entropy series from the default one.
usage: python tools/dtable_timing.py [out.json]      (default: profiles/dtable/dtable_timing.json)"""
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

SHAPES = [("config3", 1024, 30000, [500]), ("config2", 64, 3000, [50, 100, 200]),
          ("defaults", 256, 10000, [20, 50, 100, 250, 1000])]
# (run name, fp64, table policy, ask for the weights output)
RUNS = [("default_entropy", False, 0, False), ("default_entropy_weights", False, 0, True),
        ("fp64_entropy", True, 0, False), ("fp64_entropy_weights", True, 0, True), ("policy_m1_entropy", False, -1, False)]
WARMUP, ITERS = 2, 5


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    record = {"tool": "tools/dtable_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "iters": ITERS,
              "timing": "hipEvents around ITERS calls on the launch stream, after WARMUP calls (tables built)", "shapes": []}
    for name, U, T, tcs in SHAPES:
        mu_h, mv_h = bench.synth_video(U, T, 1234, 0)
        mu = torch.from_numpy(mu_h).to(dev); mv = torch.from_numpy(mv_h).to(dev)
        n0 = 2 * (tcs[0] // 2) + 1
        ent = torch.empty(T, dtype=torch.float64, device=dev)
        wts = torch.empty((T, n0), dtype=torch.float64, device=dev)
        st = torch.zeros(2, dtype=torch.int32, device=dev)
        shape = {"workload": name, "users": U, "frames": T, "tile_counts": tcs, "runs": []}
        ref = None
        for run, fp64, policy, want_w in RUNS:
            plan = _native.Plan(eng, [_quantiser.lattice_xyz(tc) for tc in tcs], 120.0, 2.0, True, 100, 200)
            plan.set_table_policy(policy)
            plan.set_fp64(fp64)

            def step():
                plan.spatial_device(mu.data_ptr(), mv.data_ptr(), U, T, ent.data_ptr(),
                                    d_weights=wts.data_ptr() if want_w else 0, d_status=st.data_ptr(), stream=stream.cuda_stream)
            for _ in range(WARMUP):
                step()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(ITERS):
                step()
            b.record(stream)
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / ITERS
            e = ent.cpu().numpy()
            if ref is None:
                ref = e.copy()
            ok = np.isfinite(ref) & np.isfinite(e)
            rel = float(np.max(np.abs(e[ok] - ref[ok]) / np.abs(ref[ok]))) if ok.any() else 0.0
            r = {"run": run, "fp64": fp64, "policy": policy, "weights": want_w, "ms_per_call": round(ms, 4),
                 "formulation": [plan.last_formulation(k) for k in range(len(tcs))],
                 "max_rel_diff_vs_default_entropy": rel,
                 "nan_frames": int(np.isnan(e).sum()), "nan_pattern_equal": bool(np.array_equal(np.isnan(e), np.isnan(ref)))}
            shape["runs"].append(r)
            print(json.dumps({"workload": name, **r}), flush=True)
            plan.close()
        record["shapes"].append(shape)
        del mu, mv, wts
        torch.cuda.empty_cache()
    record["device"] = torch.cuda.get_device_name(0)
    record["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dtable", "dtable_timing.json"))
