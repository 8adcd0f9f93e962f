"""Time of the per-viewer spatial entropy (vet_user_entropy) at BASELINE config 3's shape (1024 users x 30 000 frames, [500],
weighted) against what had to be done without it: the per-frame call of an fp64 plan (same arithmetic) on TRANSPOSED samples,
frames as "users" —
  whole video          window = T            against the per-frame call over [U][T]                (one "frame" per viewer)
  disjoint segments    window = stride = 20  against the per-frame call over the materialised [U * R][20] input.
Inputs resident, hipEvents on the launch stream after a warm-up, the two sides alternating in the same run; per side the median
and the min..max spread of REPS single calls.  The transposed copies are made once and not charged to the baseline.  Where the
per-frame kernels refuse a shape the refusal is recorded.  Also recorded: the call's per-kernel times from the engine's profile
scopes (k_spatial = k_user_dirs, k_weights = k_user_entropy_w, k_finalize = the rest) and k_user_dirs against a device-to-device
copy that moves the same bytes (16 B read + 4 B written per sample); "k_user_dirs_slower_than_2x_copy" says whether the
transpose needs another look.
usage: python tools/user_entropy_timing.py [out.json]      (default: profiles/user/user_entropy_timing.json)"""
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

U, T, TCS = 1024, 30000, [500]
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


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    mu_h, mv_h = bench.synth_video(U, T, 1234, 0)
    mu = torch.from_numpy(mu_h).to(dev); mv = torch.from_numpy(mv_h).to(dev)
    mu_t, mv_t = mu.t().contiguous(), mv.t().contiguous()              # [U][T]: what the baseline needs, not charged to it
    lattices = [_quantiser.lattice_xyz(tc) for tc in TCS]
    plan = _native.Plan(eng, lattices, 120.0, 2.0, True, 100, 200)
    base = _native.Plan(eng, lattices, 120.0, 2.0, True, 100, 200)
    base.set_fp64(True)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    record = {"tool": "tools/user_entropy_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "users": U, "frames": T, "tile_counts": TCS,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (tables built, workspace grown); "
                        "per-user call and baseline alternate in the same run; median and min..max of REPS calls", "runs": []}
    for label, window, stride in (("whole_video", T, 1), ("segments_w20_s20", 20, 20)):
        R = (T - window) // stride + 1
        ent_u = torch.empty(U * R, dtype=torch.float64, device=dev)
        ent_b = torch.empty(U * R, dtype=torch.float64, device=dev)

        def per_user():
            plan.spatial_per_user_device(mu.data_ptr(), mv.data_ptr(), U, T, window, stride, ent_u.data_ptr(),
                                         d_status=st.data_ptr(), stream=stream.cuda_stream)

        def baseline():                                                # rows of `window` samples: [U * R][window]
            base.spatial_device(mu_t.data_ptr(), mv_t.data_ptr(), window, U * R, ent_b.data_ptr(), d_status=st.data_ptr(),
                                stream=stream.cuda_stream)
        run = {"case": label, "window": window, "stride": stride, "rows": U * R}
        for _ in range(WARMUP):
            per_user()
        torch.cuda.synchronize()
        refused = None
        try:
            for _ in range(WARMUP):
                baseline()
            torch.cuda.synchronize()
        except _native.NativeError as e:
            refused = str(e)
        ms_u, ms_b = [], []
        for _ in range(REPS):
            ms_u.append(timed(stream, per_user))
            if refused is None:
                ms_b.append(timed(stream, baseline))
        eng.profile_enable(True); eng.profile_reset()
        per_user()
        eng.synchronize(); torch.cuda.synchronize()
        kern = {k: round(eng.profile_get(k)[0], 4) for k in ("k_spatial", "k_weights", "k_finalize")}
        eng.profile_enable(False)
        run.update({"per_user": stats(ms_u),
                    "per_user_kernels_ms": {"stage1_k_user_dirs": kern["k_spatial"], "stage2_k_user_entropy_w": kern["k_weights"],
                                            "stage2_counts_and_mean": kern["k_finalize"]}})
        if refused is None:
            a, b = ent_u.cpu().numpy(), ent_b.cpu().numpy()
            ok = np.isfinite(a) & np.isfinite(b)
            b_s = stats(ms_b)
            run.update({"baseline_transposed_per_frame_fp64": b_s,
                        "baseline_formulation": [base.last_formulation(k) for k in range(len(TCS))],
                        "speedup_median": round(b_s["median_ms"] / run["per_user"]["median_ms"], 3),
                        "max_rel_diff_vs_baseline": float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) if ok.any() else 0.0})
        else:
            run["baseline_refused"] = refused
        record["runs"].append(run)
        print(json.dumps(run), flush=True)
    # k_user_dirs against a device-to-device copy of the same bytes: 20 B per sample = a copy of 10 B per sample
    src = torch.empty(U * T * 10, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    with torch.cuda.stream(stream):
        dst.copy_(src)
        torch.cuda.synchronize()
        copy_ms = [timed(stream, lambda: dst.copy_(src)) for _ in range(REPS)]
    dirs_ms = record["runs"][0]["per_user_kernels_ms"]["stage1_k_user_dirs"]
    record["k_user_dirs_vs_copy"] = {"bytes_moved": U * T * 20, "k_user_dirs_ms": dirs_ms, "d2d_copy_same_bytes": stats(copy_ms),
                                     "ratio": round(dirs_ms / float(np.median(copy_ms)), 3),
                                     "k_user_dirs_slower_than_2x_copy": bool(dirs_ms > 2.0 * float(np.median(copy_ms)))}
    print(json.dumps(record["k_user_dirs_vs_copy"]), flush=True)
    plan.close(); base.close()
    record["device"] = torch.cuda.get_device_name(0)
    record["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "user", "user_entropy_timing.json"))
