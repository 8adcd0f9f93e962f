"""Time of the per-viewer transition entropy (vet_user_transition_entropy) at BASELINE config 5's shape (512 users x 10 000
frames, [200]) in three row shapes —
  window 20, stride 1     a 2-second window every frame: 9 980 rows per viewer
  window 20, stride 20    disjoint 2-second segments: 499 rows per viewer
  whole video             window = T - 1: one row per viewer
— each three ways, alternating in the same run:
  call            the call as it ships (rows of up to 64 pairs: k_user_transition_wave, longer ones: k_user_transition)
  call_hash       the same call under vet_test_user_transition_hash (k_user_transition's 64-thread hash shape for the short rows;
                  for the whole video both are the same kernel)
  baseline        what had to be done without the call: one vet_transition_entropy_windowed call per viewer on that viewer's
                  one-user video (the [U][T] transposed copy is made once and not charged to it).
Inputs resident, hipEvents on the launch stream after a warm-up; per side the median and the min..max spread of REPS timings (a
baseline timing is the U calls together).  Also recorded: the call's per-kernel times from the engine's profile scopes
(k_spatial = k_user_dirs, k_transition = stage 2) and the largest relative difference of the three results.
usage: python tools/user_transition_timing.py [out.json]      (default: profiles/user/user_transition_timing.json)"""
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

U, T, TCS = 512, 10000, [200]
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


def max_rel(a, b):
    ok = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300))) if ok.any() else 0.0


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    mu_h, mv_h = bench.synth_video(U, T, 1234, 0)
    mu = torch.from_numpy(mu_h).to(dev); mv = torch.from_numpy(mv_h).to(dev)
    mu_t, mv_t = mu.t().contiguous(), mv.t().contiguous()              # [U][T]: row u is viewer u's one-user video
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(tc) for tc in TCS], 120.0, 2.0, True, 100, 200)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    record = {"tool": "tools/user_transition_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "users": U, "frames": T, "tile_counts": TCS,
              "timing": "hipEvents on the launch stream after WARMUP calls (tables built, workspace grown); the call, the call under "
                        "the test switch and the U-call baseline alternate in the same run; median and min..max of REPS timings",
              "runs": []}
    for label, window, stride in (("w20_s1", 20, 1), ("w20_s20", 20, 20), ("whole_video", T - 1, 1)):
        R = (T - 1 - window) // stride + 1
        ent = {k: torch.empty(U * R, dtype=torch.float64, device=dev) for k in ("call", "call_hash", "baseline")}

        def call(key="call"):
            plan.transition_per_user_device(mu.data_ptr(), mv.data_ptr(), U, T, window, stride, ent[key].data_ptr(),
                                            d_status=st.data_ptr(), stream=stream.cuda_stream)

        def call_hash():
            eng.test_user_transition_hash(True)
            try:
                call("call_hash")
            finally:
                eng.test_user_transition_hash(False)

        def baseline():
            e = ent["baseline"].data_ptr()
            for u in range(U):
                plan.transition_windowed_device(mu_t.data_ptr() + u * T * 8, mv_t.data_ptr() + u * T * 8, 1, T, window, stride,
                                                e + u * R * 8, d_status=st.data_ptr(), stream=stream.cuda_stream)
        sides = (("call", call), ("call_hash", call_hash), ("baseline", baseline))
        for _ in range(WARMUP):
            for _, fn in sides:
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k, _ in sides}
        for _ in range(REPS):
            for k, fn in sides:
                ms[k].append(timed(stream, fn))
        eng.profile_enable(True); eng.profile_reset()
        call()
        eng.synchronize(); torch.cuda.synchronize()
        kern = {k: round(eng.profile_get(k)[0], 4) for k in ("k_spatial", "k_transition", "k_finalize")}
        eng.profile_enable(False)
        res = {k: v.cpu().numpy() for k, v in ent.items()}
        run = {"case": label, "window": window, "stride": stride, "rows": U * R,
               "stage2_kernel": "k_user_transition_wave" if window <= 64 else "k_user_transition",
               "call": stats(ms["call"]), "call_hash": stats(ms["call_hash"]), "baseline_u_windowed_calls": stats(ms["baseline"]),
               "call_kernels_ms": {"stage1_k_user_dirs": kern["k_spatial"], "stage2": kern["k_transition"], "mean": kern["k_finalize"]},
               "nan_rows": int(np.isnan(res["call"]).sum()),
               "max_rel_diff_call_vs_hash": max_rel(res["call"], res["call_hash"]),
               "max_rel_diff_call_vs_baseline": max_rel(res["call"], res["baseline"])}
        run["speedup_vs_hash_median"] = round(run["call_hash"]["median_ms"] / run["call"]["median_ms"], 3)
        run["speedup_vs_baseline_median"] = round(run["baseline_u_windowed_calls"]["median_ms"] / run["call"]["median_ms"], 3)
        record["runs"].append(run)
        print(json.dumps(run), flush=True)
    plan.close()
    record["device"] = torch.cuda.get_device_name(0)
    record["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "user", "user_transition_timing.json"))
