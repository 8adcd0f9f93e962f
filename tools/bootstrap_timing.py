"""Time of the bootstrap over viewers (vet_bootstrap_entropy, B = 200 replicates) at config 3's shape — 1024 viewers x 30 000
frames, [500], weighted — at window = stride = 20 (1 500 rows), window 1 (the per-frame series, 30 000 rows) and the whole video
(one row), and at config 4's shape — 256 viewers x 10 000 frames — with the reference's default tile_counts
[20, 50, 100, 250, 1000] at window = stride = 20.
Each case alternates, in the same run, the new device call with today's route to the same numbers: B calls of
vet_spatial_entropy_windowed_ids, each on the direction ids column-gathered on the device to the replicate's draw
(torch.index_select into one reused buffer; the gather is part of the route and is charged to it).
Inputs resident, hipEvents on the launch stream after a warm-up; per side the median and the min..max spread of the timed calls
(REPS, or 1 where a single call takes seconds).  There is no threshold: the record states which side is faster in each case.
Also recorded: the per-kernel times from the engine's profile scopes (k_spatial = k_user_dirs, k_weights = k_user_hist_w,
k_transition = k_bootstrap_gemm, k_finalize = k_bootstrap_counts + k_bootstrap_zero_keys + k_bootstrap_summary), the achieved FP64
FLOP/s of k_bootstrap_gemm (2 B U n flops per row and lattice over its profile time) and the largest relative difference between
the two routes' replicates.
usage: python tools/bootstrap_timing.py [out.json]      (default: profiles/bootstrap/bootstrap_timing.json)"""
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

VW, VH = 100, 200
B, SEED, CONFIDENCE = 200, 2024, 0.95
WARMUP, REPS = 1, 3
KERNELS = {"k_user_dirs": "k_spatial", "k_user_hist_w": "k_weights", "k_bootstrap_gemm": "k_transition",
           "k_bootstrap_counts_zero_keys_summary": "k_finalize"}


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "calls": len(ms)}


def direction_ids(mu, mv):
    """[T][U] i32 ids on the plan's pixel grid (-1 absent): the quantiser's truncation of mu * W, mv * H."""
    absent = torch.isnan(mu) | torch.isnan(mv)
    px, py = (torch.nan_to_num(mu) * VW).to(torch.int64), (torch.nan_to_num(mv) * VH).to(torch.int64)
    return torch.where(absent, torch.full_like(px, -1), py * (VW + 1) + px).to(torch.int32)


def draw_picks(U):
    """picks[B][U]: include/vet.h's draw in numpy uint64."""
    with np.errstate(over="ignore"):
        z = np.uint64(SEED) + (np.arange(B * U, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        return (((z >> np.uint64(32)) * np.uint64(U)) >> np.uint64(32)).astype(np.int64).reshape(B, U)


def run_case(eng, dev, stream, label, U, T, tcs, window, stride, reps):
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(tc) for tc in tcs], 120.0, 2.0, True, VW, VH)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    mu_h, mv_h = bench.synth_video(U, T, 1234, 0)
    mu = torch.from_numpy(mu_h).to(dev); mv = torch.from_numpy(mv_h).to(dev)
    ids = direction_ids(mu, mv)
    picks = torch.from_numpy(draw_picks(U)).to(dev)
    R = (T - window) // stride + 1
    summary = torch.empty((4, R), dtype=torch.float64, device=dev)
    rep = torch.empty((R, B), dtype=torch.float64, device=dev)
    valid = torch.empty(R, dtype=torch.int32, device=dev)
    base = torch.empty((B, R), dtype=torch.float64, device=dev)
    ids_b = torch.empty_like(ids)
    lib = eng.lib

    def call():
        plan.spatial_bootstrap_device(mu.data_ptr(), mv.data_ptr(), U, T, window, stride, B, SEED, CONFIDENCE, summary.data_ptr(),
                                      rep.data_ptr(), 0, valid.data_ptr(), st.data_ptr(), stream=stream.cuda_stream)

    def baseline():
        with torch.cuda.stream(stream):
            for b in range(B):
                torch.index_select(ids, 1, picks[b], out=ids_b)
                _native._check(lib, lib.vet_spatial_entropy_windowed_ids(plan.handle, ids_b.data_ptr(), U, T, window, stride,
                                                                         base[b].data_ptr(), None, None, st.data_ptr(),
                                                                         stream.cuda_stream))

    for _ in range(WARMUP):
        call(); baseline()
    torch.cuda.synchronize()
    ms_c, ms_b = [], []
    for _ in range(reps):
        ms_c.append(timed(stream, call))
        ms_b.append(timed(stream, baseline))
    eng.profile_enable(True); eng.profile_reset()
    call()
    eng.synchronize(); torch.cuda.synchronize()
    kernels = {label_: round(eng.profile_get(name)[0], 4) for label_, name in KERNELS.items()}
    eng.profile_enable(False)
    flops = 2.0 * B * U * sum(plan.n_tiles) * R
    c_s, b_s = stats(ms_c), stats(ms_b)
    a, b = rep.cpu().numpy(), base.cpu().numpy().T
    both = ~np.isnan(a) & ~np.isnan(b)
    run = {"case": label, "users": U, "frames": T, "tile_counts": tcs, "window": window, "stride": stride, "rows": R,
           "replicates": B, "bootstrap": c_s, "kernels_ms": kernels,
           "baseline_B_windowed_ids_calls_on_gathered_ids": b_s,
           "ratio_median_bootstrap_over_baseline": round(c_s["median_ms"] / b_s["median_ms"], 3),
           "bootstrap_is_faster": bool(c_s["median_ms"] < b_s["median_ms"]),
           "gemm_flop": flops, "gemm_fp64_tflops": round(flops / (kernels["k_bootstrap_gemm"] * 1e-3) / 1e12, 3),
           "nan_positions_agree_with_baseline": bool(np.array_equal(np.isnan(a), np.isnan(b))),
           "max_rel_diff_vs_baseline": float(np.max(np.abs(a[both] - b[both]) / np.abs(b[both]), initial=0.0)),
           "mean_band_width": float(np.nanmean((summary[3] - summary[2]).cpu().numpy())),
           "rows_with_all_replicates_finite": int((valid == B).sum().item())}
    print(json.dumps(run), flush=True)
    plan.close()
    return run


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    record = {"tool": "tools/bootstrap_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (tables built, workspace grown); "
                        "the call and its baseline alternate in the same run; median and min..max of the timed calls", "runs": []}
    cases = (("config3_segments_w20_s20", 1024, 30000, [500], 20, 20, REPS),
             ("config3_whole_video", 1024, 30000, [500], 30000, 1, REPS),
             ("config4_reference_default_tile_counts_w20_s20", 256, 10000, [20, 50, 100, 250, 1000], 20, 20, REPS),
             ("config3_per_frame_w1_s1", 1024, 30000, [500], 1, 1, 1))
    record["device"] = torch.cuda.get_device_name(0)
    record["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    for label, U, T, tcs, window, stride, reps in cases:
        record["runs"].append(run_case(eng, dev, stream, label, U, T, tcs, window, stride, reps))
        torch.cuda.empty_cache()
        with open(out_path, "w") as f:                 # after every case: the per-frame case runs for a while
            json.dump(record, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bootstrap", "bootstrap_timing.json"))
