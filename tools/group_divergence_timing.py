"""Time of the two-audience permutation test (vet_group_divergence) at config 3's shape — 1024 viewers x 30 000 frames, [500],
weighted, balanced groups — at window = stride = 20 (1 500 rows), window 1 (30 000 rows) and the whole video (one row), and at
config 4's shape — 256 viewers x 10 000 frames — with the reference's default tile_counts [20, 50, 100, 250, 1000] at
window = stride = 20.
Each case alternates, in the same run, the new device call with today's route to the same numbers: per labelling (the observed one
and every permutation) and lattice two calls of vet_spatial_entropy_windowed_ids with weights, each on the direction ids
column-gathered on the device to one audience (torch.index_select into a reused buffer; the gather is part of the route and is
charged to it), then the three-term combination S(A + B) - (W_A S(A) + W_B S(B)) / (W_A + W_B) in torch on the device.  The windowed
call returns lattice 0's histogram only, so today's route runs a plan of several lattices as one plan per lattice.
Today's route at 999 permutations takes minutes at these shapes (2 000 calls, 33 ms each for the whole video), so BOTH routes are
timed at P = 99 (100 labellings); the new call alone is also timed at P = 999.
Inputs resident, hipEvents on the launch stream after a warm-up; per side the median and the min..max spread of the timed calls.
Acceptance: the new route's median is not above today's route's median by more than today's route's own spread (max - min).
Also recorded: the per-kernel times from the engine's profile scopes (k_spatial = k_user_dirs, k_weights = k_user_hist_w,
k_transition = k_group_gemm, k_finalize = k_group_labels + k_bootstrap_zero_keys + k_group_samples + k_group_maxnull +
k_group_summary), the achieved FP64 FLOP/s of k_group_gemm (2 * 16 U n flops per row, lattice and block of 8 labellings over its
profile time) and the largest absolute difference between the two routes' D.
usage: python tools/group_divergence_timing.py [out.json [case ...]]      (default: profiles/group/group_divergence_timing.json,
every case)"""
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
P_BOTH, P_FULL, SEED, CONFIDENCE = 99, 999, 2025, 0.95
WARMUP, REPS = 1, 3
KERNELS = {"k_user_dirs": "k_spatial", "k_user_hist_w": "k_weights", "k_group_gemm": "k_transition",
           "k_group_labels_zero_keys_samples_maxnull_summary": "k_finalize"}


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


def bits(h, keys):
    """(S, W) of dense row histograms h[R][n] with key masks: -sum q log2 q over the keys, before the normaliser."""
    W = h.sum(dim=1)
    q = torch.where(keys, h / W[:, None], torch.ones_like(h))
    return -(q * torch.log2(q)).sum(dim=1), W


def profile_call(eng, call):
    eng.profile_enable(True); eng.profile_reset()
    call()
    eng.synchronize(); torch.cuda.synchronize()
    kernels = {label: round(eng.profile_get(name)[0], 4) for label, name in KERNELS.items()}
    eng.profile_enable(False)
    return kernels


def run_case(eng, dev, stream, label, U, T, tcs, window, stride, reps):
    lat = [_quantiser.lattice_xyz(tc) for tc in tcs]
    plan = _native.Plan(eng, lat, 120.0, 2.0, True, VW, VH)
    singles = [plan] if len(tcs) == 1 else [_native.Plan(eng, [x], 120.0, 2.0, True, VW, VH) for x in lat]
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    mu_h, mv_h = bench.synth_video(U, T, 1234, 0)
    mu = torch.from_numpy(mu_h).to(dev); mv = torch.from_numpy(mv_h).to(dev)
    ids = direction_ids(mu, mv)
    groups = (np.arange(U) % 2).astype(np.int8)                        # balanced
    labels = plan.group_labels(groups, P_BOTH, SEED)                   # [L][U], the device's own draw
    L = P_BOTH + 1
    idx = [torch.from_numpy(np.stack([np.flatnonzero(labels[l] == g) for l in range(L)])).to(dev) for g in (0, 1)]
    R = (T - window) // stride + 1
    K = len(tcs)
    lib = eng.lib

    def outputs(P):
        return (torch.empty((5, R), dtype=torch.float64, device=dev), torch.empty((R, P), dtype=torch.float64, device=dev),
                torch.empty(R, dtype=torch.int32, device=dev))

    out_both, out_full = outputs(P_BOTH), outputs(P_FULL)

    def call(P=P_BOTH, out=out_both):
        plan.spatial_group_divergence_device(mu.data_ptr(), mv.data_ptr(), U, T, window, stride, groups, P, SEED, CONFIDENCE,
                                             out[0].data_ptr(), d_null=out[1].data_ptr(), d_valid=out[2].data_ptr(),
                                             d_status=st.data_ptr(), stream=stream.cuda_stream)

    base = torch.empty((L, R), dtype=torch.float64, device=dev)
    ids_g = [torch.empty((T, idx[g].shape[1]), dtype=torch.int32, device=dev) for g in (0, 1)]
    ent = torch.empty(R, dtype=torch.float64, device=dev)
    wts = [[torch.empty((R, p.n_tiles[0]), dtype=torch.float64, device=dev) for _ in (0, 1)] for p in singles]

    def baseline():
        with torch.cuda.stream(stream):
            for l in range(L):
                for g in (0, 1):
                    torch.index_select(ids, 1, idx[g][l], out=ids_g[g])
                    for k, p in enumerate(singles):
                        _native._check(lib, lib.vet_spatial_entropy_windowed_ids(p.handle, ids_g[g].data_ptr(), ids_g[g].shape[1], T,
                                                                                 window, stride, ent.data_ptr(), wts[k][g].data_ptr(),
                                                                                 None, st.data_ptr(), stream.cuda_stream))
                D = None
                for k in range(K):
                    wa, wb = wts[k]
                    ha, hb = wa.abs(), wb.abs()
                    ka, kb = (wa != 0) | torch.signbit(wa), (wb != 0) | torch.signbit(wb)
                    (sa, Wa), (sb, Wb), (sp, _) = bits(ha, ka), bits(hb, kb), bits(ha + hb, ka | kb)
                    Dk = sp - (Wa * sa + Wb * sb) / (Wa + Wb)
                    Dk = torch.where((Wa > 0) & (Wb > 0), Dk, torch.full_like(Dk, float("nan")))
                    D = Dk if D is None else D + Dk
                base[l] = D / K

    for _ in range(WARMUP):
        call(); baseline()
    call(P_FULL, out_full)
    torch.cuda.synchronize()
    ms_c, ms_b, ms_f = [], [], []
    for _ in range(reps):
        ms_c.append(timed(stream, call))
        ms_b.append(timed(stream, baseline))
        ms_f.append(timed(stream, lambda: call(P_FULL, out_full)))
    kernels = profile_call(eng, call)
    kernels_full = profile_call(eng, lambda: call(P_FULL, out_full))
    blocks = lambda P: (P + 1 + 7) // 8
    flop = lambda P: 2.0 * 16 * blocks(P) * U * sum(plan.n_tiles) * R
    c_s, b_s, f_s = stats(ms_c), stats(ms_b), stats(ms_f)
    a = torch.cat([out_both[0][0][:, None], out_both[1]], dim=1).cpu().numpy()          # [R][L]
    b = base.cpu().numpy().T
    both = ~np.isnan(a) & ~np.isnan(b)
    spread = b_s["max_ms"] - b_s["min_ms"]
    summary = out_both[0].cpu().numpy()
    run = {"case": label, "users": U, "frames": T, "tile_counts": tcs, "window": window, "stride": stride, "rows": R,
           "permutations_both_routes": P_BOTH, "group_divergence": c_s, "kernels_ms": kernels,
           "baseline_two_windowed_ids_calls_per_labelling_and_lattice_on_gathered_ids": b_s,
           "baseline_calls": 2 * L * K, "baseline_spread_ms": round(spread, 4),
           "ratio_median_new_over_baseline": round(c_s["median_ms"] / b_s["median_ms"], 4),
           "new_route_not_slower_beyond_baseline_spread": bool(c_s["median_ms"] <= b_s["median_ms"] + spread),
           "gemm_flop": flop(P_BOTH), "gemm_fp64_tflops": round(flop(P_BOTH) / (kernels["k_group_gemm"] * 1e-3) / 1e12, 3),
           "permutations_full": P_FULL, "group_divergence_full": f_s, "kernels_ms_full": kernels_full,
           "gemm_fp64_tflops_full": round(flop(P_FULL) / (kernels_full["k_group_gemm"] * 1e-3) / 1e12, 3),
           "nan_positions_agree_with_baseline": bool(np.array_equal(np.isnan(a), np.isnan(b))),
           "max_abs_diff_vs_baseline_bits": float(np.max(np.abs(a[both] - b[both]), initial=0.0)),
           "observed_mean_bits": float(np.nanmean(summary[0])), "null_mean_bits": float(np.nanmean(summary[3])),
           "min_p_value": float(np.nanmin(summary[1])), "min_p_adjusted": float(np.nanmin(summary[2])),
           "null_equals_first_permutations_of_full_run": bool(np.array_equal(out_both[1].cpu().numpy(),
                                                                             out_full[1][:, :P_BOTH].cpu().numpy(), equal_nan=True))}
    print(json.dumps(run), flush=True)
    for p in singles:
        if p is not plan:
            p.close()
    plan.close()
    return run


def main(out_path, only=()):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    record = {"tool": "tools/group_divergence_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (tables built, workspace grown); "
                        "the call and its baseline alternate in the same run; median and min..max of the timed calls; both routes at "
                        f"P = {P_BOTH} because today's route takes minutes at P = {P_FULL}; the new call alone also at P = {P_FULL}",
              "runs": []}
    cases = (("config3_segments_w20_s20", 1024, 30000, [500], 20, 20, REPS),
             ("config3_whole_video", 1024, 30000, [500], 30000, 1, REPS),
             ("config4_reference_default_tile_counts_w20_s20", 256, 10000, [20, 50, 100, 250, 1000], 20, 20, REPS),
             ("config3_per_frame_w1_s1", 1024, 30000, [500], 1, 1, REPS))
    record["device"] = torch.cuda.get_device_name(0)
    record["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    for label, U, T, tcs, window, stride, reps in cases:
        if only and label not in only:
            continue
        record["runs"].append(run_case(eng, dev, stream, label, U, T, tcs, window, stride, reps))
        torch.cuda.empty_cache()
        with open(out_path, "w") as f:                 # after every case
            json.dump(record, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "group", "group_divergence_timing.json"), sys.argv[2:])
