"""Time of the viewer-to-crowd divergence (vet_crowd_divergence) at config 3's shape — 1024 viewers x 30 000 frames, [500],
weighted — in three cases: window = stride = 20 (1 500 rows), the whole video (one row) and window 20 at stride 1 (29 981 rows).
Each case alternates, in the same run, the new device call with today's device route to the same information:
vet_user_entropy with d_weights (every viewer's row histogram, [U][R][n] f64) plus vet_spatial_entropy_windowed with d_weights
(the pooled row histograms, [R][n]).  That route is a LOWER BOUND of today's cost: the combination of the two weight arrays into
D, pooled, within and between (numpy today) and the download of the viewer histograms are not charged to it.  At stride 1 the
viewer histograms are 123 GB, so there the baseline runs vet_user_entropy_ids on slices of SLICE viewers (contiguous id slices
prepared beforehand, not charged) into one reused weights buffer; the record says so.
Inputs resident, hipEvents on the launch stream after a warm-up; per side the median and the min..max spread of REPS single
calls.  The new call is expected to be no slower than the route at window = stride = 20; the margin is the baseline's own spread
in that run.  The record states the outcome and, where the new call is slower, by how much and which kernel carries it (each
stage's time less its counterpart's in the baseline) — no exit code depends on it.  Also recorded: the per-kernel times from the
engine's profile scopes (k_spatial = k_user_dirs, k_weights = stage 2's k_weights_gather, k_finalize = k_window_hist_w +
k_crowd_logp + k_crowd_rows, k_transition = k_crowd_w), the largest difference between the new call's D / row series and the
combination of the baseline's weight arrays in torch (window = stride = 20 and the whole video), and the largest absolute error
against the numpy oracle (tests/_crowd_oracle.py) at the tests' small shape.
usage: python tools/crowd_divergence_timing.py [out.json]      (default: profiles/user/crowd_divergence_timing.json)"""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'viewport-entropy-toolkit_amd'))
import numpy as np
import torch
from viewport_entropy_toolkit import _native, _quantiser, _synthetic
import bench

TCS = [500]
VW, VH = 100, 200
U, T = 1024, 30000
WARMUP, REPS = 1, 5
SLICE = 32                                      # viewers per vet_user_entropy_ids call of the stride-1 baseline


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def kernel_split(eng, fn, names):
    eng.profile_enable(True); eng.profile_reset()
    fn()
    eng.synchronize(); torch.cuda.synchronize()
    k = {label: round(eng.profile_get(name)[0], 4) for label, name in names.items()}
    eng.profile_enable(False)
    return k


CROWD_KERNELS = {"stage1_k_user_dirs": "k_spatial", "stage2_k_weights_gather": "k_weights",
                 "stage3_5_k_window_hist_w_and_k_crowd_rows": "k_finalize", "stage4_k_crowd_w": "k_transition"}
BASE_KERNELS = {"k_user_dirs": "k_spatial", "k_user_entropy_w_and_k_weights_gather": "k_weights", "k_window_entropy_w": "k_finalize"}


def direction_ids(mu, mv):
    """[T][U] i32 ids on the plan's pixel grid (-1 absent): the quantiser's truncation of mu * W, mv * H."""
    absent = torch.isnan(mu) | torch.isnan(mv)
    px, py = (torch.nan_to_num(mu) * VW).to(torch.int64), (torch.nan_to_num(mv) * VH).to(torch.int64)
    return torch.where(absent, torch.full_like(px, -1), py * (VW + 1) + px).to(torch.int32)


def combine(w_u, w_p, chunk=64):
    """(D[U][R], series[3][R]) from the baseline's weight arrays on the device, in torch: w_u [U][R][n], w_p [R][n] (dense
    tile_weights encoding; this input has no zero-valued keys)."""
    P = w_p.abs()
    Wr = P.sum(dim=1)                                                         # [R]
    p = P / Wr[:, None]
    pooled = -torch.where(P > 0, p * torch.log2(p), torch.zeros_like(p)).sum(dim=1)
    D = torch.empty(w_u.shape[:2], dtype=torch.float64, device=w_u.device)
    within, between = torch.zeros_like(Wr), torch.zeros_like(Wr)
    for a in range(0, w_u.shape[0], chunk):
        h = w_u[a:a + chunk].abs()                                            # [c][R][n]
        Wu = h.sum(dim=2)
        q = h / Wu[:, :, None]
        key = h > 0
        zero = torch.zeros_like(q)
        own = -torch.where(key, q * torch.log2(q), zero).sum(dim=2)
        d = torch.where(key, q * torch.log2(q / p[None]), zero).sum(dim=2)
        present = Wu > 0
        D[a:a + chunk] = torch.where(present, d, torch.full_like(d, float("nan")))
        m = torch.where(present, Wu / Wr[None, :], torch.zeros_like(Wu))
        within += (m * torch.where(present, own, torch.zeros_like(own))).sum(dim=0)
        between += (m * torch.where(present, d, torch.zeros_like(d))).sum(dim=0)
    return D, torch.stack([pooled, within, between])


def run_case(eng, dev, stream, plan, st, mu, mv, ids, label, window, stride):
    n = plan.n_tiles[0]
    R = (T - window) // stride + 1
    sliced = (U * R * n * 8) > (16 << 30)
    div = torch.empty((U, R), dtype=torch.float64, device=dev)
    rows = torch.empty((3, R), dtype=torch.float64, device=dev)
    ent_u = torch.empty((U, R), dtype=torch.float64, device=dev)
    ent_p = torch.empty(R, dtype=torch.float64, device=dev)
    w_p = torch.empty((R, n), dtype=torch.float64, device=dev)
    su = SLICE if sliced else U
    w_u = torch.empty((su, R, n), dtype=torch.float64, device=dev)
    id_slices = [ids[:, a:a + su].contiguous() for a in range(0, U, su)] if sliced else None
    lib = eng.lib

    def call():
        plan.spatial_crowd_divergence_device(mu.data_ptr(), mv.data_ptr(), U, T, window, stride, div.data_ptr(), rows.data_ptr(),
                                             d_status=st.data_ptr(), stream=stream.cuda_stream)

    def baseline():
        if sliced:
            for i, sl in enumerate(id_slices):
                _native._check(lib, lib.vet_user_entropy_ids(plan.handle, sl.data_ptr(), su, T, window, stride,
                                                             ent_u[i * su:].data_ptr(), w_u.data_ptr(), None, st.data_ptr(),
                                                             stream.cuda_stream))
        else:
            plan.spatial_per_user_device(mu.data_ptr(), mv.data_ptr(), U, T, window, stride, ent_u.data_ptr(), w_u.data_ptr(),
                                         d_status=st.data_ptr(), stream=stream.cuda_stream)
        plan.spatial_windowed_device(mu.data_ptr(), mv.data_ptr(), U, T, window, stride, ent_p.data_ptr(), w_p.data_ptr(),
                                     d_status=st.data_ptr(), stream=stream.cuda_stream)

    for _ in range(WARMUP):
        call(); baseline()
    torch.cuda.synchronize()
    ms_c, ms_b = [], []
    for _ in range(REPS):
        ms_c.append(timed(stream, call))
        ms_b.append(timed(stream, baseline))
    c_s, b_s = stats(ms_c), stats(ms_b)
    spread = round(b_s["max_ms"] - b_s["min_ms"], 4)
    run = {"case": label, "users": U, "frames": T, "window": window, "stride": stride, "rows": R,
           "output_bytes": int(div.numel() * 8 + rows.numel() * 8),
           "baseline_weight_bytes": int(U * R * n * 8 + R * n * 8),
           "crowd_divergence": c_s, "kernels_ms": kernel_split(eng, call, CROWD_KERNELS),
           "baseline_user_entropy_and_windowed_with_weights": b_s, "baseline_kernels_ms": kernel_split(eng, baseline, BASE_KERNELS),
           "baseline_spread_ms": spread,
           "baseline_note": (f"vet_user_entropy_ids on {U // su} slices of {su} viewers into one reused {su} x R x n weights buffer "
                             "(the whole array would be 123 GB); a lower bound: no combination, no download") if sliced else
                            "one vet_user_entropy call with d_weights; a lower bound: no combination, no download",
           "ratio_median_crowd_over_baseline": round(c_s["median_ms"] / b_s["median_ms"], 3),
           "no_slower_than_baseline_within_its_spread": bool(c_s["median_ms"] <= b_s["median_ms"] + spread)}
    # the two sides share k_user_dirs, the gather and the pooled row sums; what differs is k_crowd_w against k_user_entropy_w
    # (the baseline's k_weights scope less the gather, which the new call's k_weights scope holds alone)
    k, bk = run["kernels_ms"], run["baseline_kernels_ms"]
    run["k_crowd_w_vs_baseline_k_user_entropy_w_ms"] = [k["stage4_k_crowd_w"], round(
        bk["k_user_entropy_w_and_k_weights_gather"] - k["stage2_k_weights_gather"], 4)]
    if not run["no_slower_than_baseline_within_its_spread"]:
        run["slower_by_ms"] = round(c_s["median_ms"] - b_s["median_ms"], 4)
        others = {"stage1_k_user_dirs": k["stage1_k_user_dirs"] - bk["k_user_dirs"],
                  "stage3_5_k_window_hist_w_and_k_crowd_rows": k["stage3_5_k_window_hist_w_and_k_crowd_rows"] - bk["k_window_entropy_w"],
                  "stage4_k_crowd_w": k["stage4_k_crowd_w"] - run["k_crowd_w_vs_baseline_k_user_entropy_w_ms"][1]}
        run["carried_by"] = max(others, key=others.get)
        run["kernel_excess_ms"] = {n: round(v, 4) for n, v in others.items()}
    d = div.cpu().numpy()
    run["nan_entries"] = int(np.isnan(d).sum())
    run["mean_divergence_bits"] = float(np.nanmean(d))
    r3 = rows.cpu().numpy()
    run["mean_pooled_within_between_bits"] = [float(x) for x in np.nanmean(r3, axis=1)]
    run["max_identity_residual_bits"] = float(np.nanmax(np.abs(r3[0] - r3[1] - r3[2])))
    if not sliced:
        with torch.cuda.stream(stream):
            D2, S2 = combine(w_u, w_p)
        torch.cuda.synchronize()
        D2, S2 = D2.cpu().numpy(), S2.cpu().numpy()
        run["nan_positions_agree_with_baseline_combination"] = bool(np.array_equal(np.isnan(d), np.isnan(D2)))
        run["max_abs_diff_vs_baseline_combination_bits"] = {"divergence": float(np.nanmax(np.abs(d - D2))),
                                                            "rows": float(np.nanmax(np.abs(r3 - S2)))}
    print(json.dumps(run), flush=True)
    return run


def oracle_error(eng):
    """The largest |value - oracle| at the tests' small shape (U = 9, T = 150, window 20, stride 7), per plan."""
    from oracle import vet_oracle as vo
    from tests import _crowd_oracle as co
    mu, mv = _synthetic.random_walk_video(9, 150, base_seed=7, p_absent=0.1)
    out = {}
    for tcs, weighted in (([50], True), ([1000], True), ([50, 100, 200], True), ([50], False)):
        plan = _native.Plan(eng, [vo.fibonacci_lattice(t) for t in tcs], 120.0, 2.0, weighted, VW, VH)
        got = plan.spatial_crowd_divergence(mu=mu, mv=mv, window=20, stride=7)
        div, series, _ = co.fast(mu, mv, VW, VH, tcs, 20, 7, use_weight_distribution=weighted)
        assert np.array_equal(np.isnan(got["divergence"]), np.isnan(div))
        out[f"{'w' if weighted else 'u'}_tc{'_'.join(map(str, tcs))}"] = {
            "divergence": float(np.nanmax(np.abs(got["divergence"] - div))), "rows": float(np.nanmax(np.abs(got["rows"] - series)))}
        plan.close()
    return out


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(tc) for tc in TCS], 120.0, 2.0, True, VW, VH)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    record = {"tool": "tools/crowd_divergence_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "tile_counts": TCS,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (tables built, workspace grown); "
                        "the call and its baseline alternate in the same run; median and min..max of REPS calls", "runs": []}
    mu_h, mv_h = bench.synth_video(U, T, 1234, 0)
    mu = torch.from_numpy(mu_h).to(dev); mv = torch.from_numpy(mv_h).to(dev)
    ids = direction_ids(mu, mv)
    for label, window, stride in (("segments_w20_s20", 20, 20), ("whole_video", T, 1), ("sliding_w20_s1", 20, 1)):
        record["runs"].append(run_case(eng, dev, stream, plan, st, mu, mv, ids, label, window, stride))
        torch.cuda.empty_cache()
    plan.close()
    record["max_abs_err_vs_numpy_oracle_bits"] = oracle_error(eng)
    print(json.dumps(record["max_abs_err_vs_numpy_oracle_bits"]), flush=True)
    record["device"] = torch.cuda.get_device_name(0)
    record["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "user", "crowd_divergence_timing.json"))
