"""Time of the pairwise viewer divergence (vet_user_divergence) on [500], weighted, in two settings:
  A  config 3's shape, 1024 viewers x 30 000 frames: the whole video (one 1024 x 1024 matrix) and window 20 at the stride that
     gives 16 rows — the call alone, with its per-kernel split;
  B  128 viewers x 3 000 frames, against the existing way to get the same numbers on the device: vet_user_entropy_ids on the
     MATERIALISED pair input — one "viewer" per pair u < v whose frames are u's frames of the row and then v's (window doubled) —
     and on the viewers themselves, then the three-term combination D = S_uv - (W_u S_u + W_v S_v) / (W_u + W_v) in torch on the
     device (S = entropy * log2(n), W = the row sums of d_weights).  Building the pair input is not charged to the baseline.
     The new call must be faster: the tool exits with an error where it is not.
Inputs resident, hipEvents on the launch stream after a warm-up, the two sides alternating in the same run; per side the median
and the min..max spread of REPS single calls.  Also recorded: the per-kernel times from the engine's profile scopes (k_spatial =
k_user_dirs, k_weights = k_user_hist_w, k_finalize = k_user_divergence), the largest difference between the two sides' matrices,
and the largest absolute error against the numpy oracle (tests/_divergence_oracle.py) at the tests' small shape.
usage: python tools/user_divergence_timing.py [out.json]      (default: profiles/user/user_divergence_timing.json)"""
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


def kernel_split(eng, fn):
    eng.profile_enable(True); eng.profile_reset()
    fn()
    eng.synchronize(); torch.cuda.synchronize()
    k = {name: round(eng.profile_get(name)[0], 4) for name in ("k_spatial", "k_weights", "k_finalize")}
    eng.profile_enable(False)
    return {"stage1_k_user_dirs": k["k_spatial"], "stage2_k_user_hist_w": k["k_weights"], "stage3_k_user_divergence": k["k_finalize"]}


def direction_ids(mu, mv):
    """[T][U] i32 ids on the plan's pixel grid (-1 absent): the quantiser's truncation of mu * W, mv * H."""
    absent = torch.isnan(mu) | torch.isnan(mv)
    px, py = (torch.nan_to_num(mu) * VW).to(torch.int64), (torch.nan_to_num(mv) * VH).to(torch.int64)
    return torch.where(absent, torch.full_like(px, -1), py * (VW + 1) + px).to(torch.int32)


def setting_a(eng, dev, stream, plan, st):
    U, T = 1024, 30000
    mu_h, mv_h = bench.synth_video(U, T, 1234, 0)
    mu = torch.from_numpy(mu_h).to(dev); mv = torch.from_numpy(mv_h).to(dev)
    runs = []
    for label, window, stride in (("whole_video", T, 1), ("w20_16_rows", 20, (T - 20) // 15)):
        R = (T - window) // stride + 1
        div = torch.empty((R, U, U), dtype=torch.float64, device=dev)

        def call():
            plan.spatial_user_divergence_device(mu.data_ptr(), mv.data_ptr(), U, T, window, stride, div.data_ptr(),
                                                d_status=st.data_ptr(), stream=stream.cuda_stream)
        for _ in range(WARMUP):
            call()
        torch.cuda.synchronize()
        ms = [timed(stream, call) for _ in range(REPS)]
        run = {"setting": "A", "case": label, "users": U, "frames": T, "window": window, "stride": stride, "rows": R,
               "pairs_per_row": U * (U - 1) // 2, "divergence": stats(ms), "kernels_ms": kernel_split(eng, call)}
        d = div.cpu().numpy()
        run["nan_entries"] = int(np.isnan(d).sum())
        run["mean_divergence_bits"] = float(np.nanmean(d))
        runs.append(run)
        print(json.dumps(run), flush=True)
        del div
    return runs


def setting_b(eng, dev, stream, plan, st):
    U, T = 128, 3000
    n = plan.n_tiles[0]
    mu_h, mv_h = bench.synth_video(U, T, 4321, 0)
    mu = torch.from_numpy(mu_h).to(dev); mv = torch.from_numpy(mv_h).to(dev)
    ids = direction_ids(mu, mv)                                          # [T][U]
    iu, iv = torch.triu_indices(U, U, offset=1, device=dev)
    P = iu.numel()
    runs = []
    for label, window, stride in (("whole_video", T, 1), ("w20_15_rows", 20, (T - 20) // 14)):
        R = (T - window) // stride + 1
        # the pair input: row r of pair (u, v) = u's `window` frames of row r, then v's: [R * 2 * window][P], window' = stride' = 2 * window
        f = (torch.arange(R, device=dev) * stride)[:, None] + torch.arange(window, device=dev)[None, :]      # [R][window]
        rows_u, rows_v = ids[f][:, :, iu], ids[f][:, :, iv]                                               # [R][window][P]
        pair_ids = torch.cat([rows_u, rows_v], dim=1).reshape(R * 2 * window, P).contiguous()
        own_ids = ids[f].reshape(R * window, U).contiguous()                                               # the viewers' own rows
        div = torch.empty((R, U, U), dtype=torch.float64, device=dev)
        base = torch.empty((R, U, U), dtype=torch.float64, device=dev)
        ent_p = torch.empty((P, R), dtype=torch.float64, device=dev)
        ent_o, w_o = torch.empty((U, R), dtype=torch.float64, device=dev), torch.empty((U, R, n), dtype=torch.float64, device=dev)
        lib = eng.lib

        def call():
            plan.spatial_user_divergence_device(mu.data_ptr(), mv.data_ptr(), U, T, window, stride, div.data_ptr(),
                                                d_status=st.data_ptr(), stream=stream.cuda_stream)

        def baseline():
            for src, n_u, w, ent, wt in ((pair_ids, P, 2 * window, ent_p, None), (own_ids, U, window, ent_o, w_o.data_ptr())):
                _native._check(lib, lib.vet_user_entropy_ids(plan.handle, src.data_ptr(), n_u, src.shape[0], w, w, ent.data_ptr(),
                                                             wt, None, st.data_ptr(), stream.cuda_stream))
            with torch.cuda.stream(stream):
                log2n = float(np.log2(n))
                S_p = ent_p * log2n                                                                        # [P][R]
                S_o, W_o = ent_o * log2n, w_o.abs().sum(dim=2)                                             # [U][R]
                d = S_p - (W_o[iu] * S_o[iu] + W_o[iv] * S_o[iv]) / (W_o[iu] + W_o[iv])
                base.zero_()
                base[:, iu, iv] = d.t()
                base[:, iv, iu] = d.t()
        for _ in range(WARMUP):
            call(); baseline()
        torch.cuda.synchronize()
        ms_d, ms_b = [], []
        for _ in range(REPS):
            ms_d.append(timed(stream, call))
            ms_b.append(timed(stream, baseline))
        a, b = div.cpu().numpy(), base.cpu().numpy()
        offdiag = np.broadcast_to(~np.eye(U, dtype=bool), a.shape)             # the baseline leaves the diagonal 0
        off = offdiag & ~np.isnan(a) & ~np.isnan(b)
        d_s, b_s = stats(ms_d), stats(ms_b)
        run = {"setting": "B", "case": label, "users": U, "frames": T, "window": window, "stride": stride, "rows": R, "pairs_per_row": P,
               "pair_input_bytes": int(pair_ids.numel() * 4), "divergence": d_s, "kernels_ms": kernel_split(eng, call),
               "baseline_user_entropy_on_pair_input": b_s, "speedup_median": round(b_s["median_ms"] / d_s["median_ms"], 3),
               "faster_than_baseline": bool(d_s["median_ms"] < b_s["median_ms"]),
               "nan_positions_agree": bool(np.array_equal(np.isnan(a) & offdiag, np.isnan(b) & offdiag)),
               "max_abs_diff_vs_baseline_bits": float(np.max(np.abs(a[off] - b[off]))) if off.any() else 0.0}
        runs.append(run)
        print(json.dumps(run), flush=True)
    return runs


def oracle_error(eng):
    """The largest |D - oracle| at the tests' small shape (U = 9, T = 150, window 20, stride 7), per plan."""
    from oracle import vet_oracle as vo
    from tests import _divergence_oracle as do
    mu, mv = _synthetic.random_walk_video(9, 150, base_seed=7, p_absent=0.1)
    out = {}
    for tcs, weighted in (([50], True), ([1000], True), ([50, 100, 200], True), ([50], False)):
        plan = _native.Plan(eng, [vo.fibonacci_lattice(t) for t in tcs], 120.0, 2.0, weighted, VW, VH)
        got = plan.spatial_user_divergence(mu=mu, mv=mv, window=20, stride=7)["divergence"]
        want, _ = do.fast(mu, mv, VW, VH, tcs, 20, 7, use_weight_distribution=weighted)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        out[f"{'w' if weighted else 'u'}_tc{'_'.join(map(str, tcs))}"] = float(np.nanmax(np.abs(got - want)))
        plan.close()
    return out


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(tc) for tc in TCS], 120.0, 2.0, True, VW, VH)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    record = {"tool": "tools/user_divergence_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "tile_counts": TCS,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (tables built, workspace grown); "
                        "the call and its baseline alternate in the same run; median and min..max of REPS calls", "runs": []}
    record["runs"] += setting_b(eng, dev, stream, plan, st)
    record["runs"] += setting_a(eng, dev, stream, plan, st)
    plan.close()
    record["max_abs_err_vs_numpy_oracle_bits"] = oracle_error(eng)
    print(json.dumps(record["max_abs_err_vs_numpy_oracle_bits"]), flush=True)
    record["device"] = torch.cuda.get_device_name(0)
    record["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", out_path)
    if not all(r["faster_than_baseline"] for r in record["runs"] if r["setting"] == "B"):
        sys.exit("vet_user_divergence is not faster than vet_user_entropy on the materialised pair input")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "user", "user_divergence_timing.json"))
