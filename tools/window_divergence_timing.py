"""Time of the window-to-window divergence (vet_window_divergence), weighted plans, window 20:
  config 3's shape (1024 viewers x 30 000 frames, [500]): stride 20 with max_lag 1, 32 and R - 1 (the whole 1 500-row recurrence
      band), and stride 1 with max_lag 20;
  a config-4-shaped video (256 x 10 000, the reference's default tile_counts) at stride 20, max_lag 1;
  config 2 (64 x 3 000, [50, 100, 200]) at stride 1, max_lag 1.
Per shape the device call alone (inputs resident, hipEvents on the launch stream) with its per-kernel split from the engine's
profile scopes (stage 1 = k_weights + k_spatial, stage 2 = k_finalize, the pair stage = k_transition), pairs/s and overlap-tile
log2/s (tiles on which both windows of a pair have weight, counted from lattice 0's histograms), and two baselines alternating
with it in the same run:
  today   today's route to the same numbers: vet_spatial_entropy_windowed_host with weights (one call per lattice: the call
          returns lattice 0's histograms) and the band in numpy on the host; against it the new HOST entry
          (Plan.spatial_window_divergence on the same host arrays), wall clock;
  device  a device-only route, one lattice at a time: the pooled term of every pair through the per-frame fp64 call
          (vet_spatial_entropy on a vet_plan_set_fp64 plan) over the MATERIALISED pooled-pair input [pairs][2 * window * U], the own
          terms from vet_spatial_entropy_windowed with weights, the three-term combination in torch — only where the pair input
          stays under 1 GB; building the input is not charged.
After a warm-up; per side the median and the min..max spread of REPS single calls.  Nothing gates on a speed ratio: the JSON holds
the numbers, also where the new call does not win.  Also recorded: the largest absolute error against the numpy oracle
(tests/_window_divergence_oracle.py: fast) on a 128 x 3 000 slice of config 3's video.
usage: python tools/window_divergence_timing.py [out.json]      (default: profiles/windowed/window_divergence_timing.json)"""
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
WINDOW = 20
WARMUP, REPS, HOST_REPS = 1, 5, 3
PAIR_INPUT_LIMIT = 1 << 30
# (workload, users, frames, tile_counts, stride, max_lag or None = R - 1)
SHAPES = [("config3", 1024, 30000, [500], 20, 1), ("config3", 1024, 30000, [500], 20, 32), ("config3", 1024, 30000, [500], 20, None),
          ("config3", 1024, 30000, [500], 1, 20), ("config4_shape", 256, 10000, [20, 50, 100, 250, 1000], 20, 1),
          ("config2", 64, 3000, [50, 100, 200], 1, 1)]


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def band(h, keys, L):
    """The numpy band of today's route (tests/_window_divergence_oracle.py: band, without the term tables)."""
    R = h.shape[0]
    out = np.full((R, L), np.nan)
    present = keys.any(axis=1)
    with np.errstate(all="ignore"):
        Wt = h.sum(axis=1)
        q = np.where(keys, h / Wt[:, None], 1.0)
        own = -(q * np.log2(q)).sum(axis=1)
        for l in range(1, L + 1):
            a, b = slice(0, R - l), slice(l, R)
            Wp = Wt[a] + Wt[b]
            qp = np.where(keys[a] | keys[b], (h[a] + h[b]) / Wp[:, None], 1.0)
            D = -(qp * np.log2(qp)).sum(axis=1) - (Wt[a] * own[a] + Wt[b] * own[b]) / Wp
            D[~(present[a] & present[b])] = np.nan
            out[:R - l, l - 1] = D
    return out


def materialise(x, window, stride):
    """[T][U] -> [R][window * U], frame-major then user order inside a row."""
    return x.unfold(0, window, stride).permute(0, 2, 1).reshape(-1, window * x.shape[1]).contiguous()


def run_shape(eng, dev, stream, name, U, T, tcs, stride, L, video):
    mu_h, mv_h = video
    mu = torch.from_numpy(mu_h).to(dev); mv = torch.from_numpy(mv_h).to(dev)
    lattices = [_quantiser.lattice_xyz(tc) for tc in tcs]
    plan = _native.Plan(eng, lattices, 120.0, 2.0, True, VW, VH)
    singles = [_native.Plan(eng, [x], 120.0, 2.0, True, VW, VH) for x in lattices] if len(tcs) > 1 else [plan]
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    R = (T - WINDOW) // stride + 1
    L = R - 1 if L is None else L
    pairs = sum(R - l for l in range(1, L + 1))
    div = torch.empty((R, L), dtype=torch.float64, device=dev)

    def call():
        plan.spatial_window_divergence_device(mu.data_ptr(), mv.data_ptr(), U, T, WINDOW, stride, L, div.data_ptr(),
                                              d_status=st.data_ptr(), stream=stream.cuda_stream)

    def host_new():
        return plan.spatial_window_divergence(mu=mu_h, mv=mv_h, window=WINDOW, stride=stride, max_lag=L)["divergence"]

    split = {}

    def host_today():
        out, t_gpu, t_np = None, 0.0, 0.0
        for p in singles:
            t, wt = wall(lambda: p.spatial_windowed(mu=mu_h, mv=mv_h, window=WINDOW, stride=stride, want_weights=True)["weights"])
            t_gpu += t
            t, Dk = wall(lambda: band(np.abs(wt), (wt != 0) | np.signbit(wt), L))
            t_np += t
            out = Dk if out is None else out + Dk
        split["windowed_host_calls_ms"], split["numpy_band_ms"] = round(t_gpu, 3), round(t_np, 3)
        return out / len(singles)

    # ---- the device-only route, where its input fits
    pair_bytes = pairs * 2 * WINDOW * U * 16
    device_route = None
    if pair_bytes < PAIR_INPUT_LIMIT:
        rows_mu, rows_mv = materialise(mu, WINDOW, stride), materialise(mv, WINDOW, stride)           # [R][w U]
        ia = torch.cat([torch.arange(0, R - l, device=dev) for l in range(1, L + 1)])
        il = torch.cat([torch.full((R - l,), l, device=dev) for l in range(1, L + 1)])
        pmu = torch.cat([rows_mu[ia], rows_mu[ia + il]], dim=1).contiguous()                          # [pairs][2 w U]
        pmv = torch.cat([rows_mv[ia], rows_mv[ia + il]], dim=1).contiguous()
        del rows_mu, rows_mv
        fp64 = []
        for x in lattices:
            p = _native.Plan(eng, [x], 120.0, 2.0, True, VW, VH)
            p.set_fp64(True)
            fp64.append(p)
        ent_p = torch.empty(pairs, dtype=torch.float64, device=dev)
        ent_o = torch.empty(R, dtype=torch.float64, device=dev)
        w_o = torch.empty((R, max(p.n_tiles[0] for p in singles)), dtype=torch.float64, device=dev)
        base = torch.full((R, L), float("nan"), dtype=torch.float64, device=dev)

        def device_route():
            acc = None
            for p64, p1 in zip(fp64, singles):
                n = p1.n_tiles[0]
                p64.spatial_device(pmu.data_ptr(), pmv.data_ptr(), 2 * WINDOW * U, pairs, ent_p.data_ptr(), d_status=st.data_ptr(),
                                   stream=stream.cuda_stream)
                p1.spatial_windowed_device(mu.data_ptr(), mv.data_ptr(), U, T, WINDOW, stride, ent_o.data_ptr(),
                                           d_weights=w_o.data_ptr(), d_status=st.data_ptr(), stream=stream.cuda_stream)
                with torch.cuda.stream(stream):
                    log2n = float(np.log2(n))
                    S_o, W_o = ent_o * log2n, w_o.view(-1)[:R * n].view(R, n).abs().sum(dim=1)
                    ib = ia + il
                    d = ent_p * log2n - (W_o[ia] * S_o[ia] + W_o[ib] * S_o[ib]) / (W_o[ia] + W_o[ib])
                    acc = d if acc is None else acc + d
            with torch.cuda.stream(stream):
                base[ia, il - 1] = acc / len(singles)

    run = {"workload": name, "users": U, "frames": T, "tile_counts": tcs, "window": WINDOW, "stride": stride, "max_lag": L, "rows": R,
           "pairs": pairs}
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    if device_route is not None:
        try:
            device_route()
            torch.cuda.synchronize()
        except _native.NativeError as e:
            run["device_route_refused"] = str(e)
            device_route = None
    else:
        run["device_route_skipped"] = f"pooled-pair input of {pair_bytes} bytes (limit {PAIR_INPUT_LIMIT})"
    ms_c, ms_d = [], []
    for _ in range(REPS):
        ms_c.append(timed(stream, call))
        if device_route is not None:
            ms_d.append(timed(stream, device_route))
    host_new(); host_today()
    ms_hn, ms_ht = [], []
    for _ in range(HOST_REPS):
        t, got = wall(host_new)
        ms_hn.append(t)
        t, today = wall(host_today)
        ms_ht.append(t)
    eng.profile_enable(True); eng.profile_reset()
    call()
    eng.synchronize(); torch.cuda.synchronize()
    k = {x: round(eng.profile_get(x)[0], 4) for x in ("k_weights", "k_spatial", "k_finalize", "k_transition")}
    eng.profile_enable(False)
    # overlap tiles of lattice 0 (the pair stage's log2 count, up to the per-lattice differences)
    wt0 = singles[0].spatial_windowed(mu=mu_h, mv=mv_h, window=WINDOW, stride=stride, want_weights=True)["weights"]
    key0 = torch.from_numpy(np.abs(wt0) > 0).to(dev)
    overlap = int(sum(int((key0[:R - l] & key0[l:]).sum()) for l in range(1, L + 1)))
    c_s, hn_s, ht_s = stats(ms_c), stats(ms_hn), stats(ms_ht)
    d_new = div.cpu().numpy()
    ok = ~np.isnan(d_new) & ~np.isnan(today)
    run.update({"device_call": c_s,
                "kernels_ms": {"stage1_k_weights_gather": k["k_weights"], "stage1_k_window_tiles": k["k_spatial"],
                               "stage2_k_window_hist": k["k_finalize"], "stage3_k_window_divergence": k["k_transition"]},
                "pairs_per_s": round(pairs / (c_s["median_ms"] * 1e-3), 1),
                "overlap_tiles_lattice0": overlap,
                "overlap_log2_per_s_in_pair_stage": round(overlap * len(tcs) / max(k["k_transition"] * 1e-3, 1e-9), 1),
                "host_entry_wall": hn_s, "today_windowed_host_plus_numpy_band_wall": {**ht_s, **split},
                "host_speedup_median": round(ht_s["median_ms"] / hn_s["median_ms"], 3),
                "nan_positions_agree_with_today": bool(np.array_equal(np.isnan(d_new), np.isnan(today))),
                "max_abs_diff_vs_today_bits": float(np.max(np.abs(d_new[ok] - today[ok]))) if ok.any() else 0.0,
                "host_entry_equals_device_call": bool(got.tobytes() == d_new.tobytes())})
    if device_route is not None:
        d_s = stats(ms_d)
        b = base.cpu().numpy()
        okb = ~np.isnan(d_new) & ~np.isnan(b)
        run.update({"device_route_per_frame_fp64_on_pair_input": d_s, "pair_input_bytes": int(pair_bytes),
                    "device_speedup_median": round(d_s["median_ms"] / c_s["median_ms"], 3),
                    "max_abs_diff_vs_device_route_bits": float(np.max(np.abs(d_new[okb] - b[okb]))) if okb.any() else 0.0})
        for p in fp64:
            p.close()
    for p in singles:
        if p is not plan:
            p.close()
    plan.close()
    torch.cuda.empty_cache()
    return run


def oracle_error(eng, video):
    """The largest |D - fast| on a 128 x 3 000 slice of config 3's video, [500], window 20, stride 20, the whole band."""
    from tests import _window_divergence_oracle as wdo
    mu, mv = np.ascontiguousarray(video[0][:3000, :128]), np.ascontiguousarray(video[1][:3000, :128])
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(500)], 120.0, 2.0, True, VW, VH)
    got = plan.spatial_window_divergence(mu=mu, mv=mv, window=WINDOW, stride=20, max_lag=149)["divergence"]
    want, _ = wdo.fast(mu, mv, VW, VH, [500], WINDOW, 20, 149)
    plan.close()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    return float(np.nanmax(np.abs(got - want)))


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    record = {"tool": "tools/window_divergence_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "host_reps": HOST_REPS,
              "timing": "device sides: hipEvents around single calls on the launch stream after WARMUP calls (tables built, workspace "
                        "grown), the call and the device route alternating; host sides: wall clock of whole calls on host arrays, the "
                        "new host entry and today's route alternating; median and min..max", "runs": []}
    videos = {}
    for name, U, T, tcs, stride, L in SHAPES:
        if (U, T) not in videos:
            videos[(U, T)] = bench.synth_video(U, T, 1234, 0)
        run = run_shape(eng, dev, stream, name, U, T, tcs, stride, L, videos[(U, T)])
        record["runs"].append(run)
        print(json.dumps(run), flush=True)
    record["max_abs_err_vs_numpy_oracle_bits_128x3000"] = oracle_error(eng, videos[(1024, 30000)])
    print(record["max_abs_err_vs_numpy_oracle_bits_128x3000"], flush=True)
    record["device"] = torch.cuda.get_device_name(0)
    record["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "windowed", "window_divergence_timing.json"))
