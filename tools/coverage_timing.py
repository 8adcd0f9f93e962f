"""Time of the attention coverage (vet_coverage), weighted plans, fractions 0.5 / 0.8 / 0.95:
  config 3's shape (1024 viewers x 30 000 frames, [500]): window = stride = 20 (1 500 rows) at max_lag 0, 1, 32 and 1 499 (every
      later window), and window = stride = 1 (30 000 rows) at max_lag 0 and 10;
  a config-4-shaped video (256 x 10 000) on [1000]: window = stride = 20 at max_lag 8.
Per shape the device call alone (inputs resident, hipEvents on the launch stream) with its per-kernel split from the engine's
profile scopes (stage 1 = k_weights + k_spatial, stage 2 = k_finalize, k_coverage_rank = k_transition, k_coverage_hits = k_wtab),
the windowed call alone (what stage 1 and the entropy epilogue cost without coverage), and today's route to the same numbers
alternating with the new call in the same run — existing calls only, so it is the same code before and after this call existed:
  today   vet_spatial_entropy_windowed with d_weights, then torch on the device: a stable descending sort of |weights|, a
          cumulative sum, a threshold search, a rank scatter and max_lag + 1 masked sums.
After a warm-up; per side the median and the min..max spread of REPS single calls.  Nothing gates on a speed ratio: the JSON holds
the numbers, also where the new call does not win.  Also recorded: whether the two routes agree (tiles exactly — torch's cumulative
sum is a parallel scan, not the contract's single accumulator, so an entry on a threshold may differ — and hit to 1e-12), and
what the sequential sum costs inside k_coverage_rank (``chain_probe``).
usage: python tools/coverage_timing.py [out.json]      (default: profiles/coverage/coverage_timing.json)"""
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
FRACTIONS = (0.5, 0.8, 0.95)
WARMUP, REPS = 1, 5
# (workload, users, frames, tile count, window = stride, max_lag or None = R - 1)
SHAPES = [("config3", 1024, 30000, 500, 20, 0), ("config3", 1024, 30000, 500, 20, 1), ("config3", 1024, 30000, 500, 20, 32),
          ("config3", 1024, 30000, 500, 20, None), ("config3", 1024, 30000, 500, 1, 0), ("config3", 1024, 30000, 500, 1, 10),
          ("config4_shape", 256, 10000, 1000, 20, 8)]


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def run_shape(eng, dev, stream, name, U, T, tc, window, L, video):
    mu = torch.from_numpy(video[0]).to(dev); mv = torch.from_numpy(video[1]).to(dev)
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(tc)], 120.0, 2.0, True, VW, VH)
    n, Q = plan.n_tiles[0], len(FRACTIONS)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    R = (T - window) // window + 1
    L = R - 1 if L is None else L
    tiles = torch.empty((R, Q), dtype=torch.int32, device=dev)
    hit = torch.empty((R, L + 1, Q), dtype=torch.float64, device=dev)
    ent = torch.empty(R, dtype=torch.float64, device=dev)
    wts = torch.empty((R, n), dtype=torch.float64, device=dev)
    q = torch.tensor(FRACTIONS, dtype=torch.float64, device=dev)
    t_tiles = torch.empty((R, Q), dtype=torch.int64, device=dev)
    t_hit = torch.empty((R, L + 1, Q), dtype=torch.float64, device=dev)

    def call():
        plan.spatial_coverage_device(mu.data_ptr(), mv.data_ptr(), U, T, window, window, L, FRACTIONS, tiles.data_ptr(), hit.data_ptr(),
                                     d_status=st.data_ptr(), stream=stream.cuda_stream)

    def windowed(weights=True):
        plan.spatial_windowed_device(mu.data_ptr(), mv.data_ptr(), U, T, window, window, ent.data_ptr(),
                                     d_weights=wts.data_ptr() if weights else 0, d_status=st.data_ptr(), stream=stream.cuda_stream)

    def today():
        windowed()
        with torch.cuda.stream(stream):
            h = wts.abs()
            srt, order = torch.sort(h, dim=1, descending=True, stable=True)
            C = torch.cumsum(srt, dim=1)
            Wr = C[:, -1]
            k = torch.searchsorted(C, q[None, :] * Wr[:, None]) + 1
            k = torch.where(Wr[:, None] > 0, k, torch.zeros_like(k))
            rank = torch.empty_like(order)
            rank.scatter_(1, order, torch.arange(n, device=dev).expand(R, n))
            tot = h.sum(dim=1)
            t_tiles.copy_(k)
            t_hit.fill_(float("nan"))
            for l in range(L + 1):
                m = R - l
                inside = rank[:m, None, :] < k[:m, :, None]                          # [m][Q][n]
                share = (h[l:, None, :] * inside).sum(dim=2) / tot[l:, None]
                bad = (Wr[:m] <= 0) | (tot[l:] <= 0)
                t_hit[:m, l] = torch.where(bad[:, None], torch.full_like(share, float("nan")), share)

    run = {"workload": name, "users": U, "frames": T, "tile_count": tc, "tiles": n, "window": window, "stride": window, "max_lag": L,
           "rows": R, "fractions": list(FRACTIONS)}
    for _ in range(WARMUP):
        call(); today(); windowed(False)
    torch.cuda.synchronize()
    ms_c, ms_t, ms_w = [], [], []
    for _ in range(REPS):
        ms_c.append(timed(stream, call))
        ms_t.append(timed(stream, today))
        ms_w.append(timed(stream, lambda: windowed(False)))
    eng.profile_enable(True); eng.profile_reset()
    call()
    eng.synchronize(); torch.cuda.synchronize()
    k = {x: round(eng.profile_get(x)[0], 4) for x in ("k_weights", "k_spatial", "k_finalize", "k_transition", "k_wtab")}
    eng.profile_enable(False)
    c_s, t_s, w_s = stats(ms_c), stats(ms_t), stats(ms_w)
    a, b = hit.cpu().numpy(), t_hit.cpu().numpy()
    ok = ~np.isnan(a) & ~np.isnan(b)
    run.update({"device_call": c_s, "today_windowed_plus_torch": t_s, "windowed_call_alone_no_weights": w_s,
                "kernels_ms": {"stage1_k_weights_gather": k["k_weights"], "stage1_k_window_tiles": k["k_spatial"],
                               "stage2_k_window_hist": k["k_finalize"], "stage3_k_coverage_rank": k["k_transition"],
                               "stage4_k_coverage_hits": k["k_wtab"]},
                "cost_on_top_of_the_windowed_call_ms": round(c_s["median_ms"] - w_s["median_ms"], 4),
                "speedup_median": round(t_s["median_ms"] / c_s["median_ms"], 3),
                "slower_than_today_by_more_than_its_spread": bool(c_s["median_ms"] - t_s["median_ms"] > t_s["max_ms"] - t_s["min_ms"]),
                "tiles_equal_today": bool(torch.equal(tiles.to(torch.int64), t_tiles)),
                "tiles_entries_differing": int((tiles.to(torch.int64) != t_tiles).sum()),
                "nan_positions_agree_with_today": bool(np.array_equal(np.isnan(a), np.isnan(b))),
                "max_abs_diff_hit_vs_today": float(np.max(np.abs(a[ok] - b[ok]))) if ok.any() else 0.0})
    plan.close()
    del mu, mv, tiles, hit, wts, t_hit, t_tiles
    torch.cuda.empty_cache()
    return run


def chain_probe(eng, dev, video):
    """What the sequential sum costs inside k_coverage_rank: 16 viewers x 30 000 frames on [500], window 1 (30 000 rows of 501 tiles),
    at fields of view that leave fewer and fewer positive tiles per row — the sort is the same, the sum stops behind the last
    positive weight.  Five profiled calls per field of view."""
    U, T = 16, video[0].shape[0]
    mu = torch.from_numpy(np.ascontiguousarray(video[0][:, :U])).to(dev); mv = torch.from_numpy(np.ascontiguousarray(video[1][:, :U])).to(dev)
    tiles = torch.empty((T, 4), dtype=torch.int32, device=dev)
    hit = torch.empty((T, 1, 4), dtype=torch.float64, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    out = []
    for fov in (120.0, 40.0, 10.0):
        plan = _native.Plan(eng, [_quantiser.lattice_xyz(500)], fov, 2.0, True, VW, VH)
        call = lambda: plan.spatial_coverage_device(mu.data_ptr(), mv.data_ptr(), U, T, 1, 1, 0, (0.5, 0.8, 0.95, 1.0), tiles.data_ptr(),
                                                    hit.data_ptr(), d_status=st.data_ptr())
        call(); eng.synchronize()
        ms = []
        eng.profile_enable(True)
        for _ in range(REPS):
            eng.profile_reset(); call(); eng.synchronize()
            ms.append(eng.profile_get("k_transition")[0])
        eng.profile_enable(False)
        out.append({"fov_angle": fov, "rows": T, "tiles": plan.n_tiles[0],
                    "positive_tiles_per_row_mean": round(tiles[:, 3].double().mean().item(), 2), "k_coverage_rank": stats(ms)})
        plan.close()
    return out


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    record = {"tool": "tools/coverage_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (tables built, workspace grown), the new "
                        "call, today's route and the windowed call alone alternating; median and min..max", "runs": []}
    videos = {}
    for name, U, T, tc, window, L in SHAPES:
        if (U, T) not in videos:
            videos[(U, T)] = bench.synth_video(U, T, 1234, 0)
        run = run_shape(eng, dev, stream, name, U, T, tc, window, L, videos[(U, T)])
        record["runs"].append(run)
        print(json.dumps(run), flush=True)
    record["rank_kernel_vs_positive_tiles"] = chain_probe(eng, dev, videos[(1024, 30000)])
    print(json.dumps(record["rank_kernel_vs_positive_tiles"]), flush=True)
    record["device"] = torch.cuda.get_device_name(0)
    record["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "coverage", "coverage_timing.json"))
