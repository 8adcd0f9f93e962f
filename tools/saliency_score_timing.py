"""Time of the saliency scoring (vet_saliency_score) on a 180 x 90 predicted map at sigma 5 degrees:
  config 3's shape (1024 viewers x 30 000 frames): window = stride = 20 with one predicted map per row (1 500 rows), window 1 with a
  static map (30 000 rows), the whole video with a static map; 512 x 10 000 at window 1 with a static map.
Each with the distribution metrics on and off.  Per shape the device call alone (direction ids and the predicted maps resident,
hipEvents on the launch stream; stats and counts, no map output: the audience's maps stay in the workspace), and today's route to the
same numbers alternating with it in the same run:
  today   vet_saliency_ids with d_map ([R][H][W] doubles) — not in the location-only mode — then torch on the device: the pixel sums
          of include/vet.h in row chunks under 1 GB, the bilinear sample of the predicted map at every sample (not the distinct
          directions) by index arithmetic and gathers, and for the AUC one torch.sort of the predicted map's rows and per map row two
          torch.searchsorted of all sample values, the area-weighted counts accumulated in ascending y.
After a warm-up; per side the median and the min..max spread of REPS single calls.  Nothing gates on a speed ratio: the JSON holds the
numbers, also where the new call does not win.  The per-kernel split comes from the engine's profile scopes in three profiled calls
of the new entry: with the distribution metrics (k_spatial = k_saliency_map + k_score_points), location only (k_spatial =
k_score_points alone) and counts only ("the rest" = stage 0 and the lists): k_saliency_map = k_spatial(distribution) -
k_spatial(location), sort + rows = k_transition - the rest.  k_score_points is also given as (list entry, map row) searches per
second: the list entries of the call times H over its time.  Also recorded: whether the counts agree and the largest disagreement
between the routes (auc, cc, sim, jsd absolute; the others relative over 1 + |value|; today's sums are torch's and its atan2 / acos
torch's).
usage: python tools/saliency_score_timing.py [out.json]      (default: profiles/saliency/saliency_score_timing.json)"""
import json
import math
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
MW, MH, SIGMA_DEG = 180, 90, 5.0
WARMUP, REPS = 1, 3
CHUNK_BYTES = 1 << 30
STATS = _native.SALIENCY_SCORE_STATS
ABS = (0, 3, 4, 5)
# (workload, users, frames, window (None = whole video), stride, one predicted map per row)
SHAPES = [("config3", 1024, 30000, 20, 20, True), ("config3", 1024, 30000, 1, 1, False), ("config3", 1024, 30000, None, 1, False),
          ("config5_shape", 512, 10000, 1, 1, False)]


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def cell_shares(dev):
    yy = torch.arange(MH, dtype=torch.float64, device=dev)
    return (torch.cos(math.pi * yy / MH) - torch.cos(math.pi * (yy + 1) / MH)) / (2 * MW)


def run_shape(eng, plan, unit, a_y, dev, stream, name, U, T, window, stride, per_row, ids, dist):
    window = T if window is None else window
    assert stride == window or window == T                       # today's route below takes each sample into one row
    R = (T - window) // stride + 1
    npix = MW * MH
    a_pix = a_y.repeat_interleave(MW)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    lat = torch.linspace(-1.0, 1.0, MH, dtype=torch.float64, device=dev)[:, None]
    pred = ((1.25 - lat * lat) * (0.5 + torch.rand(((R if per_row else 1), MH, MW), dtype=torch.float64, device=dev, generator=gen))).contiguous()
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.empty((9, R), dtype=torch.float64, device=dev)
    counts = torch.empty((2, R), dtype=torch.int64, device=dev)
    t_out = torch.full((9, R), float("nan"), dtype=torch.float64, device=dev)
    t_maps = torch.empty((R, npix), dtype=torch.float64, device=dev) if dist else None
    t_stats = torch.empty((4, R), dtype=torch.float64, device=dev)
    t_counts = torch.empty((2, R), dtype=torch.int64, device=dev)
    n_row = window * U
    rc_pix = max(1, CHUNK_BYTES // (npix * 8 * 8))              # rows per chunk of the pixel sums (about eight temporaries)
    rc_pts = max(1, CHUNK_BYTES // (n_row * 8 * 8))             # rows per chunk of the samples

    def call(d_stats=True, distribution=dist):
        plan.saliency_score_device(0, 0, U, T, window, stride, pred.data_ptr(), pred.shape[0], MW, MH, SIGMA_DEG, distribution,
                                   0, out.data_ptr() if d_stats else 0, counts.data_ptr(), st.data_ptr(), stream=stream.cuda_stream,
                                   d_ids=ids.data_ptr())

    def today():
        plan.saliency_device(0, 0, U, T, window, stride, False, SIGMA_DEG, MW, MH, "density", t_maps.data_ptr() if dist else 0,
                             t_stats.data_ptr() if dist else 0, 0, t_counts.data_ptr(), st.data_ptr(), stream=stream.cuda_stream,
                             d_ids=ids.data_ptr())
        with torch.cuda.stream(stream):
            zero = torch.zeros((), dtype=torch.float64, device=dev)
            P = pred.reshape(pred.shape[0], npix)
            mass_p = (P * a_pix).sum(dim=1)                      # [1] or [R]
            var_p = (a_pix * (P - mass_p[:, None]) ** 2).sum(dim=1)
            t_out[8] = mass_p
            if dist:
                mass = t_stats[0]
                for r0 in range(0, R, rc_pix):
                    r1 = min(R, r0 + rc_pix)
                    a, b = t_maps[r0:r1], (P[r0:r1] if per_row else P)
                    ma, mb = mass[r0:r1, None], (mass_p[r0:r1, None] if per_row else mass_p[:, None])
                    qa, qb = (a * a_pix) / ma, (b * a_pix) / mb
                    da, db = a - ma, b - mb
                    va, cov = (a_pix * (da * da)).sum(dim=1), (a_pix * (da * db)).sum(dim=1)
                    m = 0.5 * (qa + qb)
                    t_out[3, r0:r1] = cov / (va * (var_p[r0:r1] if per_row else var_p)).sqrt()
                    t_out[4, r0:r1] = torch.minimum(qa, qb).sum(dim=1)
                    t_out[5, r0:r1] = 0.5 * (torch.where(qa != 0, qa * torch.log2(qa / m), zero) +
                                             torch.where(qb != 0, qb * torch.log2(qb / m), zero)).sum(dim=1)
                    t_out[6, r0:r1] = torch.where(qa != 0, qa * torch.log2(qa / qb), zero).sum(dim=1)
                t_out[7] = mass
            srt = torch.sort(pred, dim=2).values                 # [1 or R][H][W]
            rows = ids[:R * window].reshape(R, n_row)
            for r0 in range(0, R, rc_pts):
                r1 = min(R, r0 + rc_pts)
                i = rows[r0:r1].long()
                on = (i >= 0).double()
                A = unit[i.clamp(min=0)]
                x, y, z = A[..., 0], A[..., 1], A[..., 2]
                lon = torch.where((x == 0) & (y == 0), zero, torch.atan2(y, x))
                fx = (lon + math.pi) / (2 * math.pi) * MW - 0.5
                c0f = torch.floor(fx)
                tx = fx - c0f
                c0 = c0f.long() % MW
                c1 = (c0 + 1) % MW
                fy = (torch.acos(z.clamp(-1.0, 1.0)) / math.pi * MH - 0.5).clamp(0.0, MH - 1.0)
                y0f = torch.floor(fy)
                ty = fy - y0f
                y0 = y0f.long()
                y1 = (y0 + 1).clamp(max=MH - 1)
                Pr = P[r0:r1] if per_row else P.expand(r1 - r0, npix)
                g = lambda yy, cc: torch.gather(Pr, 1, yy * MW + cc)
                top = g(y0, c0) + tx * (g(y0, c1) - g(y0, c0))
                bot = g(y1, c0) + tx * (g(y1, c1) - g(y1, c0))
                v = (top + ty * (bot - top)).contiguous()
                L, E = torch.zeros_like(v), torch.zeros_like(v)
                for yy in range(MH):
                    s = srt[r0:r1, yy] if per_row else srt[0, yy]
                    lo, hi = torch.searchsorted(s, v, right=False), torch.searchsorted(s, v, right=True)
                    L = L + a_y[yy] * lo.double()
                    E = E + a_y[yy] * (hi - lo).double()
                n = on.sum(dim=1)
                mp = mass_p[r0:r1] if per_row else mass_p
                t_out[0, r0:r1] = (on * (L + 0.5 * E)).sum(dim=1) / n
                t_out[1, r0:r1] = ((on * v).sum(dim=1) / n - mp) / (var_p[r0:r1] if per_row else var_p).sqrt()
                t_out[2, r0:r1] = torch.where(on != 0, torch.log2(v / mp[:, None]), zero).sum(dim=1) / n
            t_out[:8, t_counts[0] == 0] = float("nan")

    run = {"workload": name, "users": U, "frames": T, "window": window, "stride": stride, "rows": R, "map": [MW, MH], "sigma_deg": SIGMA_DEG,
           "predicted_maps": int(pred.shape[0]), "distribution": bool(dist), "today_rows_per_chunk": {"pixel_sums": rc_pix, "samples": rc_pts}}
    for _ in range(WARMUP):
        call(); today()
    torch.cuda.synchronize()
    ms_c, ms_t = [], []
    for _ in range(REPS):
        ms_c.append(timed(stream, call))
        ms_t.append(timed(stream, today))

    def profiled(fn):
        eng.profile_enable(True); eng.profile_reset()
        fn()
        eng.synchronize(); torch.cuda.synchronize()
        k = {x: eng.profile_get(x)[0] for x in ("k_spatial", "k_transition")}
        eng.profile_enable(False)
        return k

    k_new, k_loc, k_rest = profiled(call), profiled(lambda: call(True, False)), profiled(lambda: call(False))
    call()
    torch.cuda.synchronize()
    c_s, t_s = stats(ms_c), stats(ms_t)
    a, b = out.cpu().numpy(), t_out.cpu().numpy()
    worst = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, key in enumerate(STATS):
            fin = np.isfinite(a[k]) & np.isfinite(b[k])
            d = np.abs(a[k][fin] - b[k][fin])
            worst[key] = float((d if k in ABS else d / (1.0 + np.abs(b[k][fin]))).max(initial=0.0))
    entries = int(counts[1].sum().item())
    pts_ms = k_loc["k_spatial"]
    run.update({"device_call": c_s, "today_route": t_s,
                "kernels_ms": {"k_saliency_map": round(k_new["k_spatial"] - k_loc["k_spatial"], 4), "k_score_points": round(pts_ms, 4),
                               "k_score_sort_and_k_score_rows": round(k_new["k_transition"] - k_rest["k_transition"], 4),
                               "the_rest": round(k_rest["k_transition"], 4)},
                "profile_scopes_ms": {"new": k_new, "new_location_only": k_loc, "new_counts_only": k_rest},
                "samples": int(counts[0].sum().item()), "list_entries": entries,
                "k_score_points_searches_per_s": round(entries * MH / (pts_ms * 1e-3), 1) if pts_ms > 0 else None,
                "speedup_median": round(t_s["median_ms"] / c_s["median_ms"], 3),
                "slower_than_today_by_more_than_its_spread": bool(c_s["median_ms"] - t_s["median_ms"] > t_s["max_ms"] - t_s["min_ms"]),
                "counts_equal_today": bool(torch.equal(counts, t_counts)),
                "not_finite_in_the_same_places": bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))),
                "largest_disagreement_with_today": worst})
    del out, counts, t_out, t_maps, t_stats, t_counts, pred
    torch.cuda.empty_cache()
    return run


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(50)], 120.0, 2.0, True, VW, VH)
    raw = torch.from_numpy(plan.read_dirs()).to(dev)
    unit = raw / raw.pow(2).sum(dim=1, keepdim=True).sqrt()
    a_y = cell_shares(dev)
    record = {"tool": "tools/saliency_score_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (workspace grown), the new call and today's "
                        "route alternating; median and min..max", "runs": []}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    ids_of = {}
    for name, U, T, window, stride, per_row in SHAPES:
        if (U, T) not in ids_of:
            ids_of.clear()
            mu, mv = bench.synth_video(U, T, 1234, 0)
            px, py = np.minimum((mu * VW).astype(np.int64), VW), np.minimum((mv * VH).astype(np.int64), VH)
            ids_of[(U, T)] = torch.from_numpy((py * (VW + 1) + px).astype(np.int32)).to(dev)
        for dist in (True, False):
            run = run_shape(eng, plan, unit, a_y, dev, stream, name, U, T, window, stride, per_row, ids_of[(U, T)], dist)
            record["runs"].append(run)
            print(json.dumps(run), flush=True)
            record["device"] = torch.cuda.get_device_name(0)
            record["date"] = time.strftime("%Y-%m-%d")
            with open(out_path, "w") as f_out:                   # after every run: a record of what has run
                json.dump(record, f_out, indent=1)
    plan.close()
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "saliency", "saliency_score_timing.json"))
