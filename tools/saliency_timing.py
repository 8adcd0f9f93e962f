"""Time of the saliency maps (vet_saliency) on a 180 x 90 map at sigma 5 degrees, scale "density":
  config 3's shape (1024 viewers x 30 000 frames), pooled: window = stride = 20 (1 500 rows) with the maps; window 1 (30 000 rows),
      statistics only; the whole video; per viewer: window = stride = 20 (1.5 M rows), statistics only;
  512 x 10 000 pooled at window 1, statistics only.
Per shape the device call alone (direction ids resident, hipEvents on the launch stream; stats, peak, counts and where stated the
maps), its per-kernel split from the engine's profile scopes (k_saliency_map = k_spatial, the other stages = k_transition) with the
map kernel's kernel evaluations per second (pixels x the row's distinct directions, summed over the rows), and today's route to the
same numbers alternating with the new call in the same run — torch on the device, so it is the same code before and after this call
existed:
  today   the rows in chunks whose [rows][samples][pixels] FP64 array stays under 1 GB (a row too long for that in chunks of its
          samples): the unit vectors gathered from the direction table, a matmul with the cell directions, exp(kappa (c - 1)),
          absent samples masked, the sum over the row's samples; the whole-video row from torch.bincount of the ids and one matmul
          with the counts; then C / N, and mass, peak, argmax, entropy and area by torch reductions.  Every sample is evaluated:
          the route does not collapse a row to its distinct directions.
After a warm-up; per side the median and the min..max spread of REPS single calls.  Nothing gates on a speed ratio: the JSON holds the
numbers, also where the new call does not win.  Also recorded: whether the sample counts agree and the largest relative disagreement
between the routes' statistics (today's dot is a matmul, not the fused dot, its sums are torch's and its sines and cosines the
device's), and — from one run of the numpy oracle of tests/_saliency_oracle.py on golden G15's video, the GPU tests' input — the
largest deviations of the new call from the oracle.
usage: python tools/saliency_timing.py [out.json]      (default: profiles/saliency/saliency_timing.json)"""
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
# (workload, users, frames, window (None = whole video), stride, per_user, with the maps)
SHAPES = [("config3", 1024, 30000, 20, 20, False, True), ("config3", 1024, 30000, 1, 1, False, False),
          ("config3", 1024, 30000, None, 1, False, False), ("config3", 1024, 30000, 20, 20, True, False),
          ("config5_shape", 512, 10000, 1, 1, False, False)]


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def cell_tables(dev):
    """(P [npix][3], a [npix]) of the map on the device: today's route takes its sines and cosines from torch"""
    lon = (torch.arange(MW, dtype=torch.float64, device=dev) + 0.5) / MW * 360.0 - 180.0
    lat = 90.0 - (torch.arange(MH, dtype=torch.float64, device=dev) + 0.5) / MH * 180.0
    theta, phi = torch.deg2rad(lon), torch.deg2rad(90.0 - lat)
    x = torch.sin(phi)[:, None] * torch.cos(theta)[None, :]
    y = torch.sin(phi)[:, None] * torch.sin(theta)[None, :]
    z = torch.cos(phi)[:, None].expand(MH, MW)
    P = torch.stack([x, y, z], dim=-1).reshape(-1, 3)
    P = P / P.pow(2).sum(dim=1, keepdim=True).sqrt()
    yy = torch.arange(MH, dtype=torch.float64, device=dev)
    a = (torch.cos(math.pi * yy / MH) - torch.cos(math.pi * (yy + 1) / MH)) / (2 * MW)
    return P.contiguous(), a.repeat_interleave(MW)


def run_shape(eng, plan, unit, P, a_pix, dev, stream, name, U, T, window, stride, per_user, with_maps, ids):
    window = T if window is None else window
    assert stride == window or window == T                       # today's route below takes each sample into one row
    R = (T - window) // stride + 1
    rows = U * R if per_user else R
    npix = MW * MH
    sigma = math.radians(SIGMA_DEG)
    kappa = 1.0 / (sigma * sigma)
    C = kappa / (2.0 * math.pi * (1.0 - math.exp(-2.0 * kappa)))
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.empty((4, rows), dtype=torch.float64, device=dev)
    peak = torch.empty(rows, dtype=torch.int32, device=dev)
    counts = torch.empty((2, rows), dtype=torch.int64, device=dev)
    maps = torch.empty((rows, MH, MW), dtype=torch.float64, device=dev) if with_maps else None
    t_stats = torch.empty((4, rows), dtype=torch.float64, device=dev)
    t_peak = torch.empty(rows, dtype=torch.int64, device=dev)
    t_n = torch.empty(rows, dtype=torch.int64, device=dev)
    t_maps = torch.empty((rows, npix), dtype=torch.float64, device=dev) if with_maps else None
    wpos = window if per_user else window * U
    row_ids = (ids.t()[:, :R * window].reshape(rows, wpos) if per_user else ids[:R * window].reshape(rows, wpos)).contiguous()
    rc = max(1, CHUNK_BYTES // (wpos * npix * 8))
    sc = max(1, CHUNK_BYTES // (npix * 8))                      # samples per chunk of a row too long for one

    def call():
        plan.saliency_device(0, 0, U, T, window, stride, per_user, SIGMA_DEG, MW, MH, "density", maps.data_ptr() if with_maps else 0,
                             out.data_ptr(), peak.data_ptr(), counts.data_ptr(), st.data_ptr(), stream=stream.cuda_stream,
                             d_ids=ids.data_ptr())

    def finish(S, n, r0, r1):
        M = S * (C / n.double())[:, None]
        w = M * a_pix[None, :]
        mass = w.sum(dim=1)
        q = w / mass[:, None]
        t = torch.where(w > 0, q * torch.log2(q / a_pix[None, :]), torch.zeros_like(q))
        ent = -t.sum(dim=1)
        t_stats[0, r0:r1], t_stats[1, r0:r1], t_stats[2, r0:r1], t_stats[3, r0:r1] = mass, M.amax(dim=1), ent, torch.exp2(ent)
        t_peak[r0:r1] = M.argmax(dim=1)
        t_n[r0:r1] = n
        if with_maps:
            t_maps[r0:r1] = M

    def today():
        with torch.cuda.stream(stream):
            if rows == 1:                                        # the whole video: the counts per direction, one matmul
                idc = row_ids[0].long()
                cnt = torch.bincount(idc[idc >= 0], minlength=unit.shape[0]).double()
                K = torch.exp(kappa * (P @ unit.t() - 1.0))
                finish((K @ cnt)[None, :], cnt.sum().long()[None], 0, 1)
            elif wpos * npix * 8 <= CHUNK_BYTES:
                for r0 in range(0, rows, rc):
                    r1 = min(rows, r0 + rc)
                    idc = row_ids[r0:r1].long()
                    ok = idc >= 0
                    K = torch.exp(kappa * (torch.matmul(unit[idc.clamp(min=0)], P.t()) - 1.0))          # [rc][wpos][npix]
                    finish((K * ok[:, :, None]).sum(dim=1), ok.sum(dim=1), r0, r1)
            else:
                for r in range(rows):
                    S = torch.zeros(npix, dtype=torch.float64, device=dev)
                    n = torch.zeros((), dtype=torch.int64, device=dev)
                    for s0 in range(0, wpos, sc):
                        idc = row_ids[r, s0:s0 + sc].long()
                        ok = idc >= 0
                        K = torch.exp(kappa * (unit[idc.clamp(min=0)] @ P.t() - 1.0))                 # [sc][npix]
                        S += (K * ok[:, None]).sum(dim=0)
                        n += ok.sum()
                    finish(S[None, :], n[None], r, r + 1)

    run = {"workload": name, "users": U, "frames": T, "window": window, "stride": stride, "per_user": per_user, "rows": rows,
           "map": [MW, MH], "sigma_deg": SIGMA_DEG, "with_maps": with_maps, "today_rows_per_chunk": rc if wpos * npix * 8 <= CHUNK_BYTES else 0}
    for _ in range(WARMUP):
        call(); today()
    torch.cuda.synchronize()
    ms_c, ms_t = [], []
    for _ in range(REPS):
        ms_c.append(timed(stream, call))
        ms_t.append(timed(stream, today))
    eng.profile_enable(True); eng.profile_reset()
    call()
    eng.synchronize(); torch.cuda.synchronize()
    k = {x: round(eng.profile_get(x)[0], 4) for x in ("k_spatial", "k_transition")}
    eng.profile_enable(False)
    c_s, t_s = stats(ms_c), stats(ms_t)
    evaluations = float(counts[1].sum().item()) * npix
    a, b = out.cpu().numpy(), t_stats.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = lambda x, y: float(np.nanmax(np.abs(x - y) / np.where(y == 0, 1.0, np.abs(y)), initial=0.0))
        run.update({"device_call": c_s, "today_torch_route": t_s,
                    "kernels_ms": {"k_saliency_map": k["k_spatial"], "other_stages": k["k_transition"]},
                    "samples": int(counts[0].sum().item()), "list_entries": int(counts[1].sum().item()),
                    "kernel_evaluations": evaluations, "today_kernel_evaluations": float(counts[0].sum().item()) * npix,
                    "map_kernel_evaluations_per_s": round(evaluations / (k["k_spatial"] * 1e-3), 1) if k["k_spatial"] > 0 else None,
                    "speedup_median": round(t_s["median_ms"] / c_s["median_ms"], 3),
                    "slower_than_today_by_more_than_its_spread": bool(c_s["median_ms"] - t_s["median_ms"] > t_s["max_ms"] - t_s["min_ms"]),
                    "samples_equal_today": bool(torch.equal(counts[0], t_n)),
                    "peak_index_differs_from_today_in_rows": int((peak.long() != t_peak).sum().item()),
                    "max_rel_diff_vs_today": {"mass": rel(a[0], b[0]), "peak": rel(a[1], b[1]), "area": rel(a[3], b[3])},
                    "max_abs_diff_vs_today": {"entropy_bits": float(np.nanmax(np.abs(a[2] - b[2]), initial=0.0))}})
        if with_maps:
            m_a, m_b = maps.reshape(rows, npix), t_maps
            big = m_b > 1e-300
            run["max_rel_diff_vs_today"]["map"] = float(((m_a - m_b).abs()[big] / m_b[big]).max().item())
    del out, peak, counts, maps, t_stats, t_peak, t_n, t_maps, row_ids
    torch.cuda.empty_cache()
    return run


def oracle_deviations(plan):
    """the new call against the numpy oracle on the GPU tests' input (golden G15's video, moved off the centre)"""
    from tests import _saliency_oracle as so
    g = np.load(os.path.join(ROOT, "tests", "golden", "g15_windowed_transition.npz"))
    mu, mv = so.off_centre(g["mu"], g["mv"])
    ids = so.ids_of(mu, mv, VW, VH)
    table = so.grid_table(VW, VH)
    worst = {"map_rel": 0.0, "mass_rel": 0.0, "peak_rel": 0.0, "area_rel": 0.0, "entropy_abs_bits": 0.0}
    for mw, mh, sigma, window in ((36, 18, 5.0, 5), (36, 18, 2.0, 1), (18, 9, 10.0, 60), (37, 19, 1.0, 5), (36, 18, 0.5, 5), (36, 18, 180.0, 5)):
        o = so.Oracle(table, mw, mh)
        for per_user in (False, True):
            got = plan.saliency(ids=ids, window=window, stride=1, per_user=per_user, sigma_deg=sigma, width=mw, height=mh)
            want = o.rows(ids, window, 1, min(math.radians(sigma), math.pi), 2, per_user)
            ok = want["counts"][0] > 0
            big = want["map"] > 2.0 ** -900
            with np.errstate(invalid="ignore", divide="ignore"):
                worst["map_rel"] = max(worst["map_rel"], float(np.max(np.abs(got["map"] - want["map"])[big] / want["map"][big], initial=0.0)))
                for k, key in ((0, "mass_rel"), (1, "peak_rel"), (3, "area_rel")):
                    worst[key] = max(worst[key], float(np.max(np.abs(got["stats"][k][ok] - want["stats"][k][ok]) / want["stats"][k][ok], initial=0.0)))
                worst["entropy_abs_bits"] = max(worst["entropy_abs_bits"], float(np.max(np.abs(got["stats"][2][ok] - want["stats"][2][ok]), initial=0.0)))
            assert np.array_equal(got["counts"], want["counts"])
    return worst


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(50)], 120.0, 2.0, True, VW, VH)
    raw = torch.from_numpy(plan.read_dirs()).to(dev)
    unit = raw / raw.pow(2).sum(dim=1, keepdim=True).sqrt()
    P, a_pix = cell_tables(dev)
    record = {"tool": "tools/saliency_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (workspace grown), the new call and today's "
                        "route alternating; median and min..max",
              "largest_deviations_from_the_numpy_oracle": oracle_deviations(plan), "runs": []}
    print(json.dumps(record["largest_deviations_from_the_numpy_oracle"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    ids_of = {}
    for name, U, T, window, stride, per_user, with_maps in SHAPES:
        if (U, T) not in ids_of:
            ids_of.clear()
            mu, mv = bench.synth_video(U, T, 1234, 0)
            px, py = np.minimum((mu * VW).astype(np.int64), VW), np.minimum((mv * VH).astype(np.int64), VH)
            ids_of[(U, T)] = torch.from_numpy((py * (VW + 1) + px).astype(np.int32)).to(dev)
        run = run_shape(eng, plan, unit, P, a_pix, dev, stream, name, U, T, window, stride, per_user, with_maps, ids_of[(U, T)])
        record["runs"].append(run)
        print(json.dumps(run), flush=True)
        record["device"] = torch.cuda.get_device_name(0)
        record["date"] = time.strftime("%Y-%m-%d")
        with open(out_path, "w") as f_out:                       # after every shape: a record of what has run
            json.dump(record, f_out, indent=1)
    plan.close()
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "saliency", "saliency_timing.json"))
