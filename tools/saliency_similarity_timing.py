"""Time of the saliency similarity (vet_saliency_similarity) on a 180 x 90 map at sigma 5 degrees with balanced random groups:
  config 3's shape (1024 viewers x 30 000 frames): window = stride = 20 (1 500 rows), window 1 (30 000 rows), the whole video;
  512 x 10 000 at window 1.
Per shape the device call alone (direction ids resident, hipEvents on the launch stream; stats and counts, no maps: they stay in the
workspace), and today's route to the same numbers alternating with it in the same run:
  today   the ids masked per audience (torch.where), two vet_saliency_ids calls with d_map (2 x [R][H][W] doubles), then torch on
          the device: the pixel sums of include/vet.h in row chunks under 1 GB, and the point evaluation by gather, a batched matmul of
          the two audiences' unit vectors and exp(kappa (c - 1)) in chunks under 1 GB (every sample, not the distinct directions; the
          one matrix serves both directions) — for the whole video torch.bincount of the ids and the kernel matrix of the directions in
          row chunks.
After a warm-up; per side the median and the min..max spread of REPS single calls.  Nothing gates on a speed ratio: the JSON holds the
numbers, also where the new call does not win.  The per-kernel split comes from the engine's profile scopes (k_spatial = k_saliency_map
+ k_saliency_points, k_transition = the other stages) in three profiled calls: the new call, the new call with counts only (no map,
no points, a trivial comparison: "the rest" = stage 0, the mask, the lists) and today's two saliency calls (their k_spatial is the
same two map launches): k_saliency_points = k_spatial(new) - k_spatial(today), k_saliency_compare = k_transition(new) - the rest.
Also recorded: whether the counts agree and the largest disagreement between the routes (cc, sim, jsd absolute; kl, nss, mass
relative over 1 + |value|; today's dot is a matmul, not the fused dot, and its sums are torch's).
usage: python tools/saliency_similarity_timing.py [out.json]      (default: profiles/saliency/saliency_similarity_timing.json)"""
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
STATS = _native.SALIENCY_SIMILARITY_STATS
# (workload, users, frames, window (None = whole video), stride)
SHAPES = [("config3", 1024, 30000, 20, 20), ("config3", 1024, 30000, 1, 1), ("config3", 1024, 30000, None, 1),
          ("config5_shape", 512, 10000, 1, 1)]


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
    a = (torch.cos(math.pi * yy / MH) - torch.cos(math.pi * (yy + 1) / MH)) / (2 * MW)
    return a.repeat_interleave(MW)


def run_shape(eng, plan, unit, a_pix, dev, stream, name, U, T, window, stride, ids, code):
    window = T if window is None else window
    assert stride == window or window == T                       # today's route below takes each sample into one row
    R = (T - window) // stride + 1
    npix = MW * MH
    sigma = math.radians(SIGMA_DEG)
    kappa = 1.0 / (sigma * sigma)
    C = kappa / (2.0 * math.pi * (1.0 - math.exp(-2.0 * kappa)))
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.empty((9, R), dtype=torch.float64, device=dev)
    counts = torch.empty((4, R), dtype=torch.int64, device=dev)
    t_out = torch.empty((9, R), dtype=torch.float64, device=dev)
    t_maps = torch.empty((2, R, npix), dtype=torch.float64, device=dev)
    t_stats = torch.empty((2, 4, R), dtype=torch.float64, device=dev)
    t_counts = torch.empty((2, 2, R), dtype=torch.int64, device=dev)
    t_ids = torch.empty((2,) + tuple(ids.shape), dtype=torch.int32, device=dev)
    label = torch.from_numpy(code.astype(np.int64)).to(dev)
    cols = [torch.nonzero(label == g).reshape(-1) for g in (0, 1)]
    absent = torch.full((), -1, dtype=torch.int32, device=dev)
    rc_pix = max(1, CHUNK_BYTES // (npix * 8 * 8))              # rows per chunk of the pixel sums (about eight temporaries)
    n_x, n_y = window * len(cols[0]), window * len(cols[1])
    rc_pts = max(1, CHUNK_BYTES // (n_x * n_y * 8))

    def call(d_stats=True):
        plan.saliency_similarity_device(0, 0, U, T, window, stride, code, SIGMA_DEG, MW, MH, 0, out.data_ptr() if d_stats else 0,
                                        counts.data_ptr(), st.data_ptr(), stream=stream.cuda_stream, d_ids=ids.data_ptr())

    def today_maps():
        with torch.cuda.stream(stream):
            for g in (0, 1):
                torch.where((label == g)[None, :], ids, absent, out=t_ids[g])
        for g in (0, 1):
            plan.saliency_device(0, 0, U, T, window, stride, False, SIGMA_DEG, MW, MH, "density", t_maps[g].data_ptr(),
                                 t_stats[g].data_ptr(), 0, t_counts[g].data_ptr(), st.data_ptr(), stream=stream.cuda_stream,
                                 d_ids=t_ids[g].data_ptr())

    def today():
        today_maps()
        with torch.cuda.stream(stream):
            mass = t_stats[:, 0]
            for r0 in range(0, R, rc_pix):
                r1 = min(R, r0 + rc_pix)
                a, b = t_maps[0, r0:r1], t_maps[1, r0:r1]
                ma, mb = mass[0, r0:r1, None], mass[1, r0:r1, None]
                qa, qb = (a * a_pix) / ma, (b * a_pix) / mb
                da, db = a - ma, b - mb
                va, vb, cov = (a_pix * (da * da)).sum(dim=1), (a_pix * (db * db)).sum(dim=1), (a_pix * (da * db)).sum(dim=1)
                m = 0.5 * (qa + qb)
                zero = torch.zeros((), dtype=torch.float64, device=dev)
                t_out[0, r0:r1] = cov / (va * vb).sqrt()
                t_out[1, r0:r1] = torch.minimum(qa, qb).sum(dim=1)
                t_out[2, r0:r1] = 0.5 * (torch.where(qa != 0, qa * torch.log2(qa / m), zero) +
                                         torch.where(qb != 0, qb * torch.log2(qb / m), zero)).sum(dim=1)
                t_out[3, r0:r1] = torch.where(qa != 0, qa * torch.log2(qa / qb), zero).sum(dim=1)
                t_out[4, r0:r1] = torch.where(qb != 0, qb * torch.log2(qb / qa), zero).sum(dim=1)
                t_out[5, r0:r1], t_out[6, r0:r1] = vb.sqrt(), va.sqrt()          # the deviations: the point values are centred below
            t_out[7], t_out[8] = mass[0], mass[1]
            n = t_counts[:, 0].double()
            if R == 1:                                           # the whole video: the counts per direction, the kernel matrix of the directions
                cnt = [torch.bincount(i[i >= 0], minlength=unit.shape[0]).double() for i in (ids[:, c].reshape(-1).long() for c in cols)]
                used = [torch.nonzero(c).reshape(-1) for c in cnt]
                V = torch.zeros(2, dtype=torch.float64, device=dev)
                step = max(1, CHUNK_BYTES // (len(used[1]) * 8))
                for i0 in range(0, len(used[0]), step):
                    ia = used[0][i0:i0 + step]
                    K = torch.exp(kappa * (unit[ia] @ unit[used[1]].t() - 1.0))
                    V[0] += (cnt[0][ia] * (K @ cnt[1][used[1]])).sum()
                    V[1] += (cnt[1][used[1]] * (cnt[0][ia] @ K)).sum()
                V = V[:, None]
            else:
                V = torch.empty((2, R), dtype=torch.float64, device=dev)
                rows = [ids[:R * window][:, c].reshape(R, -1) for c in cols]
                for r0 in range(0, R, rc_pts):
                    r1 = min(R, r0 + rc_pts)
                    ia, ib = rows[0][r0:r1].long(), rows[1][r0:r1].long()
                    oa, ob = (ia >= 0).double(), (ib >= 0).double()
                    K = torch.exp(kappa * (torch.bmm(unit[ia.clamp(min=0)], unit[ib.clamp(min=0)].transpose(1, 2)) - 1.0))
                    V[0, r0:r1] = (oa * torch.bmm(K, ob[:, :, None])[:, :, 0]).sum(dim=1)
                    V[1, r0:r1] = (ob * torch.bmm(oa[:, None, :], K)[:, 0, :]).sum(dim=1)
            t_out[5] = (V[0] * (C / n[1]) / n[0] - mass[1]) / t_out[5]
            t_out[6] = (V[1] * (C / n[0]) / n[1] - mass[0]) / t_out[6]
            empty = (n[0] == 0) | (n[1] == 0)
            t_out[:7, empty] = float("nan")

    run = {"workload": name, "users": U, "frames": T, "window": window, "stride": stride, "rows": R, "map": [MW, MH], "sigma_deg": SIGMA_DEG,
           "audiences": [int((code == 0).sum()), int((code == 1).sum())], "today_rows_per_chunk": {"pixel_sums": rc_pix, "points": rc_pts}}
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

    k_new, k_rest, k_today = profiled(call), profiled(lambda: call(False)), profiled(today_maps)
    call()
    torch.cuda.synchronize()
    c_s, t_s = stats(ms_c), stats(ms_t)
    a, b = out.cpu().numpy(), t_out.cpu().numpy()
    worst = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, key in enumerate(STATS):
            fin = np.isfinite(a[k]) & np.isfinite(b[k])
            d = np.abs(a[k][fin] - b[k][fin])
            worst[key] = float((d if k < 3 else d / (1.0 + np.abs(b[k][fin]))).max(initial=0.0))
    run.update({"device_call": c_s, "today_route": t_s,
                "kernels_ms": {"k_saliency_map": round(k_today["k_spatial"], 4),
                               "k_saliency_points": round(k_new["k_spatial"] - k_today["k_spatial"], 4),
                               "k_saliency_compare": round(k_new["k_transition"] - k_rest["k_transition"], 4),
                               "the_rest": round(k_rest["k_transition"], 4)},
                "profile_scopes_ms": {"new": k_new, "new_counts_only": k_rest, "today_two_saliency_calls": k_today},
                "samples": [int(counts[0].sum().item()), int(counts[1].sum().item())],
                "list_entries": [int(counts[2].sum().item()), int(counts[3].sum().item())],
                "speedup_median": round(t_s["median_ms"] / c_s["median_ms"], 3),
                "slower_than_today_by_more_than_its_spread": bool(c_s["median_ms"] - t_s["median_ms"] > t_s["max_ms"] - t_s["min_ms"]),
                "counts_equal_today": bool(torch.equal(counts[:2], t_counts[:, 0]) and torch.equal(counts[2:], t_counts[:, 1])),
                "not_finite_in_the_same_places": bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))),
                "largest_disagreement_with_today": worst})
    del out, counts, t_out, t_maps, t_stats, t_counts, t_ids
    torch.cuda.empty_cache()
    return run


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(50)], 120.0, 2.0, True, VW, VH)
    raw = torch.from_numpy(plan.read_dirs()).to(dev)
    unit = raw / raw.pow(2).sum(dim=1, keepdim=True).sqrt()
    a_pix = cell_shares(dev)
    record = {"tool": "tools/saliency_similarity_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (workspace grown), the new call and today's "
                        "route alternating; median and min..max", "runs": []}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    ids_of = {}
    for name, U, T, window, stride in SHAPES:
        if (U, T) not in ids_of:
            ids_of.clear()
            mu, mv = bench.synth_video(U, T, 1234, 0)
            px, py = np.minimum((mu * VW).astype(np.int64), VW), np.minimum((mv * VH).astype(np.int64), VH)
            ids_of[(U, T)] = torch.from_numpy((py * (VW + 1) + px).astype(np.int32)).to(dev)
        code = (np.random.default_rng(7).permutation(U) % 2).astype(np.int8)          # balanced random groups
        run = run_shape(eng, plan, unit, a_pix, dev, stream, name, U, T, window, stride, ids_of[(U, T)], code)
        record["runs"].append(run)
        print(json.dumps(run), flush=True)
        record["device"] = torch.cuda.get_device_name(0)
        record["date"] = time.strftime("%Y-%m-%d")
        with open(out_path, "w") as f_out:                       # after every shape: a record of what has run
            json.dump(record, f_out, indent=1)
    plan.close()
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "saliency", "saliency_similarity_timing.json"))
