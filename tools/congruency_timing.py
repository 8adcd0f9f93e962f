"""Time of the viewer congruency (vet_congruency) at sigma 5 degrees:
  config 3's shape (1024 viewers x 30 000 frames): window = stride = 20 (1 500 rows), window 1 (30 000 rows), the whole video;
  512 x 10 000 at window 1.
Per shape the device call alone (direction ids resident, hipEvents on the launch stream; stats, counts and rows), with nss and
without, and today's route to lift and info_gain alternating with it in the same run:
  today   torch on the device, per sample and not per distinct direction: the rows' ids gathered into unit vectors, a batched matmul
          of a row's samples with themselves, exp(kappa (c - 1)), and a masked sum that leaves out the viewer's own column, in chunks
          under 1 GB (rows, or blocks of a row's samples where one row is larger) — for the whole video the counts per (viewer,
          direction) by index_put, the kernel matrix of the used directions in row chunks and one matmul with the leave-one-out
          weights m - a (the kernel is evaluated once per pair of directions there, not once per viewer that holds one: the
          formulation that wins where every viewer holds most directions).
  nss     has no torch route short of the maps: NSS_VIEWERS viewers through saliency_similarity_device with {u} against the rest on
          a 180 x 90 map, one call each; reported per viewer and scaled to all viewers.
After a warm-up; per side the median and the min..max spread of REPS single calls (one call for the whole video).  Nothing gates on a
speed ratio: the JSON holds the numbers, also where the new call does not win.  k_congruency_points alone comes from the engine's
profile scopes (k_spatial holds nothing else in this call); its pair evaluations are sum over rows of (the viewers' own entries) x
(the pooled list), from the call's counts and vet_saliency's pooled counts.
usage: python tools/congruency_timing.py [out.json] [first shape] [shapes]     (default: profiles/saliency/congruency_timing.json)"""
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
SIGMA_DEG = 5.0
WARMUP, REPS = 1, 3
CHUNK_BYTES = 1 << 30
NSS_VIEWERS = 2
# (workload, users, frames, window (None = whole video), stride)
SHAPES = [("config3", 1024, 30000, 20, 20), ("config3", 1024, 30000, 1, 1), ("config5_shape", 512, 10000, 1, 1),
          ("config3", 1024, 30000, None, 1)]


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def run_shape(eng, plan, unit, dev, stream, name, U, T, window, stride, ids):
    whole = window is None
    window = T if whole else window
    assert stride == window or whole                             # today's route below takes each sample into one row
    R = (T - window) // stride + 1
    reps = 1 if whole else REPS
    sigma = math.radians(SIGMA_DEG)
    kappa = 1.0 / (sigma * sigma)
    C = kappa / (2.0 * math.pi * (1.0 - math.exp(-2.0 * kappa)))
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.empty((3, U, R), dtype=torch.float64, device=dev)
    counts = torch.empty((3, U, R), dtype=torch.int64, device=dev)
    rows = torch.empty((4, R), dtype=torch.float64, device=dev)
    t_out = torch.full((2, U, R), float("nan"), dtype=torch.float64, device=dev)
    pooled = torch.empty((2, R), dtype=torch.int64, device=dev)

    def call(nss=True):
        plan.congruency_device(0, 0, U, T, window, stride, SIGMA_DEG, nss, out.data_ptr(), counts.data_ptr(), rows.data_ptr(),
                               st.data_ptr(), stream=stream.cuda_stream, d_ids=ids.data_ptr())

    def today_rows():
        n = window * U
        viewer = torch.arange(U, device=dev).repeat(window)      # the viewer of a row's position
        rc = max(1, CHUNK_BYTES // (n * n * 8 * 3))
        qb = n if rc > 1 or n * n * 8 * 3 <= CHUNK_BYTES else max(1, CHUNK_BYTES // (n * 8 * 3))
        for r0 in range(0, R, rc):
            r1 = min(R, r0 + rc)
            i = ids[r0 * window:r1 * window].reshape(r1 - r0, n).long()
            ok = i >= 0
            X = unit[i.clamp(min=0)]
            n_u = torch.zeros((r1 - r0, U), dtype=torch.float64, device=dev).index_add_(1, viewer, ok.double())
            others = n_u.sum(dim=1, keepdim=True) - n_u
            F = torch.zeros((r1 - r0, U), dtype=torch.float64, device=dev)
            L = torch.zeros((r1 - r0, U), dtype=torch.float64, device=dev)
            for q0 in range(0, n, qb):
                q1 = min(n, q0 + qb)
                K = torch.exp(kappa * (torch.bmm(X[:, q0:q1], X.transpose(1, 2)) - 1.0))
                K = K * (ok[:, None, :] & (viewer[q0:q1, None] != viewer[None, :])[None])
                f = K.sum(dim=2) * (C / others[:, viewer[q0:q1]])
                okq = ok[:, q0:q1].double()
                F.index_add_(1, viewer[q0:q1], torch.where(ok[:, q0:q1], f, torch.zeros_like(f)))
                L.index_add_(1, viewer[q0:q1], torch.where(ok[:, q0:q1], torch.log2(4.0 * math.pi * f), torch.zeros_like(f)) * okq)
            t_out[0, :, r0:r1] = (4.0 * math.pi * F / n_u).t()
            t_out[1, :, r0:r1] = (L / n_u).t()

    def today_whole():
        D = unit.shape[0]
        viewer = torch.arange(U, device=dev)[None, :].expand(T, U).reshape(-1)
        i = ids.reshape(-1).long()
        ok = i >= 0
        A = torch.zeros((U, D), dtype=torch.float64, device=dev)
        A.index_put_((viewer[ok], i[ok]), torch.ones((), dtype=torch.float64, device=dev), accumulate=True)
        m = A.sum(dim=0)
        used = torch.nonzero(m).reshape(-1)
        A, m = A[:, used], m[used]
        Wt = m[None, :] - A
        n_u = A.sum(dim=1)
        g = C / (m.sum() - n_u)
        F = torch.zeros(U, dtype=torch.float64, device=dev)
        L = torch.zeros(U, dtype=torch.float64, device=dev)
        step = max(1, CHUNK_BYTES // (len(used) * 8 * 2))
        for i0 in range(0, len(used), step):
            Xq = unit[used[i0:i0 + step]]
            K = torch.exp(kappa * (Xq @ unit[used].t() - 1.0))
            f = (Wt @ K.t()) * g[:, None]                        # [U][block]: the others' density at the block's directions
            a = A[:, i0:i0 + step]
            F += (a * f).sum(dim=1)
            L += torch.where(a > 0, a * torch.log2(4.0 * math.pi * f), torch.zeros_like(f)).sum(dim=1)
        t_out[0, :, 0] = 4.0 * math.pi * F / n_u
        t_out[1, :, 0] = L / n_u

    def today():
        with torch.cuda.stream(stream):
            today_whole() if whole else today_rows()

    sim_stats = torch.empty((9, R), dtype=torch.float64, device=dev)

    def nss_today(u):
        code = np.ones(U, dtype=np.int8)
        code[u] = 0
        plan.saliency_similarity_device(0, 0, U, T, window, stride, code, SIGMA_DEG, 180, 90, 0, sim_stats.data_ptr(), 0, st.data_ptr(),
                                        stream=stream.cuda_stream, d_ids=ids.data_ptr())

    run = {"workload": name, "users": U, "frames": T, "window": window, "stride": stride, "rows": R, "sigma_deg": SIGMA_DEG}
    for _ in range(WARMUP):
        call(True); call(False); today(); nss_today(0)
    torch.cuda.synchronize()
    ms_n, ms_c, ms_t, ms_s = [], [], [], []
    for k in range(reps):
        ms_n.append(timed(stream, lambda: call(True)))
        ms_c.append(timed(stream, lambda: call(False)))
        ms_t.append(timed(stream, today))
    for u in range(NSS_VIEWERS):
        ms_s.append(timed(stream, lambda: nss_today(u)))

    def profiled(fn):
        eng.profile_enable(True); eng.profile_reset()
        fn()
        eng.synchronize(); torch.cuda.synchronize()
        k = {x: eng.profile_get(x)[0] for x in ("k_spatial", "k_transition")}
        eng.profile_enable(False)
        return k

    k_off, k_on = profiled(lambda: call(False)), profiled(lambda: call(True))
    torch.cuda.synchronize()
    plan.saliency_device(0, 0, U, T, window, stride, False, SIGMA_DEG, 180, 90, "density", 0, 0, 0, pooled.data_ptr(), st.data_ptr(),
                         stream=stream.cuda_stream, d_ids=ids.data_ptr())
    torch.cuda.synchronize()
    pairs = float((counts[1].sum(dim=0).double() * pooled[1].double()).sum().item())
    n_s, c_s, t_s, s_s = stats(ms_n), stats(ms_c), stats(ms_t), stats(ms_s)
    a, b = out[:2].cpu().numpy(), t_out.cpu().numpy()
    worst = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, key in enumerate(("lift", "info_gain")):
            fin = np.isfinite(a[k]) & np.isfinite(b[k])
            worst[key] = float((np.abs(a[k][fin] - b[k][fin]) / (1.0 + np.abs(b[k][fin]))).max(initial=0.0))
    run.update({"device_call_nss": n_s, "device_call_no_nss": c_s, "today_lift_info_gain": t_s,
                "today_nss_one_viewer_saliency_similarity": s_s,
                "today_nss_all_viewers_scaled_ms": round(s_s["median_ms"] * U, 1),
                "profile_scopes_ms": {"nss": k_on, "no_nss": k_off},
                "k_congruency_points": {"pair_evaluations": pairs, "ms_no_nss": round(k_off["k_spatial"], 4),
                                        "ms_nss": round(k_on["k_spatial"], 4),
                                        "pairs_per_second_no_nss": round(pairs / (k_off["k_spatial"] * 1e-3), 1),
                                        "pairs_per_second_nss": round(pairs / (k_on["k_spatial"] * 1e-3), 1)},
                "nss_costs_ms": round(n_s["median_ms"] - c_s["median_ms"], 4),
                "speedup_no_nss_over_today_median": round(t_s["median_ms"] / c_s["median_ms"], 3),
                "slower_than_today_by_more_than_its_spread": bool(c_s["median_ms"] - t_s["median_ms"] > t_s["max_ms"] - t_s["min_ms"]),
                "scored_viewer_rows": int(rows[0].sum().item()), "own_list_entries": int(counts[1].sum().item()),
                "not_finite_in_the_same_places": bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))),
                "largest_disagreement_with_today": worst})
    del out, counts, rows, t_out, pooled, sim_stats
    torch.cuda.empty_cache()
    return run


def main(out_path, first, n_shapes):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(50)], 120.0, 2.0, True, VW, VH)
    raw = torch.from_numpy(plan.read_dirs()).to(dev)
    unit = raw / raw.pow(2).sum(dim=1, keepdim=True).sqrt()
    record = {"tool": "tools/congruency_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (workspace grown), the new call with and "
                        "without nss and today's route alternating; median and min..max; one call each for the whole video", "runs": []}
    if first and os.path.exists(out_path):                       # a run split over several invocations: keep the earlier shapes
        record["runs"] = json.load(open(out_path))["runs"][:first]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    ids_of = {}
    for name, U, T, window, stride in SHAPES[first:first + n_shapes]:
        if (U, T) not in ids_of:
            ids_of.clear()
            mu, mv = bench.synth_video(U, T, 1234, 0)
            px, py = np.minimum((mu * VW).astype(np.int64), VW), np.minimum((mv * VH).astype(np.int64), VH)
            ids_of[(U, T)] = torch.from_numpy((py * (VW + 1) + px).astype(np.int32)).to(dev)
        run = run_shape(eng, plan, unit, dev, stream, name, U, T, window, stride, ids_of[(U, T)])
        record["runs"].append(run)
        print(json.dumps(run), flush=True)
        record["device"] = torch.cuda.get_device_name(0)
        record["date"] = time.strftime("%Y-%m-%d")
        with open(out_path, "w") as f_out:                       # after every shape: a record of what has run
            json.dump(record, f_out, indent=1)
    plan.close()
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "saliency", "congruency_timing.json"),
         int(sys.argv[2]) if len(sys.argv) > 2 else 0, int(sys.argv[3]) if len(sys.argv) > 3 else len(SHAPES))
