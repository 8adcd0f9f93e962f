"""Time of the viewer clusters (vet_viewer_clusters) at threshold_deg = 30, min_share = 1:
  config 3's shape (1024 viewers x 30 000 frames): window 1 (30 000 rows); window = stride = 20; the whole video;
  512 x 10 000 at window 1.  9000 viewers x 512 frames is REFUSED BY DESIGN (VET_ERR_UNSUPPORTED: at most 8192 viewers, the labels
  of a row live in LDS); the tool records the refusal instead of a time.
Per shape the device call alone (direction ids resident, hipEvents on the launch stream; labels, sizes, counts, top and stats), its
per-kernel split from the engine's profile scopes of one profiled call (k_cluster_ids = k_spatial, k_cluster_links = k_transition,
k_cluster_components = k_finalize), the link kernel's NEAR decisions per second (it decides every ORDERED pair of viewers in every
frame of every row: U * (U - 1) * window * rows, absent viewers included — the walk does not skip them), the label-propagation
sweeps the rows needed, the extra cost of the centroids (a second profiled call with d_centroids, the difference of its
k_finalize), and today's route to the same partition alternating with the new call in the same run — torch on the device, so it is
the same code before and after this call existed:
  today   in chunks of frames whose [frames][U][U] FP64 matrix stays under 1 GB: the unit vectors gathered from the direction table,
          bmm, compare with cos_threshold (or the same id), the booleans and the co-presence summed over the window's frames, LINKED
          from the two counts, then masked-min label propagation with one pointer jump per sweep to a fixpoint, and torch.unique for
          the relabelling; sizes and counts by scatter_add.  No same-Vector rule, no top, no entropy: the route is charged less.
After a warm-up; per side the median and the min..max spread of REPS single calls.  Nothing gates on a speed ratio: the JSON holds the
numbers, also where the new call does not win.  Also recorded: whether labels and counts of the two routes are equal (integers,
exact; today's dot is a bmm, not the fused dot, so a pair within a rounding of the threshold may differ: the tool counts the rows).
usage: python tools/viewer_clusters_timing.py [out.json] [quick]      (default: profiles/cluster/viewer_clusters_timing.json; quick:
the same code on 96 x 400 shapes, a trial of the tool, not a measurement)"""
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
WARMUP, REPS = 1, 3
CHUNK_BYTES = 1 << 30
THRESHOLD_DEG, MIN_SHARE = 30.0, 1.0
FRACTIONS = (0.5, 0.8, 0.95)
# (workload, users, frames, window (None = whole video), stride)
SHAPES = [("config3", 1024, 30000, 1, 1), ("config3", 1024, 30000, 20, 20), ("config3", 1024, 30000, None, 1),
          ("config5_shape", 512, 10000, 1, 1), ("wide_audience", 9000, 512, 1, 1)]


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
    window = T if window is None else window
    R = (T - window) // stride + 1
    cos_thr = math.cos(math.radians(THRESHOLD_DEG))
    run = {"workload": name, "users": U, "frames": T, "window": window, "stride": stride, "rows": R}
    if U > 8192:
        try:
            plan.viewer_clusters_device(0, 0, U, T, window, stride, cos_thr, MIN_SHARE, None, d_ids=ids.data_ptr())
            run["refused"] = False
        except _native.NativeError as e:
            run.update(refused=True, code=e.code, message=str(e), by_design="at most 8192 viewers: the labels of a row live in LDS")
        return run
    assert stride == window or window == 1 or R == 1, "today's route pools whole, non-overlapping rows"
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    labels = torch.empty((R, U), dtype=torch.int32, device=dev)
    sizes = torch.empty((R, U), dtype=torch.int32, device=dev)
    counts = torch.empty((5, R), dtype=torch.int64, device=dev)
    top = torch.empty((R, len(FRACTIONS)), dtype=torch.int32, device=dev)
    out = torch.empty((3, R), dtype=torch.float64, device=dev)
    frames_per_chunk = max(1, min(T, CHUNK_BYTES // (U * U * 8)))
    rows_per_chunk = max(1, frames_per_chunk // window)
    eye = torch.eye(U, dtype=torch.bool, device=dev)[None]
    arange = torch.arange(U, dtype=torch.int64, device=dev)
    BIG = U
    t_labels = torch.empty((R, U), dtype=torch.int64, device=dev)
    t_counts = torch.empty((5, R), dtype=torch.int64, device=dev)
    sweeps_today = []

    def call(centroids=None):
        plan.viewer_clusters_device(0, 0, U, T, window, stride, cos_thr, MIN_SHARE, FRACTIONS, labels.data_ptr(), sizes.data_ptr(),
                                    counts.data_ptr(), top.data_ptr(), out.data_ptr(), centroids.data_ptr() if centroids is not None else 0,
                                    0, st.data_ptr(), stream=stream.cuda_stream, d_ids=ids.data_ptr())

    def pair_counts(f0, f1):
        """(co, near) int32 [U][U] summed over frames [f0, f1), in chunks under the budget"""
        co = torch.zeros((U, U), dtype=torch.int32, device=dev)
        nr = torch.zeros((U, U), dtype=torch.int32, device=dev)
        for g0 in range(f0, f1, frames_per_chunk):
            idc = ids[g0:min(f1, g0 + frames_per_chunk)].long()
            ok = idc >= 0
            v = unit[idc.clamp(min=0)]
            c = torch.bmm(v, v.transpose(1, 2))
            both = ok[:, :, None] & ok[:, None, :] & ~eye
            co += both.sum(dim=0, dtype=torch.int32)
            nr += (both & ((c >= cos_thr) | (idc[:, :, None] == idc[:, None, :]))).sum(dim=0, dtype=torch.int32)
        return co, nr

    def today():
        sweeps_today.clear()
        with torch.cuda.stream(stream):
            for r0 in range(0, R, rows_per_chunk):
                r1 = min(R, r0 + rows_per_chunk)
                rc = r1 - r0
                if window > frames_per_chunk:                    # one long row at a time
                    co, nr = pair_counts(r0 * stride, r0 * stride + window)
                    co, nr = co[None], nr[None]
                    present = (ids[r0 * stride:r0 * stride + window] >= 0).any(dim=0)[None]
                else:
                    idc = ids[r0 * stride:r0 * stride + rc * window].long()
                    ok = idc >= 0
                    v = unit[idc.clamp(min=0)]
                    c = torch.bmm(v, v.transpose(1, 2))
                    both = ok[:, :, None] & ok[:, None, :] & ~eye
                    near = both & ((c >= cos_thr) | (idc[:, :, None] == idc[:, None, :]))
                    co = both.view(rc, window, U, U).sum(dim=1, dtype=torch.int32)
                    nr = near.view(rc, window, U, U).sum(dim=1, dtype=torch.int32)
                    present = ok.view(rc, window, U).any(dim=1)
                linked = (co >= 1) & (nr.double() >= MIN_SHARE * co.double())
                lab = torch.where(present, arange[None].expand(rc, U), torch.full((rc, U), BIG, dtype=torch.int64, device=dev))
                n = 0
                while True:
                    cand = torch.where(linked, lab[:, None, :].expand(rc, U, U), torch.full((), BIG, dtype=torch.int64, device=dev))
                    new = torch.minimum(lab, cand.amin(dim=2))
                    pad = torch.cat([new, torch.full((rc, 1), BIG, dtype=torch.int64, device=dev)], dim=1)
                    new = torch.minimum(new, pad.gather(1, new))     # one pointer jump (an absent viewer points at the pad)
                    n += 1
                    if torch.equal(new, lab):
                        break
                    lab = new
                sweeps_today.append(n)
                keys = lab + torch.arange(rc, device=dev)[:, None] * (U + 1)
                uniq, inv = torch.unique(keys, return_inverse=True)          # sorted: row-major, then by root
                is_root = (uniq % (U + 1)) < BIG
                row_of = uniq // (U + 1)
                first = torch.searchsorted(row_of, torch.arange(rc, device=dev))
                dense = torch.where(lab < BIG, inv - first[:, None], torch.full_like(inv, -1))
                t_labels[r0:r1] = dense
                sz = torch.zeros((rc, U + 1), dtype=torch.int64, device=dev)
                sz.scatter_add_(1, torch.where(dense >= 0, dense, torch.full_like(dense, U)), torch.ones_like(dense))
                sz = sz[:, :U]
                t_counts[0, r0:r1] = present.sum(dim=1)
                t_counts[1, r0:r1] = torch.zeros(rc, dtype=torch.int64, device=dev).scatter_add_(0, row_of, is_root.long())
                t_counts[2, r0:r1] = sz.amax(dim=1)
                t_counts[3, r0:r1] = (sz == 1).sum(dim=1)
                t_counts[4, r0:r1] = linked.sum(dim=(1, 2)) // 2

    run.update(today_frames_per_chunk=frames_per_chunk, today_rows_per_chunk=rows_per_chunk)
    for _ in range(WARMUP):
        call(); today()
    torch.cuda.synchronize()
    ms_c, ms_t = [], []
    for _ in range(REPS):
        ms_c.append(timed(stream, call))
        ms_t.append(timed(stream, today))
    names = {"k_spatial": "k_cluster_ids", "k_transition": "k_cluster_links", "k_finalize": "k_cluster_components"}

    def profiled(centroids=None):
        eng.profile_enable(True); eng.profile_reset()
        call(centroids)
        eng.synchronize(); torch.cuda.synchronize()
        k = {names[x]: round(eng.profile_get(x)[0], 4) for x in names}
        eng.profile_enable(False)
        return k
    k = profiled()
    most, total = plan.viewer_clusters_sweeps()
    cen = torch.empty((R, U, 3), dtype=torch.float64, device=dev)
    k_cen = profiled(cen)
    del cen
    c_s, t_s = stats(ms_c), stats(ms_t)
    decisions = float(U) * (U - 1) * window * R
    same_rows = (labels.long() == t_labels).all(dim=1)
    run.update({"device_call": c_s, "today_torch_route": t_s, "kernels_ms": k, "near_decisions": decisions,
                "link_kernel_near_decisions_per_s": round(decisions / (k["k_cluster_links"] * 1e-3), 1) if k["k_cluster_links"] > 0 else None,
                "dispersion_pair_kernel_angles_per_s": 2.9e11,
                "sweeps": {"most_of_a_row": most, "mean_per_row": round(total / R, 3), "today_most_of_a_chunk": max(sweeps_today)},
                "centroids_extra_ms": round(k_cen["k_cluster_components"] - k["k_cluster_components"], 4),
                "speedup_median": round(t_s["median_ms"] / c_s["median_ms"], 3),
                "slower_than_today_by_more_than_its_spread": bool(c_s["median_ms"] - t_s["median_ms"] > t_s["max_ms"] - t_s["min_ms"]),
                "rows_with_equal_labels": int(same_rows.sum().item()), "counts_equal_today": bool(torch.equal(counts, t_counts)),
                "clusters_mean": round(float(counts[1].double().mean().item()), 3), "links_mean": round(float(counts[4].double().mean().item()), 1)})
    del labels, sizes, counts, top, out, t_labels, t_counts
    torch.cuda.empty_cache()
    return run


QUICK = [("quick", 96, 400, 1, 1), ("quick", 96, 400, 20, 20), ("quick", 96, 400, None, 1), ("wide_audience", 9000, 8, 1, 1)]


def main(out_path, shapes=SHAPES):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(50)], 120.0, 2.0, True, VW, VH)
    raw = torch.from_numpy(plan.read_dirs()).to(dev)
    unit = raw / raw.pow(2).sum(dim=1, keepdim=True).sqrt()
    record = {"tool": "tools/viewer_clusters_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "threshold_deg": THRESHOLD_DEG, "min_share": MIN_SHARE, "fractions": list(FRACTIONS),
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (workspace grown), the new call and today's "
                        "route alternating; median and min..max; per-kernel times from one profiled call", "runs": []}
    ids_of = {}
    for name, U, T, window, stride in shapes:
        if (U, T) not in ids_of:
            ids_of.clear()
            mu, mv = bench.synth_video(U, T, 1234, 0)
            px, py = np.minimum((mu * VW).astype(np.int64), VW), np.minimum((mv * VH).astype(np.int64), VH)
            ids_of[(U, T)] = torch.from_numpy((py * (VW + 1) + px).astype(np.int32)).to(dev)
        run = run_shape(eng, plan, unit, dev, stream, name, U, T, window, stride, ids_of[(U, T)])
        record["runs"].append(run)
        print(json.dumps(run), flush=True)
    plan.close()
    record["device"] = torch.cuda.get_device_name(0)
    record["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f_out:
        json.dump(record, f_out, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cluster", "viewer_clusters_timing.json"),
         QUICK if "quick" in sys.argv[2:] else SHAPES)
