"""Time of the audience dispersion (vet_dispersion):
  config 3's shape (1024 viewers x 30 000 frames), pooled with 8 bins: window 1 (30 000 rows); window = stride = 20; the whole video;
      per viewer: window = stride = 20;
  512 x 10 000 pooled at window 1; 9000 viewers x 512 frames pooled at window 1.
Per shape the device call alone (direction ids resident, hipEvents on the launch stream; stats, centroid, counts and for the pooled
layout the 8-bin histogram), its per-kernel split from the engine's profile scopes (k_dispersion_pairs = k_spatial, the row stage =
k_transition) with the pair kernel's angles per second (it evaluates every ORDERED pair: present * (present - 1) angles a frame), and
today's route to the same numbers alternating with the new call in the same run — torch on the device, so it is the same code before
and after this call existed:
  today   in chunks of frames whose [frames][U][U] FP64 matrix stays under 1 GB: the unit vectors gathered from the direction table,
          bmm, clamp, acos, NaN where either viewer is absent and on the diagonal; per (frame, viewer) nansum, count, min and max
          over the partners; per frame the histogram by torch.bucketize + bincount (halved: the matrix holds every pair twice); then
          the rows from the per-frame (per-viewer) arrays by unfold + sum.  No centroid and no same-count: the route is charged less.
After a warm-up; per side the median and the min..max spread of REPS single calls.  Nothing gates on a speed ratio: the JSON holds the
numbers, also where the new call does not win.  Also recorded: whether the pair and slot counts agree, how many pairs the two
histograms place in different bins (an angle within a rounding of an edge: on the pixel grid many pairs are orthogonal, 90 degrees
is an edge, and today's dot is not the fused one) and the largest relative
disagreement between the routes' mean / max / nearest (today's dot is a bmm, not the fused dot, and its sums are torch's), from one
untimed run of today's route with the new call's same-Vector rule applied (+0.0; the timed route leaves arccos of a rounded dot there).
usage: python tools/dispersion_timing.py [out.json]      (default: profiles/dispersion/dispersion_timing.json)"""
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
WARMUP, REPS = 1, 3
CHUNK_BYTES = 1 << 30
EDGES = np.radians([0.0, 1.0, 5.0, 15.0, 30.0, 60.0, 90.0, 120.0, 180.0])
# (workload, users, frames, window (None = whole video), stride, per_user)
SHAPES = [("config3", 1024, 30000, 1, 1, False), ("config3", 1024, 30000, 20, 20, False), ("config3", 1024, 30000, None, 1, False),
          ("config3", 1024, 30000, 20, 20, True), ("config5_shape", 512, 10000, 1, 1, False), ("wide_audience", 9000, 512, 1, 1, False)]


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def run_shape(eng, plan, unit, raw, dev, stream, name, U, T, window, stride, per_user, ids):
    window = T if window is None else window
    R = (T - window) // stride + 1
    rows = U * R if per_user else R
    B = 0 if per_user else len(EDGES) - 1
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.empty((3, rows), dtype=torch.float64, device=dev)
    cen = torch.empty((rows, 3), dtype=torch.float64, device=dev)
    hist = torch.empty((rows, max(B, 1)), dtype=torch.int64, device=dev)
    counts = torch.empty((4, rows), dtype=torch.int64, device=dev)
    frames_per_chunk = max(1, min(T, CHUNK_BYTES // (U * U * 8)))
    e_t = torch.from_numpy(EDGES).to(dev)
    eye = torch.eye(U, dtype=torch.bool, device=dev)[None]
    # today's per-(frame, viewer) arrays and results
    p_sum = torch.empty((T, U), dtype=torch.float64, device=dev)
    p_min = torch.empty((T, U), dtype=torch.float64, device=dev)
    p_max = torch.empty((T, U), dtype=torch.float64, device=dev)
    p_cnt = torch.empty((T, U), dtype=torch.int64, device=dev)
    f_hist = torch.empty((T, max(B, 1)), dtype=torch.int64, device=dev)
    today_out = {}

    def call():
        plan.dispersion_device(0, 0, U, T, window, stride, per_user, None if per_user else EDGES, out.data_ptr(), cen.data_ptr(),
                               hist.data_ptr() if B else 0, counts.data_ptr(), st.data_ptr(), stream=stream.cuda_stream,
                               d_ids=ids.data_ptr())

    def today(same_rule=False):
        inf = float("inf")
        with torch.cuda.stream(stream):
            for f0 in range(0, T, frames_per_chunk):
                f1 = min(T, f0 + frames_per_chunk)
                idc = ids[f0:f1].long()
                ok = idc >= 0
                v = unit[idc.clamp(min=0)]                                                   # [fc][U][3]
                c = torch.bmm(v, v.transpose(1, 2)).clamp_(-1.0, 1.0)
                ang = torch.acos(c)
                if same_rule:                                    # the comparison only: the same Vector is +0.0, as the new call defines
                    r = raw[idc.clamp(min=0)]
                    eq = (r[:, :, None, 0] == r[:, None, :, 0]) & (r[:, :, None, 1] == r[:, None, :, 1]) & \
                        (r[:, :, None, 2] == r[:, None, :, 2])
                    ang = torch.where(eq, torch.zeros_like(ang), ang)
                pair = ok[:, :, None] & ok[:, None, :] & ~eye
                ang = torch.where(pair, ang, torch.full_like(ang, float("nan")))
                p_cnt[f0:f1] = pair.sum(dim=2)
                p_sum[f0:f1] = torch.nansum(ang, dim=2)
                p_min[f0:f1] = torch.where(pair, ang, torch.full_like(ang, inf)).amin(dim=2)
                p_max[f0:f1] = torch.where(pair, ang, torch.full_like(ang, -inf)).amax(dim=2)
                if B:
                    b = (torch.bucketize(ang, e_t, right=True) - 1).clamp_(0, B)              # NaN and a >= e_B land in bin B: dropped
                    b += torch.arange(f1 - f0, device=dev)[:, None, None] * (B + 1)
                    f_hist[f0:f1] = torch.bincount(b.reshape(-1), minlength=(f1 - f0) * (B + 1)).reshape(f1 - f0, B + 1)[:, :B] // 2
            has = p_cnt > 0
            zero = torch.zeros_like(p_sum)
            near = torch.where(has, p_min, zero)
            far = torch.where(has, p_max, torch.full_like(p_max, -inf))
            win = lambda x: x.unfold(0, window, stride)          # [R][U][window]
            if per_user:
                n = win(p_cnt).sum(dim=2).t().reshape(-1)
                slots = win(has.long()).sum(dim=2).t().reshape(-1)
                today_out["mean"] = win(p_sum).sum(dim=2).t().reshape(-1) / n
                today_out["max"] = win(far).amax(dim=2).t().reshape(-1)
                today_out["nearest"] = win(near).sum(dim=2).t().reshape(-1) / slots
                today_out["samples"] = n
            else:
                n = win(p_cnt.sum(dim=1)).sum(dim=1)
                slots = win(has.sum(dim=1)).sum(dim=1)
                today_out["mean"] = win(p_sum.sum(dim=1)).sum(dim=1) / n
                today_out["max"] = win(far.amax(dim=1)).amax(dim=1)
                today_out["nearest"] = win(near.sum(dim=1)).sum(dim=1) / slots
                today_out["samples"] = n // 2
                today_out["hist"] = f_hist.unfold(0, window, stride).sum(dim=2)
            today_out["slots"] = slots

    run = {"workload": name, "users": U, "frames": T, "window": window, "stride": stride, "per_user": per_user, "rows": rows, "bins": B,
           "today_frames_per_chunk": frames_per_chunk, "today_chunks": -(-T // frames_per_chunk)}
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
    today(same_rule=True)                                        # untimed: today's values under the new call's same-Vector rule
    torch.cuda.synchronize()
    present = (ids >= 0).sum(dim=1).double()
    ordered = float((present * (present - 1)).sum().item())
    a = {key: out[i].cpu().numpy() for i, key in enumerate(("mean", "max", "nearest"))}
    b = {key: torch.where(today_out["samples"] > 0, today_out[key], torch.full_like(today_out[key], float("nan"))).cpu().numpy()
         for key in ("mean", "max", "nearest")}
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = lambda x, y: float(np.nanmax(np.abs(x - y) / np.where(y == 0, 1.0, np.abs(y)), initial=0.0))
        run.update({"device_call": c_s, "today_torch_route": t_s,
                    "kernels_ms": {"k_dispersion_pairs": k["k_spatial"], "row_stage": k["k_transition"]},
                    "angles_evaluated": ordered, "pair_samples": ordered / 2,
                    "pair_kernel_angles_per_s": round(ordered / (k["k_spatial"] * 1e-3), 1) if k["k_spatial"] > 0 else None,
                    "speedup_median": round(t_s["median_ms"] / c_s["median_ms"], 3),
                    "slower_than_today_by_more_than_its_spread": bool(c_s["median_ms"] - t_s["median_ms"] > t_s["max_ms"] - t_s["min_ms"]),
                    "samples_equal_today": bool(torch.equal(counts[0], today_out["samples"])),
                    "slots_equal_today": bool(torch.equal(counts[2], today_out["slots"])),
                    "hist_counts_moved_vs_today": int((hist[:, :B] - today_out["hist"]).abs().sum().item()) // 2 if B else None,
                    "nan_positions_agree_with_today": bool(all(np.array_equal(np.isnan(a[x]), np.isnan(b[x])) for x in a)),
                    "max_rel_diff_vs_today": {x: rel(a[x], b[x]) for x in a}})
    del out, cen, hist, counts, p_sum, p_min, p_max, p_cnt, f_hist
    today_out.clear()
    torch.cuda.empty_cache()
    return run


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(50)], 120.0, 2.0, True, VW, VH)
    raw = torch.from_numpy(plan.read_dirs()).to(dev)
    unit = raw / raw.pow(2).sum(dim=1, keepdim=True).sqrt()
    record = {"tool": "tools/dispersion_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "edges_deg": np.degrees(EDGES).round(6).tolist(),
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (workspace grown), the new call and today's "
                        "route alternating; median and min..max", "runs": []}
    ids_of = {}
    for name, U, T, window, stride, per_user in SHAPES:
        if (U, T) not in ids_of:
            ids_of.clear()
            mu, mv = bench.synth_video(U, T, 1234, 0)
            px, py = np.minimum((mu * VW).astype(np.int64), VW), np.minimum((mv * VH).astype(np.int64), VH)
            ids_of[(U, T)] = torch.from_numpy((py * (VW + 1) + px).astype(np.int32)).to(dev)
        run = run_shape(eng, plan, unit, raw, dev, stream, name, U, T, window, stride, per_user, ids_of[(U, T)])
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
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dispersion", "dispersion_timing.json"))
