"""Time of the fixation and tile-dwell events (vet_fixations), both modes (by = "angle" at 2 degrees, by = "tile"), min_frames = 5:
  config 3's shape (1024 viewers x 30 000 frames), pooled: window = stride = 20; window 20 at stride 1; the whole video;
      per viewer: the whole video; window = stride = 20; and the same per-viewer window = stride = 20 with the event list (two calls:
      the first gives offsets[U], read back, the second fills the events and centroids);
  config 5's shape (512 x 10 000), pooled, window 1.
Per shape the device call alone (direction ids resident, hipEvents on the launch stream, counts and an 8-bin histogram), its split
from the engine's profile scopes (k_user_dirs = k_spatial; k_fix_runs, k_fix_offsets, k_fix_labels, k_fix_centroids = k_transition;
k_fix_frames, k_fix_rows = k_finalize), and today's device route to the same counts alternating with the new call in the same run —
torch on the device, so it is the same code before and after this call existed:
  today   ids -> the two unit vectors gathered from the direction table -> dot -> compare with the cosine (or the two nearest tiles
          gathered and compared) -> run starts -> run ids by cumsum over the viewer-major samples -> run lengths by bincount -> per
          sample the length of its run -> per (viewer, frame) samples / fix_frames / events / sum_len, rows as differences of a cumsum
          along the frames, max_len by an unfold and amax.  No same-Vector rule, no histogram, no labels, no event list: the route is
          charged less work.
The walks and the row kernels are also timed next to device-to-device copies that move the bytes they read and write (walks: 20 B per
sample; pooled frame totals and rows: 8 B per sample), in the same run.
After a warm-up; per side the median and the min..max spread of REPS single calls.  Nothing gates on a speed ratio: the JSON holds the
numbers, also where the new call does not win.  Also recorded: whether the two routes' counts are equal.
usage: python tools/fixations_timing.py [out.json]      (default: profiles/fixation/fixations_timing.json)"""
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
WARMUP, REPS = 1, 5
STEP_DEG, MIN_FRAMES = 2.0, 5
EDGES = (1, 2, 5, 10, 20, 50, 100, 1000, 1 << 30)
# (workload, users, frames, window (None = whole video), stride, per_user, event list)
SHAPES = [("config3", 1024, 30000, 20, 20, False, False), ("config3", 1024, 30000, 20, 1, False, False),
          ("config3", 1024, 30000, None, 1, False, False), ("config3", 1024, 30000, None, 1, True, False),
          ("config3", 1024, 30000, 20, 20, True, False), ("config3", 1024, 30000, 20, 20, True, True),
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


def _copy(stream, dst, src):
    with torch.cuda.stream(stream):
        dst.copy_(src)


def run_shape(eng, plan, unit, near, dev, stream, name, U, T, window, stride, per_user, listed, by, ids):
    window = T if window is None else window
    R = (T - window) // stride + 1
    lead = (U, R) if per_user else (R,)
    cos = min(1.0, max(-1.0, math.cos(math.radians(STEP_DEG))))
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    counts = torch.empty((5,) + lead, dtype=torch.int64, device=dev)
    hist = torch.empty(lead + (len(EDGES) - 1,), dtype=torch.int32, device=dev)
    offsets = torch.empty(U + 1, dtype=torch.int64, device=dev)
    t_counts = torch.empty((5,) + lead, dtype=torch.int64, device=dev)
    held = {}

    def call():
        common = dict(d_counts=counts.data_ptr(), d_hist=hist.data_ptr(), d_status=st.data_ptr(), stream=stream.cuda_stream,
                      d_ids=ids.data_ptr())
        if not listed:
            plan.fixations_device(0, 0, U, T, window, stride, by, cos, MIN_FRAMES, per_user, EDGES, **common)
            return
        plan.fixations_device(0, 0, U, T, window, stride, by, cos, MIN_FRAMES, per_user, EDGES, d_offsets=offsets.data_ptr(), **common)
        stream.synchronize()
        n = int(offsets[U].item())
        if held.get("n", -1) < n:
            held.update(n=n, events=torch.empty((max(n, 1), 4), dtype=torch.int32, device=dev),
                        centroids=torch.empty((max(n, 1), 3), dtype=torch.float64, device=dev))
        plan.fixations_device(0, 0, U, T, window, stride, by, cos, MIN_FRAMES, per_user, None, max_events=n,
                              d_events=held["events"].data_ptr(), d_centroids=held["centroids"].data_ptr(), stream=stream.cuda_stream,
                              d_ids=ids.data_ptr())

    def today():
        with torch.cuda.stream(stream):
            a, b = ids[:-1].long(), ids[1:].long()
            ok = (a >= 0) & (b >= 0)
            if by == "tile":
                hold = ok & (near[a.clamp(min=0)] == near[b.clamp(min=0)])
            else:
                hold = ok & ((a == b) | ((unit[a.clamp(min=0)] * unit[b.clamp(min=0)]).sum(dim=2) >= cos))
            present = ids >= 0
            start = present.clone()
            start[1:] &= ~hold
            pr, s0 = present.t().reshape(-1), start.t().reshape(-1)          # viewer-major
            run_id = (torch.cumsum(s0, 0) - 1).clamp(min=0)
            length = torch.bincount(run_id[pr], minlength=int(run_id[-1].item()) + 1)
            mine = torch.where(pr, length[run_id], torch.zeros_like(run_id))   # per sample the length of its run
            event = s0 & (mine >= MIN_FRAMES)
            per = torch.stack([pr.long(), (pr & (mine >= MIN_FRAMES)).long(), event.long(), torch.where(event, mine, torch.zeros_like(mine))])
            per = per.view(4, U, T)
            top = per[3].unfold(1, window, stride).amax(dim=-1)               # [U][R]
            if not per_user:
                per, top = per.sum(dim=1, keepdim=True), top.amax(dim=0, keepdim=True)
            cs = torch.cat([torch.zeros_like(per[:, :, :1]), torch.cumsum(per, dim=2)], dim=2)
            first = torch.arange(R, device=dev) * stride
            rows = cs[:, :, first + window] - cs[:, :, first]                 # [4][U or 1][R]
            t_counts[:4] = rows.reshape((4,) + lead)
            t_counts[4] = top.reshape(lead)

    run = {"workload": name, "users": U, "frames": T, "window": window, "stride": stride, "per_user": per_user, "by": by,
           "event_list": listed, "rows": int(np.prod(lead))}
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
    k = {x: round(eng.profile_get(x)[0], 4) for x in ("k_spatial", "k_transition", "k_finalize")}
    eng.profile_enable(False)
    S = U * T
    copies = {}
    for key, nbytes in (("walks_20B_per_sample", S * 10), ("rows_8B_per_sample", S * 4)):
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _copy(stream, dst, src)
        copies[key] = stats([timed(stream, lambda: _copy(stream, dst, src)) for _ in range(REPS)])
        del src, dst
    c_s, t_s = stats(ms_c), stats(ms_t)
    run.update({"device_call": c_s, "today_torch_route": t_s,
                "kernels_ms": {"k_user_dirs": k["k_spatial"], "walks_offsets_centroids": k["k_transition"], "frames_and_rows": k["k_finalize"]},
                "d2d_copy_same_bytes": copies, "events": int(counts[2].sum().item()),
                "speedup_median": round(t_s["median_ms"] / c_s["median_ms"], 3),
                "slower_than_today_by_more_than_its_spread": bool(c_s["median_ms"] - t_s["median_ms"] > t_s["max_ms"] - t_s["min_ms"]),
                "counts_equal_today": bool(torch.equal(counts, t_counts))})
    torch.cuda.empty_cache()
    return run


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(50)], 120.0, 2.0, True, VW, VH)
    raw = torch.from_numpy(plan.read_dirs()).to(dev)
    unit = raw / raw.pow(2).sum(dim=1, keepdim=True).sqrt()
    near = torch.from_numpy(plan.read_nearest(0)).to(dev)
    record = {"tool": "tools/fixations_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "max_step_deg": STEP_DEG, "min_frames": MIN_FRAMES, "bins": len(EDGES) - 1,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (workspace grown), the new call and today's "
                        "route alternating; median and min..max", "runs": []}
    ids_of = {}
    for name, U, T, window, stride, per_user, listed in SHAPES:
        if (U, T) not in ids_of:
            mu, mv = bench.synth_video(U, T, 1234, 0)
            px, py = np.minimum((mu * VW).astype(np.int64), VW), np.minimum((mv * VH).astype(np.int64), VH)
            ids_of[(U, T)] = torch.from_numpy((py * (VW + 1) + px).astype(np.int32)).to(dev)
        for by in ("angle", "tile"):
            run = run_shape(eng, plan, unit, near, dev, stream, name, U, T, window, stride, per_user, listed, by, ids_of[(U, T)])
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
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fixation", "fixations_timing.json"))
