"""Time of the head-motion statistics (vet_head_motion):
  config 3's shape (1024 viewers x 30 000 frames), pooled: window = stride = 20; window 20 at stride 1; the whole video;
      per viewer: the whole video; window = stride = 20;
  config 5's shape (512 x 10 000), pooled, window = stride = 20 and the whole video, at lag 1 and lag 10.
Per shape the device call alone (direction ids resident, hipEvents on the launch stream, mean / sd / max / total, three quantiles and a
16-bin histogram), its per-kernel split from the engine's profile scopes (stage 1 = k_spatial, the row kernels = k_transition), and
today's route to the same numbers alternating with the new call in the same run — torch on the device, so it is the same code before
and after this call existed:
  today   ids -> the two unit vectors gathered from the direction table -> dot -> clamp -> acos (angles [P][U], NaN absent), then per
          row, in chunks of rows under 1 GB: the [rows][window * U] slice materialised from an unfold view, sorted along the row (NaN
          last), N = the non-NaN count, nansum / N, the quantiles by lerp between gathered order statistics (torch.nanquantile refuses
          rows of more than 16 M values, and its result is this).  No sd, no histogram, no still count: the route is charged less work.
Stage 1 is also timed next to a device-to-device copy of the bytes it writes (P * U * 8), in the same run.
After a warm-up; per side the median and the min..max spread of REPS single calls.  Nothing gates on a speed ratio: the JSON holds the
numbers, also where the new call does not win.  Also recorded: the largest relative disagreement between the routes' means and
quantiles (today's dot is not fused and its sums are torch's), from one untimed run of today's route with the new call's still rule
applied (the same Vector is +0.0; the timed route leaves arccos of a rounded dot, up to 2.6e-8 rad, there).
usage: python tools/head_motion_timing.py [out.json]      (default: profiles/motion/head_motion_timing.json)"""
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
WARMUP, REPS = 1, 5
CHUNK_BYTES = 1 << 30
FRACTIONS = (0.5, 0.9, 0.99)
EDGES = np.radians(np.concatenate([[0.0], np.logspace(-1, np.log10(180.0), 16)]))
# (workload, users, frames, window (None = whole video), stride, lag, per_user)
SHAPES = [("config3", 1024, 30000, 20, 20, 1, False), ("config3", 1024, 30000, 20, 1, 1, False), ("config3", 1024, 30000, None, 1, 1, False),
          ("config3", 1024, 30000, None, 1, 1, True), ("config3", 1024, 30000, 20, 20, 1, True),
          ("config5_shape", 512, 10000, 20, 20, 1, False), ("config5_shape", 512, 10000, 20, 20, 10, False),
          ("config5_shape", 512, 10000, None, 1, 1, False), ("config5_shape", 512, 10000, None, 1, 10, False)]


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def run_shape(eng, plan, unit, raw, dev, stream, name, U, T, window, stride, lag, per_user, ids):
    P = T - lag
    window = P if window is None else window
    R = (P - window) // stride + 1
    rows, W = (U * R, window) if per_user else (R, window * U)
    Q, B = len(FRACTIONS), len(EDGES) - 1
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.empty((4, rows), dtype=torch.float64, device=dev)
    quant = torch.empty((rows, Q), dtype=torch.float64, device=dev)
    hist = torch.empty((rows, B), dtype=torch.int32, device=dev)
    still = torch.empty(rows, dtype=torch.int32, device=dev)
    samples = torch.empty(rows, dtype=torch.int32, device=dev)
    t_mean = torch.empty(rows, dtype=torch.float64, device=dev)
    t_quant = torch.empty((rows, Q), dtype=torch.float64, device=dev)
    t_samples = torch.empty(rows, dtype=torch.int64, device=dev)
    rows_per_chunk = max(1, min(rows, CHUNK_BYTES // (W * 8)))
    q_t = torch.tensor(FRACTIONS, dtype=torch.float64, device=dev)

    def call():
        plan.head_motion_device(0, 0, U, T, window, stride, lag, per_user, FRACTIONS, EDGES, out.data_ptr(), quant.data_ptr(),
                                hist.data_ptr(), still.data_ptr(), samples.data_ptr(), st.data_ptr(), stream=stream.cuda_stream,
                                d_ids=ids.data_ptr())

    def today(still_rule=False):
        with torch.cuda.stream(stream):
            a, b = ids[:P].long(), ids[lag:].long()
            ok = (a >= 0) & (b >= 0)
            c = (unit[a.clamp(min=0)] * unit[b.clamp(min=0)]).sum(dim=2).clamp(-1.0, 1.0)
            ang = torch.where(ok, torch.acos(c), torch.full_like(c, float("nan")))          # [P][U]
            if still_rule:                                       # the comparison only: the same Vector is +0.0, as the new call defines
                ang = torch.where(ok & (raw[a.clamp(min=0)] == raw[b.clamp(min=0)]).all(dim=2), torch.zeros_like(ang), ang)
            if per_user:
                view = ang.t().contiguous().unfold(1, window, stride).reshape(rows, 1, window)      # [U * R][1][window]
            else:
                view = ang.unfold(0, window, stride)                                        # [R][U][window]
            for r0 in range(0, rows, rows_per_chunk):
                r1 = min(rows, r0 + rows_per_chunk)
                x, _ = torch.sort(view[r0:r1].reshape(r1 - r0, -1), dim=1)                  # materialised, NaN last
                N = (~torch.isnan(x)).sum(dim=1)
                t_samples[r0:r1] = N
                t_mean[r0:r1] = torch.nansum(x, dim=1) / N
                pos = q_t[None, :] * (N[:, None] - 1).clamp(min=0).double()
                i = pos.floor().long()
                j = torch.minimum(i + 1, (N[:, None] - 1).clamp(min=0))
                xi, xj = torch.gather(x, 1, i), torch.gather(x, 1, j)
                t_quant[r0:r1] = xi + (xj - xi) * (pos - i.double())

    run = {"workload": name, "users": U, "frames": T, "window": window, "stride": stride, "lag": lag, "per_user": per_user, "rows": rows,
           "values_per_row": W, "shape": "one wave per row" if W <= 64 else "one workgroup per row" if W <= 16384 else "chunked, radix selection",
           "today_rows_per_chunk": rows_per_chunk, "today_materialised_bytes_total": rows * W * 8}
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
    # stage 1 next to a device-to-device copy of the bytes it writes
    src, dst = torch.empty(P * U, dtype=torch.float64, device=dev), torch.empty(P * U, dtype=torch.float64, device=dev)
    with torch.cuda.stream(stream):
        dst.copy_(src)
    ms_copy = [timed(stream, lambda: _copy(stream, dst, src)) for _ in range(REPS)]
    c_s, t_s = stats(ms_c), stats(ms_t)
    today(still_rule=True)                                       # untimed: today's values under the new call's still rule
    torch.cuda.synchronize()
    a_mean, b_mean = out[0].cpu().numpy(), t_mean.cpu().numpy()
    a_q, b_q = quant.cpu().numpy(), t_quant.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = lambda a, b: float(np.nanmax(np.abs(a - b) / np.where(b == 0, 1.0, np.abs(b)), initial=0.0))
        run.update({"device_call": c_s, "today_torch_route": t_s,
                    "kernels_ms": {"stage1_k_motion_angles" + ("_with_k_user_dirs" if per_user else ""): k["k_spatial"],
                                   "row_kernels": k["k_transition"]},
                    "stage1_bytes_written": P * U * 8, "d2d_copy_same_bytes": stats(ms_copy),
                    "speedup_median": round(t_s["median_ms"] / c_s["median_ms"], 3),
                    "slower_than_today_by_more_than_its_spread": bool(c_s["median_ms"] - t_s["median_ms"] > t_s["max_ms"] - t_s["min_ms"]),
                    "samples_equal_today": bool(torch.equal(samples.long(), t_samples)),
                    "nan_positions_agree_with_today": bool(np.array_equal(np.isnan(a_mean), np.isnan(b_mean))
                                                           and np.array_equal(np.isnan(a_q), np.isnan(b_q))),
                    "max_rel_diff_mean_vs_today": rel(a_mean, b_mean), "max_rel_diff_quantiles_vs_today": rel(a_q, b_q)})
    del src, dst, out, quant, hist, t_quant
    torch.cuda.empty_cache()
    return run


def _copy(stream, dst, src):
    with torch.cuda.stream(stream):
        dst.copy_(src)


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(50)], 120.0, 2.0, True, VW, VH)
    raw = torch.from_numpy(plan.read_dirs()).to(dev)
    unit = raw / raw.pow(2).sum(dim=1, keepdim=True).sqrt()
    record = {"tool": "tools/head_motion_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "warmup": WARMUP, "reps": REPS,
              "fractions": list(FRACTIONS), "bins": len(EDGES) - 1,
              "timing": "hipEvents around single calls on the launch stream after WARMUP calls (workspace grown), the new call and today's "
                        "route alternating; median and min..max", "runs": []}
    ids_of = {}
    for name, U, T, window, stride, lag, per_user in SHAPES:
        if (U, T) not in ids_of:
            mu, mv = bench.synth_video(U, T, 1234, 0)
            px, py = np.minimum((mu * VW).astype(np.int64), VW), np.minimum((mv * VH).astype(np.int64), VH)
            ids_of[(U, T)] = torch.from_numpy((py * (VW + 1) + px).astype(np.int32)).to(dev)
        run = run_shape(eng, plan, unit, raw, dev, stream, name, U, T, window, stride, lag, per_user, ids_of[(U, T)])
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
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "motion", "head_motion_timing.json"))
