"""Time of the tiling renders (include/vet.h: vet_tiling_*) on one MI355X, for the Fibonacci tiling of 1001 tiles (its
listed edges, every shared edge twice, and its centres) and the 36 x 18 lat/lon tiling, 180 orbit frames at 1024 x 768:
  * vet_tiling_create wall clock (H2D of the arcs + k_tiling_chords + synchronise);
  * vet_tiling_render of the 180 frames into device memory (memset + k_tiling_splat + k_tiling_compose per block of frames),
    hipEvents on the launch stream, beside a device-to-device copy of the same bytes in the same run;
  * render_tiling frames/s through the host path (pinned staging -> numpy).
The split into splat and compose time comes from a run per scene of this script under `rocprofv3 --kernel-trace --stats`
(`--trace-only SCENE`: the device renders alone), folded in by `--fold <kernel_stats.csv> SCENE`.
usage: python tools/tiling_timing.py [out.json]                       (default: profiles/tiling/tiling_timing.json)
       python tools/tiling_timing.py --trace-only fb_1001|latlon_36x18
       python tools/tiling_timing.py --fold kernel_stats.csv fb_1001|latlon_36x18 [out.json]"""
import csv
import json
import os
import sys
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'viewport-entropy-toolkit_amd'))

W, H, FRAMES = 1024, 768, 180
ITERS = 5
DEFAULT_OUT = os.path.join(ROOT, "profiles", "tiling", "tiling_timing.json")


def scenes():
    from viewport_entropy_toolkit.utilities import get_lat_lon_tiles
    from viewport_entropy_toolkit.utilities.visualization_utils import _arcs_of, _fb_scene
    arcs, centres = _fb_scene(1001)
    return {"fb_1001": (arcs, centres), "latlon_36x18": (_arcs_of(get_lat_lon_tiles(36, 18)), None)}


def timed(stream, fn, iters=ITERS):
    import torch
    fn()                                                   # warm-up
    stream.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / iters


def trace_only(scene):
    import torch
    from viewport_entropy_toolkit import _native
    from viewport_entropy_toolkit.utilities import tiling_orbit_cameras
    cams = tiling_orbit_cameras()
    rgb = torch.empty((FRAMES, H, W, 3), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    arcs, centres = scenes()[scene]
    tl = _native.Tiling(_native.Engine.default(), arcs, centres, W, H)
    for _ in range(1 + ITERS):
        tl.render_device(cams, rgb.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    tl.close()


def main(out_path):
    import torch
    import bench
    from viewport_entropy_toolkit import _native
    from viewport_entropy_toolkit.utilities import render_tiling, tiling_orbit_cameras
    eng = _native.Engine.default()
    cams = tiling_orbit_cameras()
    rec = {"tool": "tools/tiling_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "frame": [W, H], "frames": FRAMES,
           "iters": ITERS}
    rgb = torch.empty((FRAMES, H, W, 3), dtype=torch.uint8, device="cuda")
    copy = torch.empty_like(rgb)
    nbytes = rgb.numel()
    stream = torch.cuda.Stream()
    for name, (arcs, centres) in scenes().items():
        _native.Tiling(eng, arcs, centres, W, H).close()                   # module load, first-use costs
        t0 = time.perf_counter()
        tl = _native.Tiling(eng, arcs, centres, W, H)
        create_ms = (time.perf_counter() - t0) * 1e3

        def render():
            tl.render_device(cams, rgb.data_ptr(), stream=stream.cuda_stream)

        def d2d():
            with torch.cuda.stream(stream):
                copy.copy_(rgb)

        ms_render, ms_copy = timed(stream, render), timed(stream, d2d)
        tl.close()
        render_tiling(arcs, centres, cams[:16])                           # staging, warm
        t0 = time.perf_counter()
        render_tiling(arcs, centres, cams)
        s_host = time.perf_counter() - t0
        rec[name] = {
            "arcs": int(len(arcs)), "chords": int(len(arcs)) * 49, "centres": 0 if centres is None else int(len(centres)),
            "bytes_written": nbytes, "create_ms": create_ms,
            "render_device_ms": ms_render, "render_device_us_per_frame": ms_render * 1e3 / FRAMES,
            "render_device_write_TBps": nbytes / (ms_render * 1e-3) / 1e12,
            "d2d_copy_ms": ms_copy, "d2d_copy_write_TBps": nbytes / (ms_copy * 1e-3) / 1e12,
            "render_tiling_host_s": s_host, "render_tiling_frames_per_s": FRAMES / s_host,
        }
    rec["timing"] = ("create: wall clock after one warm-up create; render_device: torch.cuda.Event around ITERS calls of the "
                     "180 orbit frames on one stream after one warm-up call (memset + splat + compose per block of frames); "
                     "render_tiling: host clock, whole function (create, render to host through pinned staging, close)")
    out = Path(out_path)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


def fold(stats_csv, scene, out_path):
    """Per-kernel time of a --trace-only run (rocprofv3 kernel_stats.csv) into the scene's record: 1 + ITERS renders of
    the 180 frames, one create."""
    rec = json.loads(Path(out_path).read_text())
    kernels = {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            for key in ("k_tiling_chords", "k_tiling_splat", "k_tiling_compose"):
                if key in row["Name"]:
                    k = kernels.setdefault(key, {"calls": 0, "total_ns": 0.0})
                    k["calls"] += int(row["Calls"])
                    k["total_ns"] += float(row["TotalDurationNs"])
    renders = 1 + ITERS
    ms = {k: v["total_ns"] / 1e6 for k, v in kernels.items()}
    compose = ms.get("k_tiling_compose", 0.0) / renders
    rec[scene]["kernel_trace"] = {
        "what": f"rocprofv3 --kernel-trace --stats of tools/tiling_timing.py --trace-only {scene}: one create, "
                f"{renders} renders of the 180 frames; ms per render",
        "kernels": kernels,
        "chords_ms": ms.get("k_tiling_chords", 0.0),
        "splat_ms": ms.get("k_tiling_splat", 0.0) / renders,
        "compose_ms": compose,
        "compose_write_TBps": W * H * 3 * FRAMES / (compose * 1e-3) / 1e12 if compose > 0 else None,
    }
    Path(out_path).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec[scene]["kernel_trace"]))


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--trace-only"]:
        trace_only(args[1])
    elif args[:1] == ["--fold"]:
        fold(args[1], args[2], args[3] if len(args) > 3 else DEFAULT_OUT)
    else:
        main(args[0] if args else DEFAULT_OUT)
