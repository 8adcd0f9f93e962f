"""Time of the lat/lon cell heatmaps of naive plans (include/vet.h: vet_heatmap_create_latlon / vet_heatmap_render_binned*)
on one MI355X: 2 048 frames of 1 024 users (the default random-walk workload on the reference's 100 x 200 pixel grid)
rendered at 1200 x 600, for 10 x 20 degree cells (361 bins) and 1 x 1 degree cells (65 341 bins):
  * map build: vet_heatmap_create_latlon wall clock (k_heatmap_map_latlon + synchronise), median of ITERS;
  * bin-palette + fill, and bin-palette + fill + markers (vet_heatmap_render_binned into device memory), hipEvents on the
    launch stream, alternating for ROUNDS rounds with the spatial entry (vet_heatmap_render: palette + fill (+ markers) of
    the same video's f64 weights over the 501-tile lattice) so that clock and order effects fall on both alike;
  * the host path (samples -> device -> pinned -> numpy) frames/s: Heatmap.render_binned for both grids, and
    NaiveSpatialEntropyAnalyzer.render_heatmaps where compute_entropy accepts the grid.
The bin-palette kernel alone, and the split of every path into its kernels, come from a run per scene of this script under
`rocprofv3 --kernel-trace --stats` (`--trace-only SCENE`: one map build and 1 + ITERS device renders of that scene alone),
folded in by `--fold <kernel_stats.csv> SCENE`.
usage: python tools/naive_heatmap_timing.py [out.json]          (default: profiles/heatmap/naive_heatmap_timing.json)
       python tools/naive_heatmap_timing.py --trace-only cells_10x20|cells_1x1|spatial
       python tools/naive_heatmap_timing.py --fold kernel_stats.csv cells_10x20|cells_1x1|spatial [out.json]"""
import csv
import json
import os
import sys
import tempfile
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'viewport-entropy-toolkit_amd'))

W, H = 1200, 600
VW, VH = 100, 200
U, T, TC = 1024, 2048, 501
ITERS = 5
ROUNDS = 5
CELLS = {"cells_10x20": (10, 20), "cells_1x1": (1, 1)}          # (tile_height, tile_width) in degrees
DEFAULT_OUT = os.path.join(ROOT, "profiles", "heatmap", "naive_heatmap_timing.json")


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


class Setup:
    """The video on the device, the naive plans and heatmaps, and the spatial entry's weights of the same video."""

    def __init__(self, scenes):
        import numpy as np
        import torch
        import bench
        import viewport_entropy_toolkit as vt
        from viewport_entropy_toolkit import _native, _quantiser
        from viewport_entropy_toolkit.config import NaiveAnalyzerConfig
        self.dev = dev = torch.device('cuda', 0)
        self.eng = eng = _native.Engine(0)
        self.mu_h, self.mv_h = bench.synth_video(U, T, 1234, 0)
        self.mu, self.mv = torch.from_numpy(self.mu_h).to(dev), torch.from_numpy(self.mv_h).to(dev)
        self.stream = torch.cuda.Stream(device=dev)
        self.rgb = torch.empty((T, H, W, 3), dtype=torch.uint8, device=dev)
        self.naive = {}
        for scene in scenes:
            if scene == "spatial":
                plan = _native.Plan(eng, [_quantiser.lattice_xyz(TC)], 120.0, 2.0, True, VW, VH)
                n0 = plan.n_tiles[0]
                self.wts = torch.empty((T, n0), dtype=torch.float64, device=dev)
                self.present = torch.empty(T, dtype=torch.int32, device=dev)
                ent = torch.empty(T, dtype=torch.float64, device=dev)
                st = torch.zeros(2, dtype=torch.int32, device=dev)
                plan.spatial_device(self.mu.data_ptr(), self.mv.data_ptr(), U, T, ent.data_ptr(), d_weights=self.wts.data_ptr(),
                                    d_present=self.present.data_ptr(), d_status=st.data_ptr(), stream=self.stream.cuda_stream)
                self.stream.synchronize()
                assert int(st.sum()) == 0, "the timing video must be valid"
                self.spatial_plan, self.n_tiles = plan, n0
                self.hm_spatial = _native.Heatmap(eng, _quantiser.lattice_xyz(TC), W, H, VW, VH)
                continue
            th, tw = CELLS[scene]
            an = vt.NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(video_width=VW, video_height=VH, tile_height=th,
                                                                    tile_width=tw))
            plan = an._naive_plan()
            t0 = time.perf_counter()
            hm = _native.Heatmap.latlon(eng, tw, th, W, H, VW, VH)
            self.naive[scene] = (plan, hm, time.perf_counter() - t0)

    def naive_render(self, scene, markers):
        plan, hm, _ = self.naive[scene]
        hm.render_binned_device(plan, self.mu.data_ptr(), self.mv.data_ptr(), U, T, self.rgb.data_ptr(), markers=markers,
                                stream=self.stream.cuda_stream)

    def spatial_render(self, markers):
        mu, mv = (self.mu.data_ptr(), self.mv.data_ptr()) if markers else (0, 0)
        self.hm_spatial.render_device(self.wts.data_ptr(), self.present.data_ptr(), T, self.rgb.data_ptr(), mu, mv,
                                      U if markers else 0, stream=self.stream.cuda_stream)


def main(out_path):
    import numpy as np
    import torch
    import bench
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit import _native
    from viewport_entropy_toolkit.config import NaiveAnalyzerConfig
    s = Setup(["spatial", *CELLS])
    nbytes = s.rgb.numel()
    rec = {"tool": "tools/naive_heatmap_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "frame": [W, H],
           "video": [VW, VH], "users": U, "frames": T, "iters": ITERS, "rounds": ROUNDS, "bytes_written": nbytes}

    # map build: median of ITERS creates after the warm one of Setup
    for scene, (th, tw) in CELLS.items():
        ts = []
        for _ in range(ITERS):
            t0 = time.perf_counter()
            _native.Heatmap.latlon(s.eng, tw, th, W, H, VW, VH).close()
            ts.append(time.perf_counter() - t0)
        rec[scene] = {"tile_height": th, "tile_width": tw, "bins": s.naive[scene][1].n_tiles,
                      "map_build_ms": float(np.median(ts)) * 1e3}

    # the device paths, alternating with the spatial entry
    runs = {f"{k}_{m}": [] for k in [*CELLS, "spatial"] for m in ("fill", "markers")}
    for _ in range(ROUNDS):
        for markers in (False, True):
            m = "markers" if markers else "fill"
            for scene in CELLS:
                runs[f"{scene}_{m}"].append(timed(s.stream, lambda: s.naive_render(scene, markers)))
                runs[f"spatial_{m}"].append(timed(s.stream, lambda: s.spatial_render(markers)))
    med = {k: float(np.median(v)) for k, v in runs.items()}
    rec["spatial"] = {"tiles": s.n_tiles, "palette_fill_ms": med["spatial_fill"],
                      "palette_fill_markers_ms": med["spatial_markers"],
                      "palette_fill_ms_rounds": runs["spatial_fill"], "palette_fill_markers_ms_rounds": runs["spatial_markers"]}
    for scene in CELLS:
        r = rec[scene]
        r["bin_palette_fill_ms"] = med[f"{scene}_fill"]
        r["bin_palette_fill_markers_ms"] = med[f"{scene}_markers"]
        r["bin_palette_fill_ms_rounds"] = runs[f"{scene}_fill"]
        r["bin_palette_fill_markers_ms_rounds"] = runs[f"{scene}_markers"]
        r["vs_spatial_fill_time"] = med[f"{scene}_fill"] / med["spatial_fill"]
        r["vs_spatial_fill_markers_time"] = med[f"{scene}_markers"] / med["spatial_markers"]
        r["fill_write_TBps"] = nbytes / (med[f"{scene}_fill"] * 1e-3) / 1e12
    rec["timing"] = ("map build: wall clock of vet_heatmap_create_latlon (median of ITERS); device paths: torch.cuda.Event "
                     "around ITERS calls on one stream after one warm-up call, every naive scene alternating with the spatial "
                     "entry over the same 2 048 frames for ROUNDS rounds (medians); the spatial entry's weights are computed "
                     "once, outside the timing")
    del s
    torch.cuda.empty_cache()

    # the host path: the C-ABI host entry for both grids, and the analyzer where compute_entropy accepts the grid
    mu_h, mv_h = bench.synth_video(U, T, 1234, 0)
    n = 512
    eng = _native.Engine(0)
    with tempfile.TemporaryDirectory() as tmp:
        for scene, (th, tw) in CELLS.items():
            an = vt.NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(video_width=VW, video_height=VH, tile_height=th,
                                                                    tile_width=tw, output_dir=Path(tmp) / "out"))
            an.load_arrays(np.arange(T, dtype=np.float64), mu_h, mv_h)
            plan = an._naive_plan()
            hm = _native.Heatmap.latlon(eng, tw, th, W, H, VW, VH)
            hm.render_binned(plan, mu_h, mv_h, 0, 16)                 # staging buffers
            t0 = time.perf_counter()
            hm.render_binned(plan, mu_h, mv_h, 0, n)
            sec = time.perf_counter() - t0
            rec[scene]["render_binned_host"] = {"frames": n, "s": sec, "frames_per_s": n / sec,
                                                "GBps_to_host": n * H * W * 3 / sec / 1e9,
                                                "what": "Heatmap.render_binned (vet_heatmap_render_binned_host) of frames "
                                                        "[0, n) at 1200 x 600, markers on"}
            hm.close()
            try:
                an.compute_entropy()
            except (_native.NativeError, vt.ValidationError) as e:
                rec[scene]["render_heatmaps"] = {"skipped": f"compute_entropy refuses this grid: {e}"}
                continue
            an.render_heatmaps(frames=range(0, 16))                    # map, staging buffers
            t0 = time.perf_counter()
            an.render_heatmaps(frames=range(0, n))
            sec = time.perf_counter() - t0
            rec[scene]["render_heatmaps"] = {"frames": n, "s": sec, "frames_per_s": n / sec,
                                             "GBps_to_host": n * H * W * 3 / sec / 1e9,
                                             "what": "NaiveSpatialEntropyAnalyzer.render_heatmaps(frames=range(0, n)) at "
                                                     "1200 x 600, markers on"}
    out = Path(out_path)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


def trace_only(scene):
    """One map build (in Setup) and 1 + ITERS device renders of one scene, with markers: the run rocprofv3 traces."""
    s = Setup([scene])
    for _ in range(1 + ITERS):
        if scene == "spatial":
            s.spatial_render(True)
        else:
            s.naive_render(scene, True)
    s.stream.synchronize()


def fold(stats_csv, scene, out_path):
    """Per-kernel time of a --trace-only run (rocprofv3 kernel_stats.csv) into the scene's record, ms per render."""
    rec = json.loads(Path(out_path).read_text())
    names = ("k_heatmap_map_latlon", "k_heatmap_bin_palette", "k_heatmap_palette", "k_heatmap_fill", "k_heatmap_markers")
    kernels = {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            for key in names:
                if key + "<" in row["Name"] or key + "(" in row["Name"]:
                    k = kernels.setdefault(key, {"calls": 0, "total_ns": 0.0, "max_ns": 0.0})
                    k["calls"] += int(row["Calls"])
                    k["total_ns"] += float(row["TotalDurationNs"])
                    k["max_ns"] = max(k["max_ns"], float(row.get("MaxNs") or 0.0))
    renders = 1 + ITERS
    per = {k: v["total_ns"] / 1e6 / (1 if k == "k_heatmap_map_latlon" else renders) for k, v in kernels.items()}
    rec.setdefault(scene, {})["kernel_trace"] = {
        "what": f"rocprofv3 --kernel-trace --stats of tools/naive_heatmap_timing.py --trace-only {scene}: one map build, "
                f"{renders} renders of the {T} frames with markers; ms per render (map: per build)",
        "kernels": kernels, "ms": per,
        "fill_write_TBps": W * H * 3 * T / (per["k_heatmap_fill"] * 1e-3) / 1e12 if per.get("k_heatmap_fill") else None,
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
