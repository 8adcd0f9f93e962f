"""Time of the per-frame tile-attention heatmaps (include/vet.h: vet_heatmap_*) on one MI355X:
  * the pixel -> tile map (vet_heatmap_create: k_heatmap_map) for 500 and 1001 tiles at 1200 x 600, wall clock;
  * palette + fill (+ markers) for a config-3-shaped block resident on the device (1024 users, 2048 frames, 501 tiles, the
    reference's 100 x 200 pixel grid), hipEvents on the launch stream: ms per frame and written TB/s, beside a device-to-device
    copy of the same bytes in the same run;
  * SpatialEntropyAnalyzer.render_heatmaps frames/s through the host path (device-resident result -> pinned -> numpy);
  * save_heatmaps(.npy) to tmpfs.
usage: python tools/heatmap_timing.py [out.json]      (default: profiles/heatmap/heatmap_timing.json)"""
import json
import os
import sys
import tempfile
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'viewport-entropy-toolkit_amd'))
import numpy as np
import torch
from viewport_entropy_toolkit import _native, _quantiser
import bench

W, H = 1200, 600
VW, VH = 100, 200
U, T, TC = 1024, 2048, 501
ITERS = 5


def timed(stream, fn, iters=ITERS):
    fn()                                                   # warm-up
    stream.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / iters


def main(out_path):
    dev = torch.device('cuda', 0)
    eng = _native.Engine(0)
    rec = {"tool": "tools/heatmap_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "frame": [W, H], "iters": ITERS}

    # 1. the map
    maps = []
    for tc in (500, 1001):
        tiles = _quantiser.lattice_xyz(tc)
        _native.Heatmap(eng, tiles, W, H, VW, VH).close()          # module load, first-use costs
        t0 = time.perf_counter()
        hm = _native.Heatmap(eng, tiles, W, H, VW, VH)
        maps.append({"tile_count": tc, "tiles": len(tiles), "create_ms": (time.perf_counter() - t0) * 1e3})
        hm.close()
    rec["map_build"] = {"what": "vet_heatmap_create wall clock: H2D of the tiles + k_heatmap_map + synchronise", "runs": maps}

    # 2. fill (+ markers) of a resident config-3-shaped block
    mu_h, mv_h = bench.synth_video(U, T, 1234, 0)
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(TC)], 120.0, 2.0, True, VW, VH)
    n0 = plan.n_tiles[0]
    mu, mv = torch.from_numpy(mu_h).to(dev), torch.from_numpy(mv_h).to(dev)
    ent = torch.empty(T, dtype=torch.float64, device=dev)
    wts = torch.empty((T, n0), dtype=torch.float64, device=dev)
    present = torch.empty(T, dtype=torch.int32, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        plan.spatial_device(mu.data_ptr(), mv.data_ptr(), U, T, ent.data_ptr(), d_weights=wts.data_ptr(),
                            d_present=present.data_ptr(), d_status=st.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    hm = _native.Heatmap(eng, _quantiser.lattice_xyz(TC), W, H, VW, VH)
    rgb = torch.empty((T, H, W, 3), dtype=torch.uint8, device=dev)
    copy = torch.empty_like(rgb)
    nbytes = rgb.numel()

    def fill():
        hm.render_device(wts.data_ptr(), present.data_ptr(), T, rgb.data_ptr(), stream=stream.cuda_stream)

    def fill_markers():
        hm.render_device(wts.data_ptr(), present.data_ptr(), T, rgb.data_ptr(), mu.data_ptr(), mv.data_ptr(), U,
                         stream=stream.cuda_stream)

    def d2d():
        with torch.cuda.stream(stream):
            copy.copy_(rgb)

    ms_fill, ms_mark, ms_copy = timed(stream, fill), timed(stream, fill_markers), timed(stream, d2d)
    rec["device_block"] = {
        "users": U, "frames": T, "tiles": n0, "bytes_written": nbytes,
        "palette_fill_ms": ms_fill, "palette_fill_markers_ms": ms_mark, "d2d_copy_ms": ms_copy,
        "palette_fill_us_per_frame": ms_fill * 1e3 / T, "palette_fill_markers_us_per_frame": ms_mark * 1e3 / T,
        "fill_write_TBps": nbytes / (ms_fill * 1e-3) / 1e12,
        "fill_markers_write_TBps": nbytes / (ms_mark * 1e-3) / 1e12,
        "d2d_copy_write_TBps": nbytes / (ms_copy * 1e-3) / 1e12,
        "d2d_copy_read_plus_write_TBps": 2 * nbytes / (ms_copy * 1e-3) / 1e12,
        "fill_vs_copy_write_rate": ms_copy / ms_fill,
        "timing": "torch.cuda.Event around ITERS calls on one stream after one warm-up call; TB/s = RGB bytes / time",
    }
    del rgb, copy
    torch.cuda.empty_cache()

    # 3 + 4. the host path through the analyzer
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import AnalyzerConfig
    with tempfile.TemporaryDirectory() as tmp:
        an = vt.SpatialEntropyAnalyzer(AnalyzerConfig(video_width=VW, video_height=VH, tile_counts=[TC],
                                                      output_dir=Path(tmp) / "out"))
        an.load_arrays(np.arange(T, dtype=np.float64), mu_h, mv_h)
        an.compute_entropy()
        an.render_heatmaps(frames=range(0, 16))                        # map, staging buffers
        n = 512
        t0 = time.perf_counter()
        an.render_heatmaps(frames=range(0, n))
        s_render = time.perf_counter() - t0
        rec["render_heatmaps"] = {"frames": n, "s": s_render, "frames_per_s": n / s_render,
                                  "GBps_to_host": n * H * W * 3 / s_render / 1e9,
                                  "what": "render_heatmaps(frames=range(0, n)) at 1200 x 600, markers on, lazy weight rows"}
        shm = Path("/dev/shm") if Path("/dev/shm").is_dir() else Path(tmp)
        with tempfile.TemporaryDirectory(dir=shm) as d:
            t0 = time.perf_counter()
            an.save_heatmaps(Path(d) / "h.npy", frames=range(0, n))
            s_save = time.perf_counter() - t0
        rec["save_heatmaps_npy"] = {"frames": n, "s": s_save, "frames_per_s": n / s_save,
                                    "GBps": n * H * W * 3 / s_save / 1e9, "where": "tmpfs", "block_frames": 256}
    out = Path(out_path)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "heatmap", "heatmap_timing.json"))
