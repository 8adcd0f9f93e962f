"""Time of the per-frame heatmaps of transition results (include/vet.h: vet_heatmap_render_counts /
vet_heatmap_render_transition_result) on one MI355X, in tools/heatmap_timing.py's shape so that the numbers compare:
  * palette + fill (+ markers) of a config-3-shaped transition result resident on the device (1024 users, 2048 frames ->
    2047 rows of source-tile counts, 501 tiles, the reference's 100 x 200 pixel grid) at 1200 x 600, hipEvents on the
    launch stream, beside the spatial path (f64 weights of the same video) and a device-to-device copy of the same bytes in
    the same run;
  * TransitionEntropyAnalyzer.render_heatmaps frames/s through the host path (device-resident result -> pinned -> numpy);
  * save_heatmaps(.npy) to tmpfs.
usage: python tools/transition_heatmap_timing.py [out.json]   (default: profiles/heatmap/transition_heatmap_timing.json)"""
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
ROUNDS = 5


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
    rec = {"tool": "tools/transition_heatmap_timing.py", "kernel_src_sha16": bench.kernel_src_sha(), "frame": [W, H],
           "iters": ITERS, "rounds": ROUNDS}

    # 1. palette + fill (+ markers) of a resident config-3-shaped transition result, and the spatial path beside it
    mu_h, mv_h = bench.synth_video(U, T, 1234, 0)
    R = T - 1
    plan = _native.Plan(eng, [_quantiser.lattice_xyz(TC)], 120.0, 2.0, True, VW, VH)
    n0 = plan.n_tiles[0]
    mu, mv = torch.from_numpy(mu_h).to(dev), torch.from_numpy(mv_h).to(dev)
    ent = torch.empty(T, dtype=torch.float64, device=dev)
    pairs = torch.empty((R, U, 2), dtype=torch.int32, device=dev)
    counts = torch.empty((R, n0), dtype=torch.int32, device=dev)
    common = torch.empty(R, dtype=torch.int32, device=dev)
    wts = torch.empty((T, n0), dtype=torch.float64, device=dev)
    present_s = torch.empty(T, dtype=torch.int32, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        plan.transition_device(mu.data_ptr(), mv.data_ptr(), U, T, ent.data_ptr(), d_pairs=pairs.data_ptr(),
                               d_srccount=counts.data_ptr(), d_common=common.data_ptr(), d_status=st.data_ptr(),
                               stream=stream.cuda_stream)
        plan.spatial_device(mu.data_ptr(), mv.data_ptr(), U, T, ent.data_ptr(), d_weights=wts.data_ptr(),
                            d_present=present_s.data_ptr(), d_status=st.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert int(st.sum()) == 0, "the timing video must be valid"
    present = torch.from_numpy((~(np.isnan(mu_h) | np.isnan(mv_h)))[:-1].sum(axis=1).astype(np.int32)).to(dev)
    hm = _native.Heatmap(eng, _quantiser.lattice_xyz(TC), W, H, VW, VH)
    rgb = torch.empty((R, H, W, 3), dtype=torch.uint8, device=dev)
    copy = torch.empty_like(rgb)
    nbytes = rgb.numel()

    def fill():
        hm.render_counts_device(counts.data_ptr(), present.data_ptr(), R, rgb.data_ptr(), stream=stream.cuda_stream)

    def fill_markers():
        hm.render_counts_device(counts.data_ptr(), present.data_ptr(), R, rgb.data_ptr(), mu.data_ptr(), mv.data_ptr(), U,
                                stream=stream.cuda_stream)

    def spatial_fill():
        hm.render_device(wts.data_ptr(), present_s.data_ptr(), R, rgb.data_ptr(), stream=stream.cuda_stream)

    def d2d():
        with torch.cuda.stream(stream):
            copy.copy_(rgb)

    # the two palette + fill paths alternate (ROUNDS times each) so that clock and order effects fall on both alike
    fills, spatial = [], []
    for _ in range(ROUNDS):
        fills.append(timed(stream, fill))
        spatial.append(timed(stream, spatial_fill))
    ms_fill, ms_sp = float(np.median(fills)), float(np.median(spatial))
    ms_mark, ms_copy = timed(stream, fill_markers), timed(stream, d2d)
    rec["device_block"] = {
        "users": U, "frames": T, "rows": R, "tiles": n0, "bytes_written": nbytes,
        "palette_fill_ms": ms_fill, "palette_fill_markers_ms": ms_mark,
        "spatial_palette_fill_ms_same_rows": ms_sp, "d2d_copy_ms": ms_copy,
        "palette_fill_ms_rounds": fills, "spatial_palette_fill_ms_rounds": spatial,
        "palette_fill_us_per_frame": ms_fill * 1e3 / R, "palette_fill_markers_us_per_frame": ms_mark * 1e3 / R,
        "fill_write_TBps": nbytes / (ms_fill * 1e-3) / 1e12,
        "fill_markers_write_TBps": nbytes / (ms_mark * 1e-3) / 1e12,
        "d2d_copy_write_TBps": nbytes / (ms_copy * 1e-3) / 1e12,
        "fill_vs_spatial_time": ms_fill / ms_sp,
        "fill_vs_copy_write_rate": ms_copy / ms_fill,
        "timing": "torch.cuda.Event around ITERS calls on one stream after one warm-up call; TB/s = RGB bytes / time; the "
                  "spatial entry renders the first R rows of the same video's f64 weights into the same buffer, alternating "
                  "with the transition entry for ROUNDS rounds (medians)",
    }
    del rgb, copy
    torch.cuda.empty_cache()

    # 2 + 3. the host path through the analyzer
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import AnalyzerConfig
    with tempfile.TemporaryDirectory() as tmp:
        an = vt.TransitionEntropyAnalyzer(AnalyzerConfig(video_width=VW, video_height=VH, tile_counts=[TC],
                                                         output_dir=Path(tmp) / "out"))
        an.load_arrays(np.arange(T, dtype=np.float64), mu_h, mv_h)
        an.compute_entropy()
        an.render_heatmaps(frames=range(0, 16))                        # map, staging buffers, presence counts
        n = 512
        t0 = time.perf_counter()
        an.render_heatmaps(frames=range(0, n))
        s_render = time.perf_counter() - t0
        rec["render_heatmaps"] = {"frames": n, "s": s_render, "frames_per_s": n / s_render,
                                  "GBps_to_host": n * H * W * 3 / s_render / 1e9,
                                  "what": "TransitionEntropyAnalyzer.render_heatmaps(frames=range(0, n)) at 1200 x 600, "
                                          "markers on"}
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
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "heatmap", "transition_heatmap_timing.json"))
