"""Lat/lon cell heatmaps of naive plans on the GPU (include/vet.h: vet_heatmap_create_latlon / vet_heatmap_render_binned*;
NaiveSpatialEntropyAnalyzer.render_heatmaps / save_heatmaps) against the numpy oracle of tests/_naive_heatmap_oracle.py.

Each frame colours every pixel by its cell's users over the users present in the frame, the cells counted from the
samples through the plan's own quantiser and LUT.  The frames are checked bit for bit."""
import shutil

import numpy as np
import pandas as pd
import pytest

from tests import _heatmap_oracle as ho
from tests import _naive_heatmap_oracle as nho

pytestmark = pytest.mark.gpu

CELLS = [(10, 10), (30, 45), (20, 20), (90, 180), (180, 360), (1, 1)]      # (tile_height, tile_width) in degrees
GOLDEN = [(10, 10), (30, 45), (20, 20), (90, 180)]


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    return native.Engine.default()


def naive_plan(th, tw, VW, VH, weighted=True):
    """The naive analyzer's own plan for this grid."""
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import EntropyConfig, NaiveAnalyzerConfig
    an = vt.NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(video_width=VW, video_height=VH, tile_height=th,
                                                            tile_width=tw,
                                                            entropy_config=EntropyConfig(use_weight_distribution=weighted)))
    return an._naive_plan()


def samples(T, U, seed, out_of_range=True):
    """Random samples with users who leave, a frame with nobody (1) and, spread over frames 2-6, samples at px = 0,
    px = W and py = 0 (and, with out_of_range, outside [0, 1])."""
    rng = np.random.default_rng(seed)
    mu, mv = rng.random((T, U)), rng.random((T, U))
    leave = rng.integers(2, T, U)
    gone = (np.arange(T)[:, None] >= leave[None, :]) & (rng.random(U) < 0.3)[None, :]
    mu[gone] = np.nan
    mu[rng.random((T, U)) < 0.05] = np.nan
    mu[1] = np.nan
    mu[2, 0] = 0.0
    mu[3, U // 2] = 1.0
    mv[4, U - 1] = 0.0
    mu[5, 0], mv[5, 0] = 0.0, 0.0
    mu[5, U - 1], mv[5, U - 1] = 1.0, 1.0
    if out_of_range:
        mu[6, 0] = 1.5
        mv[6, U - 1] = -0.25
    return mu, mv


# --------------------------------------------------------------------------- frames against the oracle
@pytest.mark.parametrize("th,tw", CELLS)
@pytest.mark.parametrize("U", [1, 7, 1024, 5000])
@pytest.mark.parametrize("VW,VH", [(200, 100), (640, 480)])
def test_frames_bit_exact(native, engine, th, tw, U, VW, VH):
    W, H = (90, 45) if U != 7 else (97, 61)                           # 97 x 61: HW % 4 != 0
    T = 9
    mu, mv = samples(T, U, seed=U + th + VW)
    plan = naive_plan(th, tw, VW, VH)
    hm = native.Heatmap.latlon(engine, tw, th, W, H, VW, VH, 2)
    assert hm.n_tiles == nho.n_cells(tw, th) == plan.n_tiles[0]
    assert np.array_equal(hm.map(), nho.cell_map(tw, th, W, H))
    got = hm.render_binned(plan, mu, mv)
    assert got.shape == (T, H, W, 3) and got.dtype == np.uint8
    assert np.array_equal(got, nho.render(mu, mv, tw, th, W, H, VW, VH))
    assert (got[1] == 204).all()                                       # nobody present: grey
    plain = hm.render_binned(plan, mu, mv, markers=False)
    assert np.array_equal(plain, nho.render(mu, mv, tw, th, W, H, VW, VH, markers=False))


@pytest.mark.parametrize("th,tw", [(10, 20), (1, 1)])
def test_many_frames_in_blocks(native, engine, th, tw):
    """1200 x 600 frames: the host entry's two-buffer pipeline runs several sub-blocks; sub-ranges and a repeat agree."""
    T, U = 40, 64
    mu, mv = samples(T, U, seed=41)
    plan = naive_plan(th, tw, 1200, 600)
    hm = native.Heatmap.latlon(engine, tw, th, 1200, 600, 1200, 600, 3)
    whole = hm.render_binned(plan, mu, mv)
    assert np.array_equal(whole, nho.render(mu, mv, tw, th, 1200, 600, 1200, 600, radius=3))
    assert np.array_equal(hm.render_binned(plan, mu, mv), whole)
    out = np.empty((13, 600, 1200, 3), dtype=np.uint8)
    assert hm.render_binned(plan, mu, mv, row0=17, n=13, out=out) is out
    assert np.array_equal(out, whole[17:30])
    assert np.array_equal(hm.render_binned(plan, mu[17:30], mv[17:30]), whole[17:30])
    assert hm.render_binned(plan, mu, mv, row0=40, n=0).shape == (0, 600, 1200, 3)


def test_more_than_65535_users(native, engine):
    """U > 65535: one u32 count per cell (the packed 16-bit counts would carry); a grid too large for that is refused."""
    T, U = 3, 70000
    rng = np.random.default_rng(9)
    mu, mv = rng.random((T, U)), rng.random((T, U))
    mu[:, :66000] = 0.51                                               # 66 000 users in one cell: beyond 16 bits
    mv[:, :66000] = 0.52
    mu[2, 100:] = np.nan
    plan = naive_plan(20, 20, 200, 100)
    hm = native.Heatmap.latlon(engine, 20, 20, 64, 32, 200, 100)
    assert np.array_equal(hm.render_binned(plan, mu, mv), nho.render(mu, mv, 20, 20, 64, 32, 200, 100))
    big = native.Heatmap.latlon(engine, 1, 1, 64, 32, 200, 100)
    with pytest.raises(native.NativeError) as e:
        big.render_binned(naive_plan(1, 1, 200, 100), mu, mv)
    assert e.value.code == native.VET_ERR_UNSUPPORTED


def test_device_entry_matches_host_entry(native, engine):
    import torch
    T, U, W, H = 11, 33, 97, 61
    mu, mv = samples(T, U, seed=5)
    plan = naive_plan(30, 45, 640, 480)
    hm = native.Heatmap.latlon(engine, 45, 30, W, H, 640, 480)
    dev = torch.device("cuda", 0)
    dmu, dmv = torch.from_numpy(mu).to(dev), torch.from_numpy(mv).to(dev)
    stream = torch.cuda.current_stream(dev)
    for markers in (True, False):
        rgb = torch.full((T, H, W, 3), 7, dtype=torch.uint8, device=dev)
        hm.render_binned_device(plan, dmu.data_ptr(), dmv.data_ptr(), U, T, rgb.data_ptr(), markers=markers,
                                stream=stream.cuda_stream)
        stream.synchronize()
        want = hm.render_binned(plan, mu, mv, markers=markers)
        assert np.array_equal(rgb.cpu().numpy(), want)
        assert np.array_equal(want, nho.render(mu, mv, 45, 30, W, H, 640, 480, markers=markers))


# --------------------------------------------------------------------------- errors
def test_errors(native, engine):
    from oracle import vet_oracle as vo
    mu, mv = samples(7, 8, seed=2)
    plan = naive_plan(10, 20, 200, 100)
    hm = native.Heatmap.latlon(engine, 20, 10, 64, 32, 200, 100)
    cases = [
        (native.Heatmap(engine, vo.fibonacci_lattice(20), 64, 32, 200, 100), plan),      # a Fibonacci heatmap
        (hm, native.Plan(engine, [vo.fibonacci_lattice(20)], 120.0, 2.0, True, 200, 100)),  # lattice 0 not binned
        (hm, naive_plan(10, 10, 200, 100)),                                              # another bin count
        (hm, naive_plan(10, 20, 640, 480)),                                              # another video size
    ]
    for h, p in cases:
        with pytest.raises(native.NativeError) as e:
            h.render_binned(p, mu, mv)
        assert e.value.code == native.VET_ERR_INVALID
    fib = native.Plan(engine, [vo.fibonacci_lattice(20)], 120.0, 2.0, True, 200, 100)
    rng = np.random.default_rng(4)
    sp = fib.spatial_resident(mu=rng.random((6, 8)), mv=rng.random((6, 8)))
    with pytest.raises(native.NativeError) as e:                      # a lat/lon heatmap renders no result
        hm.render_result(sp["result"], sp["present"])
    assert e.value.code == native.VET_ERR_INVALID
    import torch
    dev = torch.device("cuda", 0)
    w = torch.zeros((2, hm.n_tiles), dtype=torch.float64, device=dev)
    c = torch.zeros((2, hm.n_tiles), dtype=torch.int32, device=dev)
    p = torch.ones(2, dtype=torch.int32, device=dev)
    rgb = torch.empty((2, 32, 64, 3), dtype=torch.uint8, device=dev)
    for render, rows in ((hm.render_device, w), (hm.render_counts_device, c)):   # nor cell-ordered weight rows
        with pytest.raises(native.NativeError) as e:
            render(rows.data_ptr(), p.data_ptr(), 2, rgb.data_ptr())
        assert e.value.code == native.VET_ERR_INVALID
    for tw, th in ((7, 10), (20, 7), (0, 10), (20, -10)):
        with pytest.raises(native.NativeError) as e:
            native.Heatmap.latlon(engine, tw, th, 64, 32, 200, 100)
        assert e.value.code == native.VET_ERR_INVALID
    with pytest.raises(native.NativeError) as e:
        native.Heatmap.latlon(engine, 20, 10, 64, 32, 200, 100, marker_radius=17)
    assert e.value.code == native.VET_ERR_INVALID
    lib = engine.lib
    assert lib.vet_heatmap_render_binned_host(hm.handle, plan.handle, mu.ctypes.data, mv.ctypes.data, 8, -1, 1,
                                              np.empty(1, np.uint8).ctypes.data) == native.VET_ERR_INVALID
    assert lib.vet_heatmap_render_binned_host(hm.handle, plan.handle, mu.ctypes.data, mv.ctypes.data, 0, 6, 1,
                                              np.empty(1, np.uint8).ctypes.data) == native.VET_ERR_INVALID


# --------------------------------------------------------------------------- the reference's own cell counts
def _write_g10(golden_dir, d):
    g = np.load(golden_dir / "g10_naive.npz")
    d.mkdir()
    for u in range(len(g["mu_in"])):
        pd.DataFrame({"time": g["time_in"][u], "2dmu": g["mu_in"][u], "2dmv": g["mv_in"][u], "x": 1}).to_csv(
            d / f"user{u:03d}.csv", index=False)
    return g


def _naive_analyzer(tmp_path, th, tw, flag=True):
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import EntropyConfig, NaiveAnalyzerConfig
    return vt.NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(
        output_dir=tmp_path / "out", tile_height=th, tile_width=tw,
        entropy_config=EntropyConfig(use_weight_distribution=flag)))


@pytest.mark.parametrize("th,tw", GOLDEN)
@pytest.mark.parametrize("flag", [True, False])
def test_golden_reference_cells(tmp_path, golden_dir, th, tw, flag):
    """Frames 0, 150, 299 are colour(count, present) of the reference's own per-frame cell dicts, grey elsewhere."""
    g = _write_g10(golden_dir, tmp_path / "video")
    an = _naive_analyzer(tmp_path, th, tw, flag)
    an.process_directory(tmp_path / "video")
    an.compute_entropy()
    W, H = 180, 90
    tag = f"h{th}_w{tw}_{'w' if flag else 'u'}"
    cmap = nho.cell_map(tw, th, W, H)
    mu = an._dense[1]
    for fi in (0, 150, 299):
        keys = [str(k) for k in g[f"{tag}__f{fi}_wkeys"]]
        vals = g[f"{tag}__f{fi}_wvals"]
        present = int(vals.sum())
        assert present == (~np.isnan(mu[fi])).sum()
        pal = np.full((nho.n_cells(tw, th), 3), 204, dtype=np.uint8)        # no user: grey
        for k, v in zip(keys, vals):
            li, lj = (int(x) for x in k.split("_"))
            pal[li * nho.n_lat(th) + lj] = ho.colour(v, present)
        got = an.render_heatmaps(frames=range(fi, fi + 1), width=W, height=H, markers=False)[0]
        assert np.array_equal(got, pal[cmap]), (tag, fi)


# --------------------------------------------------------------------------- the analyzer
def test_analyzer_render_and_writers(native, engine, tmp_path, golden_dir):
    from PIL import Image
    from viewport_entropy_toolkit.data_types import ValidationError
    _write_g10(golden_dir, tmp_path / "video")
    an = _naive_analyzer(tmp_path, 30, 45)
    an.process_directory(tmp_path / "video")
    res = an.compute_entropy()
    before = res.copy(deep=True)
    _, mu, mv, _ = an._dense
    VW, VH = an.config.video_width, an.config.video_height
    whole = an.render_heatmaps(width=160, height=80, marker_radius=1)
    assert whole.shape == (300, 80, 160, 3)
    assert np.array_equal(whole, nho.render(mu, mv, 45, 30, 160, 80, VW, VH, radius=1))
    frames = an.render_heatmaps(frames=range(20, 37), width=160, height=80)
    assert np.array_equal(frames, nho.render(mu[20:37], mv[20:37], 45, 30, 160, 80, VW, VH))
    assert np.array_equal(an.render_heatmaps(frames=slice(20, 37), width=160, height=80), frames)
    assert np.array_equal(an.render_heatmaps(frames=range(20, 37), width=160, height=80, markers=False),
                          nho.render(mu[20:37], mv[20:37], 45, 30, 160, 80, VW, VH, markers=False))
    npy = an.save_heatmaps(tmp_path / "h.npy", width=160, height=80, marker_radius=1, block_frames=64)
    assert np.array_equal(np.load(npy), whole)
    pngs = tmp_path / "png"
    pngs.mkdir()
    an.save_heatmaps(pngs, frames=range(20, 37), width=160, height=80, block_frames=7)
    names = sorted(p.name for p in pngs.iterdir())
    assert names == [f"frame_{t:06d}.png" for t in range(20, 37)]
    for j, t in enumerate(range(20, 37)):
        assert np.array_equal(np.asarray(Image.open(pngs / f"frame_{t:06d}.png").convert("RGB")), frames[j])
    if shutil.which("ffmpeg"):
        mp4 = an.save_heatmaps(tmp_path / "h.mp4", frames=range(0, 12), width=160, height=80)
        assert mp4.stat().st_size > 0
    else:
        with pytest.raises(RuntimeError):
            an.save_heatmaps(tmp_path / "h.mp4", width=160, height=80)
        assert not (tmp_path / "h.mp4").exists()
    with pytest.raises(ValidationError):
        an.save_heatmaps(tmp_path / "odd.mp4", width=161, height=80)
    with pytest.raises(ValidationError):
        an.render_heatmaps(marker_radius=17, width=16, height=8)
    with pytest.raises(ValidationError):
        an.render_heatmaps(frames=range(0, 301))
    default = an.render_heatmaps(frames=range(0, 2))                  # figure_size x dpi
    assert default.shape == (2, 600, 1200, 3)
    assert np.array_equal(default, nho.render(mu[:2], mv[:2], 45, 30, 1200, 600, VW, VH))
    # compute_entropy's frame is untouched by rendering, and a second run gives the same frame
    pd.testing.assert_frame_equal(an._entropy_results, before)
    pd.testing.assert_frame_equal(an.compute_entropy(), before)
    assert all(w is None for w in an._entropy_results["tile_weights"])


def test_analyzer_renders_the_last_compute(native, engine, tmp_path):
    """The cells and samples are those of the last compute_entropy, not of a config changed since."""
    rng = np.random.default_rng(13)
    T, U = 20, 30
    mu, mv = rng.random((T, U)), rng.random((T, U))
    mu[rng.random((T, U)) < 0.2] = np.nan
    mu[:, 0] = rng.random(T)                                           # no empty frame
    an = _naive_analyzer(tmp_path, 10, 20)
    an.load_arrays(np.arange(T, dtype=np.float64), mu, mv)
    an.compute_entropy()
    an.config.tile_width = 45
    got = an.render_heatmaps(width=120, height=60)
    VW, VH = an.config.video_width, an.config.video_height
    assert np.array_equal(got, nho.render(mu, mv, 20, 10, 120, 60, VW, VH))
    an.compute_entropy()
    assert np.array_equal(an.render_heatmaps(width=120, height=60), nho.render(mu, mv, 45, 10, 120, 60, VW, VH))
