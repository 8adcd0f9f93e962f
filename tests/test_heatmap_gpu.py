"""Per-frame tile-attention heatmaps on the GPU (include/vet.h: vet_heatmap_*; SpatialEntropyAnalyzer.render_heatmaps /
save_heatmaps) against the numpy oracle of tests/_heatmap_oracle.py.

The pixel -> tile map is checked against the oracle's first minimum (only near-ties may differ); the frames are checked bit
for bit against the oracle's palette gathered through the device's own map, so that check does not rest on near-ties."""
import shutil

import numpy as np
import pandas as pd
import pytest

from oracle import vet_oracle as vo
from tests import _heatmap_oracle as ho

pytestmark = pytest.mark.gpu

VW, VH = 1200, 600


@pytest.fixture(scope="module")
def native():
    from viewport_entropy_toolkit import _native
    return _native


@pytest.fixture(scope="module")
def engine(native):
    return native.Engine.default()


def walk(U, T, seed, p_absent=0.1):
    from viewport_entropy_toolkit import _synthetic
    return _synthetic.random_walk_video(U, T, base_seed=seed, p_absent=p_absent)


def plan_of(native, engine, tcs, weighted=True, power=2.0, fov=120.0, fp64=False):
    plan = native.Plan(engine, [vo.fibonacci_lattice(t) for t in tcs], fov, power, weighted, VW, VH)
    if fp64:
        plan.set_fp64(True)
    return plan


def check_result(native, engine, plan, mu, mv, tcs, W, H, radius=2, markers=True):
    """Renders every frame of plan's resident result and compares it with the oracle; returns (frames, weights)."""
    res = plan.spatial_resident(mu=mu, mv=mv, check=False)
    result, present = res["result"], res["present"]
    weights = result.rows(1, 0, len(mu))
    hm = native.Heatmap(engine, vo.fibonacci_lattice(tcs[0]), W, H, VW, VH, radius)
    tile_map = hm.map()
    got = hm.render_result(result, present, mu if markers else None, mv if markers else None)
    want = ho.render(tile_map, weights, present, mu if markers else None, mv if markers else None, VW, VH, radius)
    assert got.shape == (len(mu), H, W, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want)
    return got, weights, hm, result, present


# --------------------------------------------------------------------------- the map
@pytest.mark.parametrize("W,H", [(1200, 600), (97, 61)])
@pytest.mark.parametrize("tc", [20, 50, 501, 1001])
def test_map_matches_first_minimum(native, engine, W, H, tc):
    tiles = vo.fibonacci_lattice(tc)
    hm = native.Heatmap(engine, tiles, W, H, VW, VH)
    m = hm.map()
    assert m.shape == (H, W) and m.min() >= 0 and m.max() < len(tiles)
    differ, ties = ho.near_ties(m, tiles, W, H)
    print(f"map {W}x{H} tc={tc}: {differ} pixel(s) differ from the oracle, {ties} of them near-ties (<= 4 ulp)")
    assert differ == ties
    assert len(np.unique(m)) > min(len(tiles), W * H) // 2           # a real tiling, not a constant


# --------------------------------------------------------------------------- fill, bit-exact
@pytest.mark.parametrize("kw,tcs,U", [
    pytest.param({}, [50], 16, id="weighted-lazy"),
    pytest.param({}, [20], 200, id="weighted-stored"),
    pytest.param(dict(weighted=False), [50], 16, id="nearest-tile"),
    pytest.param(dict(fp64=True), [50], 16, id="fp64"),
    pytest.param({}, [50, 100, 200], 16, id="three-lattices"),
])
@pytest.mark.parametrize("W,H", [(128, 64), (97, 61)])
def test_fill_bit_exact(native, engine, kw, tcs, U, W, H):
    mu, mv = walk(U, 33, seed=7)
    plan = plan_of(native, engine, tcs, **kw)
    got, weights, *_ = check_result(native, engine, plan, mu, mv, tcs, W, H)
    n0 = 2 * (tcs[0] // 2) + 1
    lazy = U * 4 <= n0 * 8
    assert lazy == (U == 16)
    assert (weights > 0).any() and len(np.unique(got.reshape(-1, 3), axis=0)) > 3
    plan.close()


def test_frames_without_users_are_grey(native, engine):
    mu, mv = walk(16, 9, seed=3)
    mu[[0, 4, 8]] = np.nan
    plan = plan_of(native, engine, [50])
    got, _, _, _, present = check_result(native, engine, plan, mu, mv, [50], 97, 61)
    assert present[[0, 4, 8]].tolist() == [0, 0, 0]
    assert (got[[0, 4, 8]] == 204).all()
    plan.close()


def test_negative_zero_keys(native, engine):
    """A tile in some FoV whose weight underflowed is the key -0.0: grey, like a tile no user sees."""
    mu, mv = walk(16, 20, seed=11)
    plan = plan_of(native, engine, [50], power=400.0)
    _, weights, *_ = check_result(native, engine, plan, mu, mv, [50], 97, 61)
    assert ((weights == 0) & np.signbit(weights)).any()
    plan.close()


# --------------------------------------------------------------------------- against the reference's values
def _analyzer_on_g4(tmp_path, golden_dir, tcs, weighted):
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import AnalyzerConfig
    from viewport_entropy_toolkit.utilities import EntropyConfig
    g = np.load(golden_dir / "g4_spatial.npz")
    d = tmp_path / "video"
    d.mkdir()
    for u in range(len(g["mu_in"])):
        pd.DataFrame({"time": g["time_in"][u], "2dmu": g["mu_in"][u], "2dmv": g["mv_in"][u], "x": 1}).to_csv(
            d / f"user{u:03d}.csv", index=False)
    an = vt.SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=tcs, output_dir=tmp_path / "out",
                                                  entropy_config=EntropyConfig(use_weight_distribution=weighted)))
    an.process_directory(d)
    an.compute_entropy()
    return g, an


@pytest.mark.parametrize("tag,weighted", [("w_tc50", True), ("u_tc50", False)])
def test_golden_weights(native, engine, tmp_path, golden_dir, tag, weighted):
    g, an = _analyzer_on_g4(tmp_path, golden_dir, [50], weighted)
    frames = g[f"{tag}__weights_frames"]
    _, mu, mv, _ = an._dense
    hm = native.Heatmap(engine, vo.fibonacci_lattice(50), 1200, 600, VW, VH)
    tile_map = hm.map()
    for j, f in enumerate(frames):
        got = an.render_heatmaps(frames=range(int(f), int(f) + 1))
        want = ho.render(tile_map, g[f"{tag}__weights"][j:j + 1], an._present[f:f + 1], mu[f:f + 1], mv[f:f + 1],
                         an.config.video_width, an.config.video_height, 2)
        assert got.shape == (1, 600, 1200, 3)
        assert np.array_equal(got, want), f"frame {f}"


# --------------------------------------------------------------------------- markers
def test_markers_edges_and_absent_users(native, engine):
    T, U = 6, 8
    mu, mv = walk(U, T, seed=5, p_absent=0.0)
    mu[0, :4] = [0.0, 1.0, 1.0, 0.0]
    mv[0, :4] = [0.0, 1.0, 0.0, 1.0]
    mu[1, 2] = np.nan                                   # absent
    mu[2, :3] = [0.9999999, 0.5, 0.0004]
    plan = plan_of(native, engine, [50])
    for radius in (0, 2, 3):
        got, *_ = check_result(native, engine, plan, mu, mv, [50], 97, 61, radius=radius)
        assert (got[0, 0, 0] == 0).all() and (got[0, 60, 96] == 0).all() and (got[0, 0, 96] == 0).all()
    got_off, weights, hm, result, present = check_result(native, engine, plan, mu, mv, [50], 97, 61, markers=False)
    assert np.array_equal(got_off, ho.render(hm.map(), weights, present))
    plan.close()


def test_out_of_range_samples_draw_nothing(native, engine):
    mu, mv = walk(8, 4, seed=9, p_absent=0.0)
    mu[1, 3] = 1.5
    plan = plan_of(native, engine, [50])
    res = plan.spatial_resident(mu=mu, mv=mv, check=False)
    assert res["code"] == native.VET_ERR_RANGE
    hm = native.Heatmap(engine, vo.fibonacci_lattice(50), 97, 61, VW, VH)
    got = hm.render_result(res["result"], res["present"], mu, mv)
    want = ho.render(hm.map(), res["result"].rows(1, 0, 4), res["present"], mu, mv, VW, VH, 2)
    assert np.array_equal(got, want)
    plan.close()


# --------------------------------------------------------------------------- blocks, repeatability, device pointers
def test_blocks_and_repeat(native, engine):
    """40 frames at 1200 x 600 are three sub-blocks of the two-buffer pipeline; blocks of 7 frames give the same bytes."""
    T = 40
    mu, mv = walk(24, T, seed=13)
    plan = plan_of(native, engine, [50])
    whole, weights, hm, result, present = check_result(native, engine, plan, mu, mv, [50], 1200, 600)
    parts = [hm.render_result(result, present[r:r + 7], mu[r:r + 7], mv[r:r + 7], row0=r, n=min(7, T - r))
             for r in range(0, T, 7)]
    assert np.array_equal(np.concatenate(parts), whole)
    assert np.array_equal(hm.render_result(result, present, mu, mv), whole)
    plan.close()


def test_render_device_matches_render_result(native, engine):
    import torch
    T, U, n = 13, 16, 51
    mu, mv = walk(U, T, seed=17)
    plan = plan_of(native, engine, [50])
    want, weights, hm, result, present = check_result(native, engine, plan, mu, mv, [50], 97, 61)
    dev = torch.device("cuda", 0)
    w = torch.from_numpy(weights).to(dev)
    p = torch.from_numpy(present).to(dev)
    dmu, dmv = torch.from_numpy(mu).to(dev), torch.from_numpy(mv).to(dev)
    rgb = torch.full((T, 61, 97, 3), 7, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    hm.render_device(w.data_ptr(), p.data_ptr(), T, rgb.data_ptr(), dmu.data_ptr(), dmv.data_ptr(), U,
                     stream=stream.cuda_stream)
    stream.synchronize()
    assert weights.shape == (T, n)
    assert np.array_equal(rgb.cpu().numpy(), want)
    plain = torch.zeros_like(rgb)
    hm.render_device(w.data_ptr(), p.data_ptr(), T, plain.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(plain.cpu().numpy(), ho.render(hm.map(), weights, present))
    plan.close()


# --------------------------------------------------------------------------- errors
def test_errors(native, engine):
    tiles = vo.fibonacci_lattice(50)
    with pytest.raises(native.NativeError) as e:
        native.Heatmap(engine, tiles, 97, 61, VW, VH, marker_radius=17)
    assert e.value.code == native.VET_ERR_INVALID
    with pytest.raises(native.NativeError) as e:
        native.Heatmap(engine, tiles, 0, 61, VW, VH)
    assert e.value.code == native.VET_ERR_INVALID
    with pytest.raises(native.NativeError) as e:
        native.Heatmap(engine, vo.fibonacci_lattice(7001), 97, 61, VW, VH)
    assert e.value.code == native.VET_ERR_UNSUPPORTED
    mu, mv = walk(8, 5, seed=2, p_absent=0.0)
    plan = plan_of(native, engine, [50])
    hm = native.Heatmap(engine, vo.fibonacci_lattice(20), 97, 61, VW, VH)
    res = plan.spatial_resident(mu=mu, mv=mv)
    with pytest.raises(native.NativeError) as e:                     # lattice of another size
        hm.render_result(res["result"], res["present"])
    assert e.value.code == native.VET_ERR_INVALID
    tr = plan.transition_resident(mu=mu, mv=mv)
    hm50 = native.Heatmap(engine, tiles, 97, 61, VW, VH)
    with pytest.raises(native.NativeError) as e:
        hm50.render_result(tr["result"], tr["common"])
    assert e.value.code == native.VET_ERR_INVALID
    plan.close()


# --------------------------------------------------------------------------- the analyzer
def test_analyzer_render_and_writers(native, tmp_path, golden_dir):
    from PIL import Image
    from viewport_entropy_toolkit.data_types import ValidationError
    g, an = _analyzer_on_g4(tmp_path, golden_dir, [50, 100], True)
    frames = an.render_heatmaps(frames=range(20, 37), width=160, height=80)
    assert frames.shape == (17, 80, 160, 3)
    assert np.array_equal(an.render_heatmaps(frames=slice(20, 37), width=160, height=80), frames)
    whole = an.render_heatmaps(width=160, height=80, marker_radius=1)
    assert whole.shape == (300, 80, 160, 3)
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


def test_analyzer_default_size_and_fp64(native, tmp_path, golden_dir):
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import AnalyzerConfig
    g, an = _analyzer_on_g4(tmp_path, golden_dir, [50], True)
    a = an.render_heatmaps(frames=range(0, 3))
    assert a.shape == (3, 600, 1200, 3)
    an64 = vt.SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=[50], output_dir=tmp_path / "out64"), fp64=True)
    an64.process_directory(tmp_path / "video")
    an64.compute_entropy()
    assert np.array_equal(an64.render_heatmaps(frames=range(0, 3)), a)     # same tile_weights values, same frames


def test_analyzer_vectors_render_without_markers(native, tmp_path, golden_dir):
    g, an = _analyzer_on_g4(tmp_path, golden_dir, [50], True)
    with_markers = an.render_heatmaps(frames=range(0, 5), width=160, height=80)
    an._data_cache["vectors"] = an._data_cache["vectors"]          # hand-assigned frame table: the ids path
    an.compute_entropy()
    assert an._marker_samples is None
    plain = an.render_heatmaps(frames=range(0, 5), width=160, height=80)
    assert np.array_equal(plain, an.render_heatmaps(frames=range(0, 5), width=160, height=80, markers=False))
    assert not np.array_equal(plain, with_markers)
    assert (with_markers == 0).all(-1).any() and not (plain == 0).all(-1).any()
