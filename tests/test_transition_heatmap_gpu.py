"""Per-frame heatmaps of transition results on the GPU (include/vet.h: vet_heatmap_render_counts /
vet_heatmap_render_transition_result; TransitionEntropyAnalyzer.render_heatmaps / save_heatmaps) against the numpy oracle of
tests/_heatmap_oracle.py.

Row r of a transition result (frames r -> r+1) is coloured by srccount[r][tile] / users present in frame r, with frame r's
markers.  The frames are checked bit for bit against the oracle's palette gathered through the device's own map."""
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


def plan_of(native, engine, tcs):
    return native.Plan(engine, [vo.fibonacci_lattice(t) for t in tcs], 120.0, 2.0, True, VW, VH)


def prior_present(mu, mv):
    """Users present in frame r, r = 0 .. T-2."""
    return (~(np.isnan(mu) | np.isnan(mv)))[:-1].sum(axis=1).astype(np.int32)


def check_result(native, engine, plan, mu, mv, tcs, W, H, radius=2, markers=True):
    """Renders every row of plan's resident transition result and compares it with the oracle."""
    tr = plan.transition_resident(mu=mu, mv=mv)
    result, R = tr["result"], len(mu) - 1
    counts = result.rows(1, 0, R)
    present = prior_present(mu, mv)
    smu, smv = (mu[:-1], mv[:-1]) if markers else (None, None)
    hm = native.Heatmap(engine, vo.fibonacci_lattice(tcs[0]), W, H, VW, VH, radius)
    tile_map = hm.map()
    got = hm.render_transition_result(result, present, smu, smv)
    want = ho.render(tile_map, counts, present, smu, smv, VW, VH, radius)
    assert got.shape == (R, H, W, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want)
    return got, counts, hm, result, present, tr["common"]


# --------------------------------------------------------------------------- bit-exact against the oracle
@pytest.mark.parametrize("tcs", [[50], [20], [50, 100, 200]], ids=["tc50", "tc20", "three-lattices"])
@pytest.mark.parametrize("W,H", [(128, 64), (97, 61)])
def test_counts_bit_exact(native, engine, tcs, W, H):
    mu, mv = walk(16, 33, seed=7, p_absent=0.2)
    plan = plan_of(native, engine, tcs)
    got, counts, _, _, present, common = check_result(native, engine, plan, mu, mv, tcs, W, H)
    n0 = 2 * (tcs[0] // 2) + 1
    assert counts.shape == (32, n0) and counts.dtype == np.int32
    assert np.array_equal(counts.sum(axis=1), common)                  # every common user counted at its source tile
    assert (present > common).any()                                    # users who leave at r+1: n is not h_common
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 3
    plan.close()


def test_more_than_4096_users(native, engine):
    """U > 4 096: the counts come from k_transition_big."""
    mu, mv = walk(5000, 5, seed=19, p_absent=0.1)
    plan = plan_of(native, engine, [50])
    got, counts, _, _, present, common = check_result(native, engine, plan, mu, mv, [50], 97, 61)
    assert (present > common).all() and (counts.max(axis=1) > 100).all()
    assert len(np.unique(got[..., 0])) > 3
    plan.close()


# --------------------------------------------------------------------------- against the reference's counts
def _analyzer_on_g5(tmp_path, golden_dir, tag, tcs):
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import AnalyzerConfig
    g = np.load(golden_dir / "g5_transition.npz")
    cols = [str(c) for c in g[f"{tag}__columns"]]
    order = [int(c[4:]) for c in cols]
    times, mu, mv = vo.format_trajectories([(g["time_in"][u], g["mu_in"][u], g["mv_in"][u]) for u in order])
    an = vt.TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=tcs, output_dir=tmp_path / "out"))
    an.load_arrays(times, mu, mv, cols)
    an.compute_entropy()
    return g, an


@pytest.mark.parametrize("tag,tcs", [("tc200", [200]), ("tc20_50", [20, 50])])
def test_golden_counts(native, engine, tmp_path, golden_dir, tag, tcs):
    g, an = _analyzer_on_g5(tmp_path, golden_dir, tag, tcs)
    _, mu, mv, _ = an._dense
    assert not np.isnan(mu).any()                                      # G5: every user in every frame
    src = g[f"{tag}__srccount"]
    present = np.full(len(src), mu.shape[1], dtype=np.int32)
    VWa, VHa = an.config.video_width, an.config.video_height
    hm = native.Heatmap(engine, vo.fibonacci_lattice(tcs[0]), 240, 120, VWa, VHa)
    got = an.render_heatmaps(width=240, height=120)
    assert got.shape == (299, 120, 240, 3)
    assert np.array_equal(got, ho.render(hm.map(), src, present, mu[:-1], mv[:-1], VWa, VHa, 2))
    big = native.Heatmap(engine, vo.fibonacci_lattice(tcs[0]), 1200, 600, VWa, VHa)
    for r in (0, 150, 298):
        want = ho.render(big.map(), src[r:r + 1], present[r:r + 1], mu[r:r + 1], mv[r:r + 1], VWa, VHa, 2)
        assert np.array_equal(an.render_heatmaps(frames=range(r, r + 1)), want), f"row {r}"


# --------------------------------------------------------------------------- blocks, repeatability, device pointers
def test_blocks_and_repeat(native, engine):
    """40 rows at 1200 x 600 are three sub-blocks of the two-buffer pipeline; blocks of 7 rows give the same bytes."""
    R = 40
    mu, mv = walk(24, R + 1, seed=13)
    plan = plan_of(native, engine, [50])
    whole, counts, hm, result, present, _ = check_result(native, engine, plan, mu, mv, [50], 1200, 600)
    pmu, pmv = mu[:-1], mv[:-1]                                        # frame r's samples for row r
    parts = [hm.render_transition_result(result, present[r:r + 7], pmu[r:r + 7], pmv[r:r + 7], row0=r, n=min(7, R - r))
             for r in range(0, R, 7)]
    assert np.array_equal(np.concatenate(parts), whole)
    assert np.array_equal(hm.render_transition_result(result, present, pmu, pmv), whole)
    plan.close()


def test_render_counts_device_matches_result(native, engine):
    import torch
    T, U = 14, 16
    mu, mv = walk(U, T, seed=17)
    plan = plan_of(native, engine, [50])
    want, counts, hm, result, present, _ = check_result(native, engine, plan, mu, mv, [50], 97, 61)
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(counts).to(dev)
    p = torch.from_numpy(present).to(dev)
    dmu, dmv = torch.from_numpy(mu[:-1].copy()).to(dev), torch.from_numpy(mv[:-1].copy()).to(dev)
    rgb = torch.full((T - 1, 61, 97, 3), 7, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    hm.render_counts_device(c.data_ptr(), p.data_ptr(), T - 1, rgb.data_ptr(), dmu.data_ptr(), dmv.data_ptr(), U,
                            stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(rgb.cpu().numpy(), want)
    plain = torch.zeros_like(rgb)
    hm.render_counts_device(c.data_ptr(), p.data_ptr(), T - 1, plain.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(plain.cpu().numpy(), hm.render_transition_result(result, present))
    assert np.array_equal(plain.cpu().numpy(), ho.render(hm.map(), counts, present))
    plan.close()


# --------------------------------------------------------------------------- errors
def test_errors(native, engine):
    mu, mv = walk(8, 6, seed=2, p_absent=0.0)
    plan = plan_of(native, engine, [50])
    tr = plan.transition_resident(mu=mu, mv=mv)
    sp = plan.spatial_resident(mu=mu, mv=mv)
    present = prior_present(mu, mv)
    hm = native.Heatmap(engine, vo.fibonacci_lattice(50), 97, 61, VW, VH)
    with pytest.raises(native.NativeError) as e:                      # a spatial result
        hm.render_transition_result(sp["result"], sp["present"])
    assert e.value.code == native.VET_ERR_INVALID
    with pytest.raises(native.NativeError) as e:                      # the spatial entry still refuses transition results
        hm.render_result(tr["result"], present)
    assert e.value.code == native.VET_ERR_INVALID
    hm20 = native.Heatmap(engine, vo.fibonacci_lattice(20), 97, 61, VW, VH)
    with pytest.raises(native.NativeError) as e:                      # lattice of another size
        hm20.render_transition_result(tr["result"], present)
    assert e.value.code == native.VET_ERR_INVALID
    for row0, n in ((0, 6), (3, 3), (-1, 1)):                          # outside [0, T-1)
        with pytest.raises(native.NativeError) as e:
            hm.render_transition_result(tr["result"], np.ones(n, dtype=np.int32), row0=row0, n=n)
        assert e.value.code == native.VET_ERR_INVALID
    with pytest.raises(native.NativeError) as e:                      # samples of another audience
        hm.render_transition_result(tr["result"], present, mu[:-1, :4], mv[:-1, :4])
    assert e.value.code == native.VET_ERR_INVALID
    assert hm.render_transition_result(tr["result"], present[:0], row0=5, n=0).shape == (0, 61, 97, 3)
    plan.close()


# --------------------------------------------------------------------------- the analyzer
def test_analyzer_render_and_writers(native, tmp_path, golden_dir):
    from PIL import Image
    from viewport_entropy_toolkit.data_types import ValidationError
    g, an = _analyzer_on_g5(tmp_path, golden_dir, "tc20_50", [20, 50])
    frames = an.render_heatmaps(frames=range(20, 37), width=160, height=80)
    assert frames.shape == (17, 80, 160, 3)
    assert np.array_equal(an.render_heatmaps(frames=slice(20, 37), width=160, height=80), frames)
    whole = an.render_heatmaps(width=160, height=80, marker_radius=1)
    assert whole.shape == (299, 80, 160, 3)
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
        an.render_heatmaps(frames=range(0, 300))                       # 299 result rows
    assert an.render_heatmaps(frames=range(0, 2)).shape == (2, 600, 1200, 3)      # figure_size x dpi


def test_analyzer_absent_users_use_prior_frame_presence(native, engine, tmp_path):
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import AnalyzerConfig
    mu, mv = walk(12, 25, seed=23, p_absent=0.25)
    an = vt.TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=[50], video_width=VW, video_height=VH,
                                                     output_dir=tmp_path / "out"))
    an.load_arrays(np.arange(25, dtype=np.float64), mu, mv)
    res = an.compute_entropy()
    assert an._present is None                                         # counted on the first render, not in compute_entropy
    got = an.render_heatmaps(width=97, height=61)
    present = prior_present(mu, mv)
    assert np.array_equal(an._present, present)
    counts = an._device_result.rows(1, 0, 24)
    hm = native.Heatmap(engine, vo.fibonacci_lattice(50), 97, 61, VW, VH)
    assert np.array_equal(got, ho.render(hm.map(), counts, present, mu[:-1], mv[:-1], VW, VH, 2))
    assert len(res) == 24


def test_analyzer_vectors_render_without_markers(native, tmp_path, golden_dir):
    import viewport_entropy_toolkit as vt
    from viewport_entropy_toolkit.config import AnalyzerConfig
    g = np.load(golden_dir / "g5_transition.npz")
    d = tmp_path / "video"
    d.mkdir()
    for u in range(len(g["mu_in"])):
        pd.DataFrame({"time": g["time_in"][u], "2dmu": g["mu_in"][u], "2dmv": g["mv_in"][u], "x": 1}).to_csv(
            d / f"user{u:03d}.csv", index=False)
    an = vt.TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=[200], output_dir=tmp_path / "out"))
    an.process_directory(d)
    an.compute_entropy()
    with_markers = an.render_heatmaps(frames=range(0, 5), width=160, height=80)
    an._data_cache["vectors"] = an._data_cache["vectors"]          # hand-assigned frame table: the ids path
    an.compute_entropy()
    assert an._marker_samples is None and an._present is None
    plain = an.render_heatmaps(frames=range(0, 5), width=160, height=80)
    assert np.array_equal(plain, an.render_heatmaps(frames=range(0, 5), width=160, height=80, markers=False))
    assert np.array_equal(an._present, np.full(299, 8))
    assert not np.array_equal(plain, with_markers)
    assert (with_markers == 0).all(-1).any() and not (plain == 0).all(-1).any()
