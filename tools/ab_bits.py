"""Bit-for-bit A / B of two builds of libvet_hip.so over the row calls (per-viewer entropy and transitions, the windowed calls,
the three divergence calls): what a refactor of vet_user*.hip, vet_window*.hip, vet_crowd.hip or vet_hostapi.hip must keep.
Each library is loaded through VET_HIP_LIBRARY in a fresh child process; both run the same seeded cases; every output array is
compared as bytes (its SHA-256), nothing by tolerance.  A call that fails is a result too: its code and message are compared.
Inputs: _synthetic.random_walk_video(65, 150, base_seed=7, p_absent=0.1) with viewer 3 absent over frames 40..75 — 65 viewers
cross the 64-user transpose tile and the 32-viewer pair block; windows 20, 100 and 150 run 1, 2 and 4 waves per (viewer, row)
workgroup; strides 7 and 1.  Plans: weighted [50], [50, 100, 200] and [1000], unweighted [50], the naive analyzer's lat/lon
plan.  Calls: the host entries with (mu, mv) and with ids, the device entries with (mu, mv) and with ids; per-viewer and windowed
spatial entropy with weights, viewer divergence, crowd divergence with its row series, window divergence at max_lag 1, 8 and
R - 1, the two transition row calls; the divergence calls also at forced chunks of 1 and 7 rows.
Then what the layers above the kernels must keep, on the weighted [50] plan.  The refusals of the seven host entries and of their
device entries, called through ctypes: window 0, window one more than the frames (pairs), stride 0, max_lag 0 and R, a null
primary output, neither ids nor (mu, mv), the windowed transition's 2^19 refusal (U = 2048, T = 258, window = 256) and the
per-viewer transition's own refusal together with missing samples (which one wins); ids with a null h_mu is accepted and its
outputs are compared.  The Plan wrappers: their ValueErrors, the optional output not wanted, the *_device wrappers (with d_ids
where they take it).  The analyzers' twelve row methods on a 12 x 3 video: their frames, a sample of 1.5, a window without a
sample.
The saliency family is what a refactor of vet_saliency.hip must keep: the eight device entries (vet_saliency, _similarity, _score,
vet_congruency, each with (mu, mv) and with ids) on the same video and the 100 x 200 grid plan.  Maps of 37 x 19 (703 pixels: one
partial block of the summation rule, a partial last workgroup) and 64 x 33 (2 112: three blocks, the last partial), sigma 5 and 1
degrees; windows 1, 20 and 150 at stride 7 and window 20 at stride 1 (65 and 1 300 positions: the LDS sort, the latter at 2 048 keys
with lists beyond one LDS tile and one rule block; 9 750: counted, in LDS).  vet_saliency pooled and per viewer, scales 0 to 2, each
optional output present and absent, vet_test_saliency_tile 0, 4 and 1; the similarity with viewer u in audience A, B or neither by
u mod 3, with and without d_maps, tile 0 and 4; the congruency with and without NSS and d_rows, tile 0 and 4; the scoring of a seeded
noise map, static and one per row, with and without the distribution metrics and d_map.  One vet_saliency_ids case on a 300 x 200
grid plan (60 501 directions, past the LDS counts) with rows of 4 550 positions.  The refusals: window 0 and T + 1, stride 0, sigma
0, W 1 and 4 097, H 2 049, scale 3, groups NULL, an audience without a viewer, pred NULL, n_pred 2, one viewer for the congruency.
One line per case; exit status 1 on any difference.  A refusal's line holds the exception's type name or the code before the
message, so the lines of profiles/refactor/row_calls_ab_bits.txt (message only) do not compare with today's.
usage: python tools/ab_bits.py libA.so libB.so [rows|saliency|all]      (the family; default all)
       python tools/ab_bits.py --dump LIB [family]   the case lines of one library with the Python layer of this checkout, to diff
                                               against the same from another checkout"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'viewport-entropy-toolkit_amd'))

VW, VH = 100, 200
U, T = 65, 150
WINDOWS, STRIDES = (20, 100, 150), (7, 1)
FAMILIES = ("rows", "saliency", "all")
CHUNKS = (0, 1, 7)                              # forced rows per chunk of the divergence calls (0: sized by the budget)


def child(family):
    import numpy as np
    import torch
    from viewport_entropy_toolkit import NaiveSpatialEntropyAnalyzer, _native, _quantiser, _synthetic
    from viewport_entropy_toolkit.config import EntropyConfig, NaiveAnalyzerConfig

    eng = _native.Engine.default()
    lib = eng.lib
    dev = torch.device('cuda', 0)
    mu, mv = _synthetic.random_walk_video(U, T, base_seed=7, p_absent=0.1)
    mu[40:76, 3] = np.nan; mv[40:76, 3] = np.nan
    absent = np.isnan(mu) | np.isnan(mv)
    px, py = (np.nan_to_num(mu) * VW).astype(np.int64), (np.nan_to_num(mv) * VH).astype(np.int64)
    ids = np.where(absent, -1, py * (VW + 1) + px).astype(np.int32)
    d_mu, d_mv, d_ids = (torch.from_numpy(a).to(dev) for a in (mu, mv, ids))
    status = torch.zeros(2, dtype=torch.int32, device=dev)

    def emit(case, outputs):
        print(json.dumps({"case": case, "outputs": outputs}), flush=True)

    def digest(a):
        return None if a is None else hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

    def host(case, fn, **kw):
        for src, samples in (("mu_mv", dict(mu=mu, mv=mv)), ("ids", dict(ids=ids))):
            try:
                out = fn(**samples, **kw)
                res = {k: (int(v) if k == "code" else digest(v)) for k, v in out.items()}
            except (_native.NativeError, ValueError) as e:
                res = {"error": f"{type(e).__name__}: {e}"}
            emit(f"{case} host {src}", res)

    def device(case, entry, window, stride, extra, shapes):
        """entry(_ids): the C-ABI symbol; extra: ints between stride and the outputs; shapes: (name, shape, dtype) of the outputs"""
        for src in ("mu_mv", "ids"):
            outs = [torch.full(shape, -7, dtype=dtype, device=dev) for _, shape, dtype in shapes]
            status.zero_()
            torch.cuda.synchronize()
            ptrs = [o.data_ptr() for o in outs]
            if src == "ids":
                rc = getattr(lib, entry + "_ids")(plan.handle, d_ids.data_ptr(), U, T, window, stride, *extra, *ptrs,
                                                  status.data_ptr(), None)
            else:
                rc = getattr(lib, entry)(plan.handle, d_mu.data_ptr(), d_mv.data_ptr(), U, T, window, stride, *extra, *ptrs,
                                         status.data_ptr(), None)
            eng.synchronize()
            if rc:
                res = {"error": f"{rc}: {(lib.vet_last_error() or b'').decode()}"}
            else:
                res = {name: digest(o.cpu().numpy()) for (name, _, _), o in zip(shapes, outs)}
                res["status"] = digest(status.cpu().numpy())
            emit(f"{case} device {src}", res)


    # the seven row calls: (name, C symbol stem, Plan method, windows of frame pairs, max_lag argument, outputs (key, dims, dtype)
    # in the entries' order; dims: U users, R rows, n tiles, L max_lag)
    ROW_CALLS = [
        ("windowed", "vet_spatial_entropy_windowed", "spatial_windowed", False, False,
         [("entropy", "R", "f8"), ("weights", "Rn", "f8"), ("samples", "R", "i4")]),
        ("user_entropy", "vet_user_entropy", "spatial_per_user", False, False,
         [("entropy", "UR", "f8"), ("weights", "URn", "f8"), ("samples", "UR", "i4")]),
        ("user_divergence", "vet_user_divergence", "spatial_user_divergence", False, False,
         [("divergence", "RUU", "f8"), ("samples", "UR", "i4")]),
        ("crowd_divergence", "vet_crowd_divergence", "spatial_crowd_divergence", False, False,
         [("divergence", "UR", "f8"), ("rows", "3R", "f8"), ("samples", "UR", "i4")]),
        ("window_divergence", "vet_window_divergence", "spatial_window_divergence", False, True,
         [("divergence", "RL", "f8"), ("samples", "R", "i4")]),
        ("windowed_transition", "vet_transition_entropy_windowed", "transition_windowed", True, False,
         [("entropy", "R", "f8"), ("srccount", "Rn", "i4"), ("samples", "R", "i4")]),
        ("user_transition", "vet_user_transition_entropy", "transition_per_user", True, False,
         [("entropy", "UR", "f8"), ("srccount", "URn", "i4"), ("samples", "UR", "i4")]),
    ]

    def layers(plan):
        """The refusals of the C entries, the Plan wrappers and the analyzers (module docstring); plan: weighted [50]."""
        n0 = plan.n_tiles[0]
        big_u, big_t = 2048, 258                                 # window 256 of 257 pairs: window * U = 2^19
        half = np.full((big_t, big_u), 0.5)
        d_half = torch.from_numpy(half).to(dev)
        d_big_ids = torch.zeros((big_t, big_u), dtype=torch.int32, device=dev)

        def shape(dims, u, r, lag):                              # lag: the call's max_lag argument(s); a refused 0 still gets a buffer
            return tuple({"U": u, "R": r, "n": n0, "L": max(lag[0], 1) if lag else 0, "3": 3}[d] for d in dims)

        def raw_host(case, stem, outs, u, t, window, stride, lag, h_mu, h_mv, h_ids, r, no_primary=False):
            bufs = [np.full(shape(dims, u, r, lag), -7, dtype=dt) for _, dims, dt in outs]
            ptrs = [_native._ptr(b) for b in bufs]
            if no_primary:
                ptrs[0] = None
            rc = getattr(lib, stem + "_host")(plan.handle, _native._ptr(h_mu), _native._ptr(h_mv), _native._ptr(h_ids), u, t,
                                              window, stride, *lag, *ptrs)
            if rc:
                emit(case, {"error": f"{rc}: {(lib.vet_last_error() or b'').decode()}"})
            else:
                emit(case, {key: digest(b) for (key, _, _), b in zip(outs, bufs)})

        def raw_device(case, stem, outs, u, t, window, stride, lag, samples, r, no_primary=False):
            tdt = {"f8": torch.float64, "i4": torch.int32}
            bufs = [torch.full(shape(dims, u, r, lag), -7, dtype=tdt[dt], device=dev) for _, dims, dt in outs]
            ptrs = [b.data_ptr() for b in bufs]
            if no_primary:
                ptrs[0] = None
            status.zero_()
            torch.cuda.synchronize()
            entry = getattr(lib, stem + ("_ids" if len(samples) == 1 else ""))
            rc = entry(plan.handle, *samples, u, t, window, stride, *lag, *ptrs, status.data_ptr(), None)
            eng.synchronize()
            emit(case, {"error": f"{rc}: {(lib.vet_last_error() or b'').decode()}"} if rc else {"accepted": True})

        for name, stem, method, pairs, has_lag, outs in ROW_CALLS:
            n = T - 1 if pairs else T
            r = (n - 20) // 7 + 1
            lag = (2,) if has_lag else ()
            refusals = [("window0", 0, 7, lag), ("window_long", n + 1, 7, lag), ("stride0", 20, 0, lag)]
            if has_lag:
                refusals += [("lag0", 20, 7, (0,)), ("lagR", 20, 7, (r,))]
            for what, window, stride, lg in refusals:
                raw_host(f"refusal {name} {what} host", stem, outs, U, T, window, stride, lg, mu, mv, None, r)
                raw_device(f"refusal {name} {what} device", stem, outs, U, T, window, stride, lg, (d_mu.data_ptr(), d_mv.data_ptr()), r)
                raw_device(f"refusal {name} {what} device ids", stem, outs, U, T, window, stride, lg, (d_ids.data_ptr(),), r)
            raw_host(f"refusal {name} no_output host", stem, outs, U, T, 20, 7, lag, mu, mv, None, r, no_primary=True)
            raw_device(f"refusal {name} no_output device", stem, outs, U, T, 20, 7, lag, (d_mu.data_ptr(), d_mv.data_ptr()), r,
                       no_primary=True)
            raw_host(f"refusal {name} no_samples host", stem, outs, U, T, 20, 7, lag, None, None, None, r)
            raw_host(f"refusal {name} no_samples bad_window host", stem, outs, U, T, 0, 7, lag, None, None, None, r)
            raw_device(f"refusal {name} no_samples device", stem, outs, U, T, 20, 7, lag, (None, None), r)
            raw_device(f"refusal {name} no_samples device ids", stem, outs, U, T, 20, 7, lag, (None,), r)
            raw_host(f"accepted {name} ids_null_mu host", stem, outs, U, T, 20, 7, lag, None, None, ids, r)
            if name == "windowed_transition":
                raw_host(f"refusal {name} 2^19 host", stem, outs, big_u, big_t, 256, 1, (), half, half, None, 2)
                raw_device(f"refusal {name} 2^19 device", stem, outs, big_u, big_t, 256, 1, (), (d_half.data_ptr(), d_half.data_ptr()), 2)
                raw_device(f"refusal {name} 2^19 device ids", stem, outs, big_u, big_t, 256, 1, (), (d_big_ids.data_ptr(),), 2)

            # the Plan wrappers: ValueErrors, the optional output not wanted, the *_device wrapper
            fn = getattr(plan, method)
            kw = dict(max_lag=2) if has_lag else {}
            for what, window, stride, extra in [("window_none", None, 7, kw), ("window0", 0, 7, kw), ("window_long", n + 1, 7, kw),
                                                ("stride0", 20, 0, kw), ("plain", 20, 7, kw)] + \
                                               ([("lag0", 20, 7, dict(max_lag=0)), ("lagR", 20, 7, dict(max_lag=r))] if has_lag else []):
                host(f"plan {name} {what}", fn, window=window, stride=stride, **extra)
            dev_fn = getattr(plan, method + "_device")
            bufs = [torch.full(shape(dims, U, r, lag), -7, dtype={"f8": torch.float64, "i4": torch.int32}[dt], device=dev)
                    for _, dims, dt in outs]
            for src, samples in (("mu_mv", {}), ("ids", dict(d_ids=d_ids.data_ptr()))):
                if src == "ids" and name not in ("crowd_divergence", "window_divergence"):
                    continue
                status.zero_()
                torch.cuda.synchronize()
                dev_fn(d_mu.data_ptr(), d_mv.data_ptr(), U, T, 20, 7, *lag, *(b.data_ptr() for b in bufs), d_status=status.data_ptr(),
                       **samples)
                eng.synchronize()
                res = {key: digest(b.cpu().numpy()) for (key, _, _), b in zip(outs, bufs)}
                res["status"] = digest(status.cpu().numpy())
                emit(f"plan {name} device wrapper {src}", res)

        # the analyzers on a 12 x 3 video with viewer 1 absent over frames 4..8; then a sample of 1.5; then frames 0..4 empty
        from viewport_entropy_toolkit import SpatialEntropyAnalyzer, TransitionEntropyAnalyzer
        from viewport_entropy_toolkit.config import AnalyzerConfig
        a_mu, a_mv = _synthetic.random_walk_video(3, 12, base_seed=7, p_absent=0.1)
        a_mu[4:9, 1] = np.nan; a_mv[4:9, 1] = np.nan
        cfg = dict(video_width=VW, video_height=VH, entropy_config=EntropyConfig(use_weight_distribution=True),
                   output_dir=os.path.join(tempfile.gettempdir(), "ab_bits"))
        makers = [("spatial", lambda: SpatialEntropyAnalyzer(AnalyzerConfig(tile_counts=[50], **cfg))),
                  ("naive", lambda: NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20, **cfg))),
                  ("transition", lambda: TransitionEntropyAnalyzer(AnalyzerConfig(tile_counts=[50], **cfg)))]
        methods = [("compute_windowed_entropy", dict(window=5, stride=2)), ("compute_user_entropy", dict(window=5, stride=2)),
                   ("compute_user_entropy", {}), ("compute_user_divergence", dict(window=5, stride=2)),
                   ("compute_window_divergence", dict(window=5, stride=2, max_lag=2)),
                   ("compute_crowd_divergence", dict(window=5, stride=2)), ("compute_windowed_entropy", dict(window=13))]

        def frame(df):
            out = {}
            for col in df.columns:
                if col != "tile_weights":
                    v = df[col].to_numpy()
                    out[col] = digest(np.stack(v)) if v.dtype == object and not isinstance(v[0], str) else \
                        hashlib.sha256(repr(v.tolist()).encode()).hexdigest() if v.dtype == object else digest(v)
            return out

        for aname, make in makers:
            for variant in ("plain", "out_of_range", "empty_window"):
                x_mu, x_mv = a_mu.copy(), a_mv.copy()
                if variant == "empty_window":
                    x_mu[0:5] = np.nan; x_mv[0:5] = np.nan
                an = make()
                an.load_arrays(np.arange(12) * 0.1, x_mu, x_mv)
                if variant == "out_of_range":                    # past load_arrays' own check: the engine's refusal
                    an._dense[1][2, 0], an._dense[2][2, 0] = 1.5, 0.5
                for method, kw in methods:
                    if hasattr(an, method):
                        try:
                            res = frame(getattr(an, method)(**kw))
                        except Exception as e:  # noqa: BLE001
                            res = {"error": f"{type(e).__name__}: {e}"}
                        emit(f"analyzer {aname} {variant} {method} {sorted(kw.items())}", res)

    f64, i32 = torch.float64, torch.int32
    lattice = lambda tcs: [_quantiser.lattice_xyz(tc) for tc in tcs]
    naive = NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=VW, video_height=VH,
                                                            entropy_config=EntropyConfig(use_weight_distribution=True)))
    plans = [("w_50", lambda: _native.Plan(eng, lattice([50]), 120.0, 2.0, True, VW, VH)),
             ("w_50_100_200", lambda: _native.Plan(eng, lattice([50, 100, 200]), 120.0, 2.0, True, VW, VH)),
             ("w_1000", lambda: _native.Plan(eng, lattice([1000]), 120.0, 2.0, True, VW, VH)),
             ("u_50", lambda: _native.Plan(eng, lattice([50]), 120.0, 2.0, False, VW, VH)),
             ("naive_10x20", naive._naive_plan)]
    for pname, make in plans if family != "saliency" else []:
        plan = make()
        n0 = plan.n_tiles[0]
        for window in WINDOWS:
            for stride in STRIDES:
                tag = f"{pname} w{window} s{stride}"
                R = (T - window) // stride + 1
                host(f"{tag} user_entropy", plan.spatial_per_user, window=window, stride=stride, want_weights=True)
                device(f"{tag} user_entropy", "vet_user_entropy", window, stride, (),
                       [("entropy", (U, R), f64), ("weights", (U, R, n0), f64), ("samples", (U, R), i32)])
                host(f"{tag} windowed", plan.spatial_windowed, window=window, stride=stride, want_weights=True)
                device(f"{tag} windowed", "vet_spatial_entropy_windowed", window, stride, (),
                       [("entropy", (R,), f64), ("weights", (R, n0), f64), ("samples", (R,), i32)])
                for chunk in CHUNKS:
                    ctag = f"{tag} chunk{chunk}"
                    eng.test_divergence_chunk_rows(chunk)
                    eng.test_crowd_divergence_chunk_rows(chunk)
                    eng.test_window_divergence_chunk_rows(chunk)
                    host(f"{ctag} user_divergence", plan.spatial_user_divergence, window=window, stride=stride)
                    device(f"{ctag} user_divergence", "vet_user_divergence", window, stride, (),
                           [("divergence", (R, U, U), f64), ("samples", (U, R), i32)])
                    host(f"{ctag} crowd_divergence", plan.spatial_crowd_divergence, window=window, stride=stride)
                    device(f"{ctag} crowd_divergence", "vet_crowd_divergence", window, stride, (),
                           [("divergence", (U, R), f64), ("rows", (3, R), f64), ("samples", (U, R), i32)])
                    for lag in sorted({l for l in (1, 8, R - 1) if 1 <= l <= R - 1}):
                        host(f"{ctag} window_divergence lag{lag}", plan.spatial_window_divergence, window=window, stride=stride,
                             max_lag=lag)
                        device(f"{ctag} window_divergence lag{lag}", "vet_window_divergence", window, stride, (lag,),
                               [("divergence", (R, lag), f64), ("samples", (R,), i32)])
                eng.test_divergence_chunk_rows(0)
                eng.test_crowd_divergence_chunk_rows(0)
                eng.test_window_divergence_chunk_rows(0)
                pw = min(window, T - 1)                         # transitions: windows of frame pairs
                Rp = (T - 1 - pw) // stride + 1
                ptag = f"{pname} w{pw} s{stride}"
                host(f"{ptag} user_transition", plan.transition_per_user, window=pw, stride=stride, want_srccount=True)
                device(f"{ptag} user_transition", "vet_user_transition_entropy", pw, stride, (),
                       [("entropy", (U, Rp), f64), ("srccount", (U, Rp, n0), i32), ("samples", (U, Rp), i32)])
                host(f"{ptag} windowed_transition", plan.transition_windowed, window=pw, stride=stride, want_srccount=True,
                     check=False)
                device(f"{ptag} windowed_transition", "vet_transition_entropy_windowed", pw, stride, (),
                       [("entropy", (Rp,), f64), ("srccount", (Rp, n0), i32), ("samples", (Rp,), i32)])
        if pname == "w_50":
            layers(plan)
        if pname != "naive_10x20":
            plan.close()

    def saliency_family():
        """The eight device entries of vet_saliency.hip (module docstring), called through ctypes on the 100 x 200 grid plan."""
        plan = _native.Plan(eng, lattice([50]), 120.0, 2.0, True, VW, VH)
        rad = lambda deg: deg * (np.pi / 180.0)
        groups = (np.arange(U) % 3).astype(np.int8)
        groups[groups == 2] = -1
        SHAPES = ((37, 19), (64, 33))                           # 703 pixels: one partial rule block; 2 112: three, the last partial
        SIGMAS = (5.0, 1.0)
        WS = ((1, 7), (20, 7), (150, 7), (20, 1))               # 65 and 1 300 positions: sorted; 9 750: counted in LDS
        corners = ((SHAPES[0], SIGMAS[0]), (SHAPES[1], SIGMAS[1]))

        def call(case, stem, args, shapes, samples=None, u=U, hold=()):
            """args: what follows (U, T) up to the outputs; shapes: (name, shape or None = not wanted, dtype) in the entry's order;
            hold: arrays the arguments point to"""
            for src, ptrs in (("mu_mv", (d_mu.data_ptr(), d_mv.data_ptr())), ("ids", (d_ids.data_ptr(),))) if samples is None else samples:
                outs = [None if shape is None else torch.full(shape, -7, dtype=dtype, device=dev) for _, shape, dtype in shapes]
                status.zero_()
                torch.cuda.synchronize()
                rc = getattr(lib, stem + ("_ids" if len(ptrs) == 1 else ""))(
                    plan.handle, *ptrs, u, T, *args, *(None if o is None else o.data_ptr() for o in outs), status.data_ptr(), None)
                eng.synchronize()
                if rc:
                    res = {"error": f"{rc}: {(lib.vet_last_error() or b'').decode()}"}
                else:
                    res = {name: digest(o.cpu().numpy()) for (name, _, _), o in zip(shapes, outs) if o is not None}
                    res["status"] = digest(status.cpu().numpy())
                emit(f"{case} device {src}", res)

        i64 = torch.int64
        for window, stride in WS:
            R = (T - window) // stride + 1
            for (W, H), sigma in [(wh, sg) for wh in SHAPES for sg in SIGMAS]:
                tag = f"w{window} s{stride} {W}x{H} sigma{sigma:g}"
                corner = ((W, H), sigma) in corners
                # vet_saliency: the base case everywhere; scales, absent outputs and tiles at the two corners
                variants = [(2, "mspc", 0)]
                if corner:
                    variants += [(0, "mspc", 0), (1, "mspc", 0), (2, "mspc", 4), (2, "mspc", 1)]
                if corner and sigma == SIGMAS[0]:
                    variants += [(2, "spc", 0), (2, "mc", 0), (2, "msp", 0), (2, "c", 0)]
                for per_user in (0, 1):
                    rows = R * U if per_user else R
                    for scale, want, tile in variants:
                        eng.test_saliency_tile(tile)
                        call(f"saliency {tag} {'viewer' if per_user else 'pooled'} scale{scale} outs={want} tile{tile}", "vet_saliency",
                             (window, stride, per_user, rad(sigma), W, H, scale),
                             [("map", (rows, H, W) if "m" in want else None, f64), ("stats", (4, rows) if "s" in want else None, f64),
                              ("peak", (rows,) if "p" in want else None, i32), ("counts", (2, rows) if "c" in want else None, i64)])
                for tile in (0, 4):
                    eng.test_saliency_tile(tile)
                    for maps in (True, False):
                        call(f"similarity {tag} maps={int(maps)} tile{tile}", "vet_saliency_similarity",
                             (window, stride, groups.ctypes.data, rad(sigma), W, H),
                             [("maps", (2, R, H, W) if maps else None, f64), ("stats", (9, R), f64), ("counts", (4, R), i64)], hold=(groups,))
                eng.test_saliency_tile(0)
                noise = torch.from_numpy(np.random.default_rng(11).random((R, H, W))).to(dev)
                for n_pred in sorted({1, R}):
                    for dist in (0, 1):
                        for own in (True, False):
                            call(f"score {tag} n_pred={'1' if n_pred == 1 else 'R'} dist{dist} map={int(own)}", "vet_saliency_score",
                                 (window, stride, rad(sigma), W, H, noise.data_ptr(), n_pred, dist),
                                 [("map", (R, H, W) if own else None, f64), ("stats", (9, R), f64), ("counts", (2, R), i64)], hold=(noise,))
            for sigma in SIGMAS:
                for tile in (0, 4):
                    eng.test_saliency_tile(tile)
                    for nss in (0, 1):
                        for rows in (True, False):
                            call(f"congruency w{window} s{stride} sigma{sigma:g} nss{nss} rows={int(rows)} tile{tile}", "vet_congruency",
                                 (window, stride, rad(sigma), nss),
                                 [("stats", (3, U, R), f64), ("counts", (3, U, R), i64), ("rows", (4, R) if rows else None, f64)])
                eng.test_saliency_tile(0)

        # the refusals: every output NULL, so a call that is not refused writes nothing
        none = lambda names: [(n, None, f64) for n in names]
        pred = torch.zeros((19, 37), dtype=f64, device=dev)
        sal = lambda window=20, stride=7, sigma=rad(5.0), W=37, H=19, scale=2: (window, stride, 0, sigma, W, H, scale)
        sim = lambda g=groups, window=20, stride=7, sigma=rad(5.0), W=37, H=19: (window, stride, None if g is None else g.ctypes.data,
                                                                                   sigma, W, H)
        sco = lambda p=pred, n_pred=1, window=20, stride=7, sigma=rad(5.0), W=37, H=19: (window, stride, sigma, W, H,
                                                                                       None if p is None else p.data_ptr(), n_pred, 1)
        only_a = np.zeros(U, dtype=np.int8)
        common = [("window0", dict(window=0)), ("window_long", dict(window=T + 1)), ("stride0", dict(stride=0)), ("sigma0", dict(sigma=0.0))]
        mapped = common + [("W1", dict(W=1)), ("W4097", dict(W=4097)), ("H2049", dict(H=2049))]
        for what, kw in mapped + [("scale3", dict(scale=3))]:
            call(f"refusal saliency {what}", "vet_saliency", sal(**kw), none(("map", "stats", "peak", "counts")))
        for what, kw in mapped + [("groups_null", dict(g=None)), ("empty_audience", dict(g=only_a))]:
            call(f"refusal similarity {what}", "vet_saliency_similarity", sim(**kw), none(("maps", "stats", "counts")), hold=(only_a,))
        for what, kw in mapped + [("pred_null", dict(p=None)), ("n_pred2", dict(n_pred=2))]:
            call(f"refusal score {what}", "vet_saliency_score", sco(**kw), none(("map", "stats", "counts")))
        for what, kw in common:
            a = dict(window=20, stride=7, sigma=rad(5.0)); a.update(kw)
            call(f"refusal congruency {what}", "vet_congruency", (a["window"], a["stride"], a["sigma"], 1), none(("stats", "counts", "rows")))
        call("refusal congruency U1", "vet_congruency", (20, 7, rad(5.0), 1), none(("stats", "counts", "rows")), u=1)
        plan.close()

        # a direction table beyond the LDS counts: a 300 x 200 pixel grid (60 501 directions), rows of 70 frames (4 550 positions)
        plan = _native.Plan(eng, lattice([50]), 120.0, 2.0, True, 300, 200)
        big_ids = np.where(absent, -1, (np.nan_to_num(mv) * 200).astype(np.int64) * 301 + (np.nan_to_num(mu) * 300).astype(np.int64))
        d_big = torch.from_numpy(big_ids.astype(np.int32)).to(dev)
        R = (T - 70) // 40 + 1
        call("saliency big_table w70 s40 12x6 sigma10", "vet_saliency", (70, 40, 0, rad(10.0), 12, 6, 2),
             [("map", (R, 6, 12), f64), ("stats", (4, R), f64), ("peak", (R,), i32), ("counts", (2, R), i64)],
             samples=(("ids", (d_big.data_ptr(),)),), hold=(d_big,))
        plan.close()

    if family != "rows":
        saliency_family()


def run_child(lib, family):
    env = dict(os.environ, VET_HIP_LIBRARY=os.path.abspath(lib))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", family], env=env, stdout=subprocess.PIPE, text=True)
    cases = {}
    for line in p.stdout.splitlines():
        if line.startswith("{"):
            rec = json.loads(line)
            cases[rec["case"]] = rec["outputs"]
    return p.returncode, cases


def main(lib_a, lib_b, family):
    rc_a, a = run_child(lib_a, family)
    if rc_a:                                                     # nothing more is started on a GPU that a run may have faulted
        sys.exit(f"the run of A ({lib_a}) ended with status {rc_a} after {len(a)} cases; B was not run")
    rc_b, b = run_child(lib_b, family)
    bad = 0
    for case in sorted(set(a) | set(b), key=lambda c: (list(a).index(c) if c in a else len(a), c)):
        same = case in a and case in b and a[case] == b[case]
        differing = sorted(k for k in set(a.get(case, {})) | set(b.get(case, {})) if a.get(case, {}).get(k) != b.get(case, {}).get(k))
        refused = " (refused: " + a[case]["error"] + ")" if same and "error" in a[case] else ""
        print(f"{'same' if same else 'DIFF'}  {case}{refused}{'' if same else '  ' + ', '.join(differing)}")
        bad += not same
    print(f"{len(a)} cases from A ({lib_a}, exit {rc_a}), {len(b)} from B ({lib_b}, exit {rc_b}); {bad} differ")
    return 1 if bad or rc_a or rc_b or not a else 0


def dump(lib, family):
    rc, cases = run_child(lib, family)
    for case, outputs in cases.items():
        print(f"{case}  {json.dumps(outputs, sort_keys=True)}")
    print(f"{len(cases)} cases (exit {rc})")
    return 1 if rc or not cases else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    family = args.pop() if args and args[-1] in FAMILIES else "all"
    if args == ["--child"]:
        child(family)
    elif len(args) == 2 and args[0] == "--dump":
        sys.exit(dump(args[1], family))
    elif len(args) == 2:
        sys.exit(main(args[0], args[1], family))
    else:
        sys.exit(__doc__)
