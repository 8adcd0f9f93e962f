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
One line per case; exit status 1 on any difference.
usage: python tools/ab_bits.py libA.so libB.so"""
import hashlib
import json
import os
import subprocess
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'viewport-entropy-toolkit_amd'))

VW, VH = 100, 200
U, T = 65, 150
WINDOWS, STRIDES = (20, 100, 150), (7, 1)
CHUNKS = (0, 1, 7)                              # forced rows per chunk of the divergence calls (0: sized by the budget)


def child():
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
            except _native.NativeError as e:
                res = {"error": str(e)}
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

    f64, i32 = torch.float64, torch.int32
    lattice = lambda tcs: [_quantiser.lattice_xyz(tc) for tc in tcs]
    naive = NaiveSpatialEntropyAnalyzer(NaiveAnalyzerConfig(tile_height=10, tile_width=20, video_width=VW, video_height=VH,
                                                            entropy_config=EntropyConfig(use_weight_distribution=True)))
    plans = [("w_50", lambda: _native.Plan(eng, lattice([50]), 120.0, 2.0, True, VW, VH)),
             ("w_50_100_200", lambda: _native.Plan(eng, lattice([50, 100, 200]), 120.0, 2.0, True, VW, VH)),
             ("w_1000", lambda: _native.Plan(eng, lattice([1000]), 120.0, 2.0, True, VW, VH)),
             ("u_50", lambda: _native.Plan(eng, lattice([50]), 120.0, 2.0, False, VW, VH)),
             ("naive_10x20", naive._naive_plan)]
    for pname, make in plans:
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
        if pname != "naive_10x20":
            plan.close()


def run_child(lib):
    env = dict(os.environ, VET_HIP_LIBRARY=os.path.abspath(lib))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE, text=True)
    cases = {}
    for line in p.stdout.splitlines():
        if line.startswith("{"):
            rec = json.loads(line)
            cases[rec["case"]] = rec["outputs"]
    return p.returncode, cases


def main(lib_a, lib_b):
    (rc_a, a), (rc_b, b) = run_child(lib_a), run_child(lib_b)
    bad = 0
    for case in sorted(set(a) | set(b), key=lambda c: (list(a).index(c) if c in a else len(a), c)):
        same = case in a and case in b and a[case] == b[case]
        differing = sorted(k for k in set(a.get(case, {})) | set(b.get(case, {})) if a.get(case, {}).get(k) != b.get(case, {}).get(k))
        refused = " (refused: " + a[case]["error"] + ")" if same and "error" in a[case] else ""
        print(f"{'same' if same else 'DIFF'}  {case}{refused}{'' if same else '  ' + ', '.join(differing)}")
        bad += not same
    print(f"{len(a)} cases from A ({lib_a}, exit {rc_a}), {len(b)} from B ({lib_b}, exit {rc_b}); {bad} differ")
    return 1 if bad or rc_a or rc_b or not a else 0


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        child()
    elif len(sys.argv) == 3:
        sys.exit(main(sys.argv[1], sys.argv[2]))
    else:
        sys.exit(__doc__)
