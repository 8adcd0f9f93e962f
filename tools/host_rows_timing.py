"""Wall clock of the seven row calls' host entries through their Plan wrappers (each call ends in a stream synchronise), this
checkout against another one: A B A B, one fresh process per run, A = the other checkout (its library and its Python layer),
B = this one.  Shapes: `small`, the 9 x 150 video, [50], window 20, stride 7 at which tools/user_divergence_timing.py and
tools/crowd_divergence_timing.py call the host entries (the call is all overhead there: what the layers above the kernels can
change), and `config2`, 64 x 3 000, [50, 100, 200], window 20, stride 5.  Per series the median and the minimum of REPS calls
after WARMUP; the margin of a series is the spread between A's own two runs.
usage: python tools/host_rows_timing.py OTHER_CHECKOUT OUT.json"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VW, VH = 100, 200
WARMUP = 3
# (name, users, frames, tile counts, window, stride, max_lag of the window divergence, repetitions)
SHAPES = [("small", 9, 150, [50], 20, 7, 8, 40), ("config2", 64, 3000, [50, 100, 200], 20, 5, 32, 12)]
CALLS = [("spatial_windowed", dict(want_weights=True)), ("spatial_per_user", dict(want_weights=True)),
         ("spatial_user_divergence", {}), ("spatial_crowd_divergence", {}), ("spatial_window_divergence", None),
         ("transition_windowed", dict(want_srccount=True, check=False)), ("transition_per_user", dict(want_srccount=True))]


def child(tree):
    sys.path.insert(0, os.path.join(tree, "viewport-entropy-toolkit_amd"))
    import numpy as np
    from viewport_entropy_toolkit import _native, _quantiser, _synthetic
    eng = _native.Engine.default()
    out = {}
    for name, U, T, tcs, window, stride, lag, reps in SHAPES:
        mu, mv = _synthetic.random_walk_video(U, T, base_seed=7, p_absent=0.1)
        plan = _native.Plan(eng, [_quantiser.lattice_xyz(t) for t in tcs], 120.0, 2.0, True, VW, VH)
        for method, kw in CALLS:
            kw = dict(max_lag=lag) if kw is None else kw
            fn = getattr(plan, method)
            times = []
            for i in range(WARMUP + reps):
                t0 = time.perf_counter()
                fn(mu=mu, mv=mv, window=window, stride=stride, **kw)
                times.append((time.perf_counter() - t0) * 1e3)
            times = times[WARMUP:]
            out[f"{name} {method}"] = {"median_ms": round(float(np.median(times)), 4), "min_ms": round(min(times), 4)}
        plan.close()
    print(json.dumps(out), flush=True)


def main(other, out_path):
    runs = []
    for label, tree in (("A", other), ("B", ROOT)) * 2:
        env = dict(os.environ, VET_HIP_LIBRARY=os.path.join(tree, "viewport-entropy-toolkit_amd", "lib", "libvet_hip.so"))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], env=env, stdout=subprocess.PIPE, text=True)
        if p.returncode:
            sys.exit(f"run {label} ({tree}) failed with status {p.returncode}")
        runs.append((label, json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])))
    series = {}
    for key in runs[0][1]:
        a = [r[key]["median_ms"] for label, r in runs if label == "A"]
        b = [r[key]["median_ms"] for label, r in runs if label == "B"]
        series[key] = {"A_median_ms": a, "B_median_ms": b, "A_min_ms": [r[key]["min_ms"] for label, r in runs if label == "A"],
                       "B_min_ms": [r[key]["min_ms"] for label, r in runs if label == "B"],
                       "A_spread_percent": round(100 * (max(a) - min(a)) / min(a), 2),
                       "B_over_A_percent": round(100 * (sum(b) / sum(a) - 1), 2),
                       "both_B_slower_than_both_A_by_more_than_the_spread": bool(min(b) > max(a) + (max(a) - min(a)))}
        print(key, json.dumps(series[key]), flush=True)
    with open(out_path, "w") as f:
        json.dump({"order": "A B A B, one process each; A = the other checkout, B = this one", "warmup": WARMUP,
                   "shapes": [dict(zip(("name", "users", "frames", "tile_counts", "window", "stride", "max_lag", "reps"), s)) for s in SHAPES],
                   "clock": "time.perf_counter around the Plan wrapper call", "series": series}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    elif len(sys.argv) == 3:
        main(os.path.abspath(sys.argv[1]), sys.argv[2])
    else:
        sys.exit(__doc__)
