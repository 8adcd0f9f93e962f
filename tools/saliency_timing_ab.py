"""Speed of the saliency family, another build of libvet_hip.so against this checkout's: each of tools/saliency_timing.py,
saliency_similarity_timing.py, congruency_timing.py and saliency_score_timing.py is run unchanged four times, A B A B, one fresh
process per run, A = the other library and B = this checkout's through VET_HIP_LIBRARY (the Python layer is this checkout's in both).
From every run's JSON the device call's medians (`device_call*`) and the per-kernel split (`kernels_ms`) of every shape are taken.
The margin of a series is the spread between A's own two runs, as in tools/host_rows_timing.py: B is `within` when the mean of its
two medians lies within that spread of the mean of A's, `faster` or `slower` (with the excess) otherwise.  Nothing gates; the JSON
holds the numbers.  A run that fails ends the tool: nothing more is started on the device after it.
usage: python tools/saliency_timing_ab.py OTHER_LIB OUT.json [tool[:arg...] ...]
       (default: the four tools; OUT.json is updated per tool; the args follow the tool's own output path, as in congruency_timing:2:1)"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ("saliency_timing", "saliency_similarity_timing", "congruency_timing", "saliency_score_timing")
RUN_LIMIT_S = 420


def series_of(record):
    """{series name: milliseconds} of one tool run: per shape the device call's medians and the kernels' split"""
    out = {}
    for run in record["runs"]:
        shape = " ".join(f"{k}={run[k]}" for k in ("workload", "window", "stride", "per_user", "with_maps", "predicted_maps", "distribution")
                         if k in run)
        for key, val in run.items():
            if key.startswith("device_call"):
                out[f"{shape} {key}"] = val["median_ms"]
            elif key == "kernels_ms":
                for kernel, ms in val.items():
                    if isinstance(ms, (int, float)):
                        out[f"{shape} {kernel}"] = ms
    return out


def write(result, out_path):
    """one line per series"""
    with open(out_path, "w") as f:
        f.write("{\n" + ",\n".join(
            json.dumps(k) + ": " + ("{\n" + ",\n".join(f"  {json.dumps(n)}: {json.dumps(v)}" for n, v in val.items()) + "\n }"
                                    if isinstance(val, dict) else json.dumps(val)) for k, val in result.items()) + "\n}\n")


def main(other, out_path, tools):
    mine = os.path.join(ROOT, "viewport-entropy-toolkit_amd", "lib", "libvet_hip.so")
    result = json.load(open(out_path)) if os.path.exists(out_path) else {}
    result["order"] = "A B A B, one process per run; A = the other library, B = this checkout's"
    result["margin"] = "the spread between A's own two runs"
    for tool in tools:
        tool, *args = tool.split(":")
        runs = []
        for label, lib in (("A", other), ("B", mine)) * 2:
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "run.json")
                p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool + ".py"), path, *args],
                                   env=dict(os.environ, VET_HIP_LIBRARY=os.path.abspath(lib)), timeout=RUN_LIMIT_S)
                if p.returncode:
                    sys.exit(f"{tool}: run {label} ({lib}) ended with status {p.returncode}")
                runs.append((label, series_of(json.load(open(path)))))
        series = {}
        for key in runs[0][1]:
            a = [r[key] for label, r in runs if label == "A"]
            b = [r[key] for label, r in runs if label == "B"]
            spread, diff = max(a) - min(a), sum(b) / 2 - sum(a) / 2
            verdict = "within" if abs(diff) <= spread else ("slower" if diff > 0 else "faster") + f" by {abs(diff) - spread:.4f} ms beyond the spread"
            series[key] = {"A_ms": a, "B_ms": b, "A_spread_ms": round(spread, 4), "B_minus_A_ms": round(diff, 4), "verdict": verdict}
            print(tool, key, json.dumps(series[key]), flush=True)
        result[":".join([tool, *args])] = series
        write(result, out_path)


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2], sys.argv[3:] or TOOLS)
