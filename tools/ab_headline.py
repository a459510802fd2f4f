"""Interleaved A/B of the headline on ONE box with its own yardstick: `bench.py --gpus 1` with the library of another revision
(tools/libmuse_prev.bin, through MUSE_HIP_LIB) and with the in-tree library, alternating, REPS repetitions each; then the mean and
the standard deviation of ms_per_step of both series and the difference in units of the OTHER revision's own spread.
usage: python tools/ab_headline.py [reps=6] [min_seconds=2.0] [workload ...]   (further workloads: one pair each, reported only)"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREV = os.path.join(ROOT, "tools", "libmuse_prev.bin")


def bench(lib, workload, min_seconds):
    env = dict(os.environ)
    env.pop("MUSE_HIP_LIB", None)
    if lib:
        env["MUSE_HIP_LIB"] = lib
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20", "--min-seconds", str(min_seconds),
           "--workload", workload]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=180)
    if p.returncode != 0:
        sys.exit(f"bench.py failed ({p.returncode}) with lib={lib or 'in-tree'}:\n{p.stderr[-2000:]}")
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    min_seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
    if not os.path.exists(PREV):
        sys.exit(f"{PREV} not found: copy the other revision's libmuse_hip.so there")
    series = {"prev": [], "cur": []}
    for r in range(reps):
        for name, lib in (("prev", PREV), ("cur", None)):
            d = bench(lib, "funnel_1e4", min_seconds)
            series[name].append(d["ms_per_step"])
            print(f"rep {r} {name:4s} funnel_1e4 ms_per_step {d['ms_per_step']:.5f} value {d['value']:.0f}", flush=True)
    m = {k: statistics.mean(v) for k, v in series.items()}
    s = {k: statistics.stdev(v) for k, v in series.items()}
    for k in ("prev", "cur"):
        print(f"{k:4s} mean {1e3 * m[k]:.3f} us  sd {1e3 * s[k]:.3f} us  min {1e3 * min(series[k]):.3f}  max {1e3 * max(series[k]):.3f}  n {reps}")
    diff = m["prev"] - m["cur"]
    print(f"cur is {1e3 * diff:.3f} us ({100 * diff / m['prev']:.2f} %) below prev = {diff / s['prev']:.1f} x prev's own sd")
    for w in sys.argv[3:]:
        for name, lib in (("prev", PREV), ("cur", None)):
            d = bench(lib, w, min_seconds)
            print(f"other {name:4s} {w} ms_per_step {d['ms_per_step']:.5f} value {d['value']:.0f}", flush=True)


if __name__ == "__main__":
    main()
