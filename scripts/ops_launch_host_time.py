"""Host time per eager call of two small fused ops, for one or several builds of the package, interleaved.

    python scripts/ops_launch_host_time.py --tree this=. --tree parent=/path/to/a/built/checkout --out result.json

At these sizes the device is idle long before the host has enqueued the next call, so the time of N back-to-back calls with
one synchronize at the end is the host's: torch's autograd.Function, the wrapper, ctypes and the launch.  Every repeat of
every tree is a fresh process (two builds of one package cannot share an interpreter), the trees taking turns.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time


def child(calls, warmup):
    import torch

    from manigaussian_amd import _lib
    from manigaussian_amd.attention import fused_attention
    from manigaussian_amd.spatial_softmax import spatial_softmax3d
    dev = torch.device("cuda:0")
    x = torch.randn(1, 4, 4, 4, 4, device=dev)
    q, k, v = (torch.randn(1, 64, 64, device=dev) for _ in range(3))
    ops = {"spatial_softmax3d": lambda: spatial_softmax3d(x), "fused_attention": lambda: fused_attention(q, k, v, 1)}
    out = {"build_id": _lib.build_id()}
    for name, op in ops.items():
        for _ in range(warmup):
            op()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            op()
        torch.cuda.synchronize()
        out[name] = (time.perf_counter() - t0) / calls * 1e6
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", action="append", default=[], help="NAME=DIR of a built checkout; repeat for several")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.calls, a.warmup)
    trees = [t.split("=", 1) for t in a.tree] or [["this", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]]
    runs = {name: {"tree": d, "build_id": None, "us_per_call": {}} for name, d in trees}
    for _ in range(a.repeats):
        for name, d in trees:
            env = dict(os.environ, PYTHONPATH=os.path.abspath(d))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--warmup", str(a.warmup)],
                               env=env, cwd=d, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"{name}: the measuring process ended with {p.returncode}\n{p.stderr[-2000:]}")
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            runs[name]["build_id"] = r.pop("build_id")
            for op, us in r.items():
                runs[name]["us_per_call"].setdefault(op, []).append(round(us, 3))
    for run in runs.values():
        run["median_us"] = {op: round(statistics.median(v), 3) for op, v in run["us_per_call"].items()}
        run["spread_us"] = {op: round(max(v) - min(v), 3) for op, v in run["us_per_call"].items()}
    result = {"calls": a.calls, "warmup": a.warmup, "repeats": a.repeats,
              "shapes": {"spatial_softmax3d": [1, 4, 4, 4, 4], "fused_attention": "B=1 H=1 Nq=Nk=64 D=64"}, "runs": runs}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
