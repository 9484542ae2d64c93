"""Times ops.dtw_align (csrc/dtw.hip) on one MI355X: 256 pairs of 600 .. 1 600 frames, D = 59, unbanded and with
band = 200, and one pair of 1 977 x 2 100.

    python scripts/bench_dtw.py [--processes 5] [--reps 10] [--out FILE.json]

Every figure is the median over fresh processes of each process's median over `reps` calls (after 3 warm-up calls),
with the smallest and largest process median as the spread; a call is timed between device events around
ops.dtw_align on padded device tensors, path included.  Beside them:
  * the numpy statement of the same recurrence (tests/dtw_spec.py) on one core for four pairs of the batch,
    EXTRAPOLATED to the batch by its cell count (labelled so);
  * the dependency-chain floor: (T1 + T2 - 1) of the longest pair x the measured time of one empty step of a chain in
    one workgroup (ops.dtw_step_probe: a workgroup barrier a step, and a lane shift a step as the kernel's recurrence
    uses), and the steps the kernel's tiling really takes (tiles x (rows of a pass + columns of a block - 1)).
There is no pass / fail time.  Without a GPU the script fails (a CPU run says nothing about the device)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

D = 59


def batch_lengths(n=256, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    return rng.integers(600, 1601, size=n).tolist(), rng.integers(600, 1601, size=n).tolist()


def kernel_steps(t1, t2, W, R):
    """recurrence steps of the forward kernel for one unbanded pair: per tile, rows + columns - 1"""
    steps = 0
    for c0 in range(0, t2, W):
        for r0 in range(0, t1, R):
            steps += min(R, t1 - r0) + min(W, t2 - c0) - 1
    return steps


def child(reps):
    import numpy as np
    import torch
    from idiaptts_amd import lib, ops
    lib.require_gpu()
    t1, t2 = batch_lengths()
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((len(t1), max(t1), D), dtype=torch.float64, device="cuda", generator=gen)
    y = torch.randn((len(t2), max(t2), D), dtype=torch.float64, device="cuda", generator=gen)
    x1 = torch.randn((1, 1977, D), dtype=torch.float64, device="cuda", generator=gen)
    y1 = torch.randn((1, 2100, D), dtype=torch.float64, device="cuda", generator=gen)

    def timed(fn, n):
        for _ in range(3):
            fn()
        out = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return statistics.median(out)

    res = {
        "batch_ms": timed(lambda: ops.dtw_align(x, t1, y, t2), reps),
        "batch_band200_ms": timed(lambda: ops.dtw_align(x, t1, y, t2, band=200), reps),
        "batch_no_path_ms": timed(lambda: ops.dtw_align(x, t1, y, t2, return_path=False), reps),
        "one_pair_ms": timed(lambda: ops.dtw_align(x1, [1977], y1, [2100]), reps),
    }
    n_probe = 200000
    res["barrier_step_us"] = timed(lambda: ops.dtw_step_probe("barrier", n_probe), 5) * 1e3 / n_probe
    res["shift_step_us"] = timed(lambda: ops.dtw_step_probe("shift", n_probe), 5) * 1e3 / n_probe
    print("__DTW__" + json.dumps(res), flush=True)


def numpy_spec_seconds(t1, t2, pairs=4):
    import numpy as np
    import dtw_spec
    rng = np.random.default_rng(1)
    cells, secs = 0, 0.0
    for b in range(pairs):
        x, y = rng.standard_normal((t1[b], D)), rng.standard_normal((t2[b], D))
        t = time.perf_counter()
        dtw_spec.dtw(x, y)
        secs += time.perf_counter() - t
        cells += t1[b] * t2[b]
    return secs, cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.reps)
        return
    runs = []
    for _ in range(args.processes):                    # one process with the GPU open at a time
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)],
                             stdout=subprocess.PIPE, text=True, timeout=600)
        if res.returncode != 0:
            raise SystemExit("a measuring process failed with status {}".format(res.returncode))
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("__DTW__")][-1]
        runs.append(json.loads(line[len("__DTW__"):]))
        print("process {}: {}".format(len(runs), line[len("__DTW__"):]), flush=True)
    report = {k: {"median": statistics.median(r[k] for r in runs), "min": min(r[k] for r in runs),
                  "max": max(r[k] for r in runs)} for k in runs[0]}
    from idiaptts_amd import ops
    plan = ops.dtw_plan(1600, 1600, D)
    W, R = plan["col_block"], plan["rows_per_pass"]
    t1, t2 = batch_lengths()
    cells = sum(a * b for a, b in zip(t1, t2))
    longest = max(range(len(t1)), key=lambda b: kernel_steps(t1[b], t2[b], W, R))
    secs, spec_cells = numpy_spec_seconds(t1, t2)
    report.update({
        "processes": args.processes, "reps": args.reps, "pairs": len(t1), "cells": cells, "plan": plan,
        "numpy_one_core_4_pairs_s": secs,
        "numpy_one_core_batch_s_EXTRAPOLATED": secs * cells / spec_cells,
        "chain_steps_longest_pair": t1[longest] + t2[longest] - 1,
        "kernel_steps_longest_pair": kernel_steps(t1[longest], t2[longest], W, R),
        "chain_steps_one_pair": 1977 + 2100 - 1,
        "kernel_steps_one_pair": kernel_steps(1977, 2100, W, R),
    })
    for name, steps in (("longest_pair", report["chain_steps_longest_pair"]), ("one_pair", 4076)):
        report["chain_floor_barrier_ms_" + name] = steps * report["barrier_step_us"]["median"] * 1e-3
        report["chain_floor_shift_ms_" + name] = steps * report["shift_step_us"]["median"] * 1e-3
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
