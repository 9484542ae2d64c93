"""Times the MLPG adjoint (csrc/mlpg_adjoint.h) on a training-sized batch: 64 utterances of 600 .. 1 600 frames (seeded
lengths), the three streams of a WORLD reader with deltas (60 + 1 + 1 dimensions in rows of 187 columns), float32.

  adjoint      (a) ops.mlpg_adjoint, one call per stream into one [N, 187] gradient -- MlpgFunction's backward -- in the
               form the library chooses (recorded per call: `adjoint_forms`), and the same under each form forced
               with ops.mlpg_adjoint_forced: `adjoint_stream`, `adjoint_sweeps`
  forward      (b) ops.mlpg_generation on the same batch in the form the library chooses -- MlpgFunction's forward
  composition  (c) the same gradient without a new kernel: ops.mlpg_generation on rows (g * var_0, 0, 0), whose
               right-hand side is g itself, followed by the three windows and the edge precisions in torch ops

All of them use one ops.MlpgPlan and preallocated outputs.  They are measured alternately, HIP events around every
call, `--iters` calls per process; a process reports its medians, and the parent starts `--processes` (six) fresh
processes one after the other and reports the median over their medians and the spread (smallest, largest).  (a) is
also given as a fraction of its byte floor -- dim * 4 bytes read and 3 * dim * 4 written per frame at the 8.0 TB/s
HBM3E peak.

Usage: python scripts/bench_mlpg_adjoint.py [--iters N] [--warmup W] [--processes P] [--out FILE.jsonl]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM = 8.0e12                     # bytes / s
UTTERANCES, WIDTH = 64, 187
STREAMS = ((0, 60), (180, 1), (184, 1))          # (first column, dim): coded sp, lf0, bap; V/UV is column 183


def measure(iters, warmup):
    import torch
    from idiaptts_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1234)
    lengths = rng.randint(600, 1601, size=UTTERANCES)
    offsets = [0] + [int(o) for o in np.cumsum(lengths)]
    N, total = offsets[-1], sum(d for _, d in STREAMS)
    plan = ops.MlpgPlan(offsets)
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = torch.randn(N, WIDTH, device=dev, generator=gen)
    gout = torch.randn(N, total, device=dev, generator=gen)
    variances = [torch.tensor(np.repeat([1.3, 0.05, 0.02], d) * rng.uniform(0.5, 2.0, 3 * d), device=dev)
                 for _, d in STREAMS]
    traj = torch.empty(N, total, dtype=torch.float64, device=dev)
    gfeat = torch.zeros(N, WIDTH, device=dev)

    adjoint_forms = []

    def adjoint():
        del adjoint_forms[:]
        o0 = 0
        for (c0, d), var in zip(STREAMS, variances):
            ops.mlpg_adjoint(gout, var, d, offsets, gcol0=o0, out=gfeat, col0=c0, plan=plan)
            adjoint_forms.append(ops.mlpg_form_name(ops.mlpg_adjoint_last_form()))
            o0 += d

    def adjoint_stream():
        with ops.mlpg_adjoint_forced(ops.MLPG_STREAM):
            adjoint()

    def adjoint_sweeps():
        with ops.mlpg_adjoint_forced(ops.MLPG_SWEEPS):
            adjoint()

    forms = []

    def forward():
        o0 = 0
        for (c0, d), var in zip(STREAMS, variances):
            ops.mlpg_generation(rows, var, d, offsets, col0=c0, out=traj, ocol0=o0, plan=plan)
            o0 += d

    # the composition: what it needs besides the forward's kernels, prepared once
    first = torch.zeros(N, 1, device=dev)
    first[offsets[:-1]] = 1.0
    last = torch.zeros(N, 1, device=dev)
    last[[o - 1 for o in offsets[1:]]] = 1.0
    inner, edge = 1.0 - torch.clamp(first + last, max=1.0), torch.clamp(first + last, max=1.0)
    not_first, not_last = (1.0 - first).double(), (1.0 - last).double()
    taus = []
    for (_, d), var in zip(STREAMS, variances):
        t0, t1, t2 = (1.0 / var[w * d:(w + 1) * d] for w in range(3))
        taus.append((var[:d].float(), t0, inner.double() * t1 + edge.double() * 1e-11,
                     inner.double() * t2 + edge.double() * 1e-11))
    rhs_rows = torch.zeros(N, WIDTH, device=dev)
    z = torch.empty(N, total, dtype=torch.float64, device=dev)
    gfeat_c = torch.zeros(N, WIDTH, device=dev)
    zero_row = torch.zeros(1, total, dtype=torch.float64, device=dev)

    def composition():
        o0 = 0
        for (c0, d), var, (v0, _, _, _) in zip(STREAMS, variances, taus):
            rhs_rows[:, c0:c0 + d] = gout[:, o0:o0 + d] * v0
            ops.mlpg_generation(rhs_rows, var, d, offsets, col0=c0, out=z, ocol0=o0, plan=plan)
            o0 += d
        zp = torch.cat((zero_row, z[:-1]), dim=0) * not_first
        zn = torch.cat((z[1:], zero_row), dim=0) * not_last
        o0 = 0
        for (c0, d), (_, t0, t1, t2) in zip(STREAMS, taus):
            zs, zps, zns = z[:, o0:o0 + d], zp[:, o0:o0 + d], zn[:, o0:o0 + d]
            gfeat_c[:, c0:c0 + d] = t0 * zs
            gfeat_c[:, c0 + d:c0 + 2 * d] = t1 * (0.5 * (zns - zps))
            gfeat_c[:, c0 + 2 * d:c0 + 3 * d] = t2 * (zps - 2.0 * zs + zns)
            o0 += d

    fns = (adjoint, forward, composition, adjoint_stream, adjoint_sweeps)
    for _ in range(warmup):
        for fn in fns:
            fn()
    forward()
    forms.append(ops.mlpg_form_name(ops.mlpg_last_form()))
    adjoint_sweeps()
    swept = gfeat.clone()
    adjoint()                                  # (last: gfeat holds the chosen form's gradient, adjoint_forms its forms)
    chosen_forms = list(adjoint_forms)
    torch.cuda.synchronize()
    diff = float((gfeat - gfeat_c).abs().max())
    forms_diff = float((gfeat - swept).abs().max())
    scale = float(gfeat.abs().max())
    times = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    torch.cuda.synchronize()
    plan.close()
    return dict(frames=N, longest=int(lengths.max()), forward_form=forms[0], adjoint_forms=chosen_forms,
                composition_max_abs_diff=diff, stream_sweeps_max_abs_diff=forms_diff,
                gradient_max_abs=scale, adjoint_ms=float(np.median(times[0])), forward_ms=float(np.median(times[1])),
                composition_ms=float(np.median(times[2])), adjoint_stream_ms=float(np.median(times[3])),
                adjoint_sweeps_ms=float(np.median(times[4])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--processes", type=int, default=6)
    ap.add_argument("--out", default=None, help="append the result line to this file as well")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_mlpg_adjoint.py needs a GPU: nothing is measured without one")
        print(json.dumps(measure(args.iters, args.warmup)), flush=True)
        return
    runs = []
    for _ in range(args.processes):           # fresh processes, one at a time
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters),
                              "--warmup", str(args.warmup)], stdout=subprocess.PIPE, universal_newlines=True, timeout=600)
        if res.returncode != 0:
            raise SystemExit("a measuring process failed with status {}".format(res.returncode))
        runs.append(json.loads(res.stdout.strip().splitlines()[-1]))
    out = dict(kernel="mlpg_adjoint", utterances=UTTERANCES, streams=[d for _, d in STREAMS], dtype="float32",
               processes=args.processes, iters=args.iters)
    for key in ("frames", "longest", "forward_form", "adjoint_forms", "composition_max_abs_diff",
                "stream_sweeps_max_abs_diff", "gradient_max_abs"):
        out[key] = runs[0][key]
    for name in ("adjoint", "forward", "composition", "adjoint_stream", "adjoint_sweeps"):
        vals = [r[name + "_ms"] for r in runs]
        out[name + "_ms"] = round(float(np.median(vals)), 4)
        out[name + "_ms_spread"] = [round(min(vals), 4), round(max(vals), 4)]
    floor_bytes = out["frames"] * sum(out["streams"]) * 16.0
    out["adjoint_floor_bytes"] = floor_bytes
    out["adjoint_floor_ms"] = round(floor_bytes / PEAK_HBM * 1e3, 5)
    out["adjoint_fraction_of_floor_rate"] = round(floor_bytes / PEAK_HBM * 1e3 / out["adjoint_ms"], 4)
    out["adjoint_vs_composition"] = round(out["adjoint_ms"] / out["composition_ms"], 3)
    out["adjoint_below_composition_beyond_spread"] = bool(out["adjoint_ms_spread"][1] < out["composition_ms_spread"][0])
    out["adjoint_above_composition_beyond_spread"] = bool(out["adjoint_ms_spread"][0] > out["composition_ms_spread"][1])
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
