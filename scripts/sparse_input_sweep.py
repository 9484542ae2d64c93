"""Density sweep behind native_ff.SPARSE_INPUT_MAX_DENSITY: layer 0's forward product of bench.py's model
(x [M, 428] of 32 utterances against w [512, 428], bias + tanh) as the dense launch and as row-list build + sparse
launch, at several shares of non-zeros in x.  Each form is queued `--calls` times back to back between two events
on the launch stream (the host side hides behind the launch before it), the forms take turns round by round, and
the median over rounds is reported.  The same for layer 0's weight gradient (dz [M, 512]): the dense launch, the
column build and the sparse launch (native_ff's sparse_wgrad).  The last rows are one skewed input (34 columns at
0.9, the rest filling up to 10 % overall) and the bench's own input (make_ff_batch).

Usage: python scripts/sparse_input_sweep.py [--rounds R] [--calls C] [--densities 0.02,0.05,...]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idiaptts_amd import ops  # noqa: E402
from idiaptts_amd.bench_support import make_ff_batch  # noqa: E402
from idiaptts_amd.native_ff import FlatFFModel  # noqa: E402


def queued_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--densities", default="0.02,0.05,0.1,0.2,0.3,0.5")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = FlatFFModel((425, 512, 512, 187), ("tanh", "tanh", None), device=dev, seed=0)
    xq, _, _ = make_ff_batch(args.utts, seed=0, device=dev)
    xq = model.pack_input(xq)
    M = xq.shape[0]
    g = torch.Generator(device=dev).manual_seed(1)
    inputs = []
    for d in [float(v) for v in args.densities.split(",")]:
        x = torch.zeros_like(xq)
        keep = torch.rand((M, 425), generator=g, device=dev) < d
        x[:, :425] = torch.where(keep, 1.0 - torch.rand((M, 425), generator=g, device=dev), torch.zeros((), device=dev))
        inputs.append(("%g" % d, x))
    dens = torch.full((425,), (0.10 * 425 - 0.9 * 34) / (425 - 34), device=dev)
    dens[torch.randperm(425, generator=g, device=dev)[:34]] = 0.9
    keep = torch.rand((M, 425), generator=g, device=dev) < dens[None, :]
    x = torch.zeros_like(xq)
    x[:, :425] = torch.where(keep, 1.0 - torch.rand((M, 425), generator=g, device=dev), torch.zeros((), device=dev))
    inputs.append(("skewed", x))
    inputs.append(("make_ff_batch", xq))
    dz = model._rows_buffer("dz0", M, 512)
    dz.copy_(torch.rand((M, 512), generator=g, device=dev) - 0.5)
    dw, db = model.weight_padded(0, model.grads), model.bias(0, model.grads)
    w, b, out = model.weight_padded(0), model.bias(0), model._rows_buffer("h0", M, 512)
    rows = []
    for name, x in inputs:
        lists = ops.sparse_rows_build(x, want_record=True)
        plan = ops.sparse_cols_plan(x, K=425)
        cols = ops.sparse_cols_build(x, plan, K=425)
        forms = {
            "dense_fwd": lambda: ops.linear_fwd(x, w, b, ops.ACT_TANH, out=out),
            "build": lambda: ops.sparse_rows_build(x, lists=lists, want_record=False),
            "sparse_fwd": lambda: ops.linear_fwd_sparse(lists, x, w, b, ops.ACT_TANH, out=out),
            "dense_dw": lambda: ops.linear_bwd_weight(dz, x, dw=dw, db=db),
            "col_build": lambda: ops.sparse_cols_build(x, plan, K=425, cols=cols),
            "sparse_dw": lambda: ops.linear_bwd_weight_sparse(dz, x, cols, plan, dw=dw, db=db, K=425),
        }
        times = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                queued_us(fn, 10)
                times[k].append(queued_us(fn, args.calls))
        med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
        rows.append({"input": name, "measured_density": lists.density(), "max_nnz_per_row": lists.record()[1],
                     "us": med, "us_build_plus_sparse": med["build"] + med["sparse_fwd"],
                     "sparse_over_dense": (med["build"] + med["sparse_fwd"]) / med["dense_fwd"],
                     "heavy_columns": len(plan.heavy),
                     "dw_sparse_over_dense": (med["col_build"] + med["sparse_dw"]) / med["dense_dw"]})
    print(json.dumps({"shape": {"M": M, "N": 512, "K": 428}, "calls": args.calls, "rounds": args.rounds,
                      "rows": rows}))


if __name__ == "__main__":
    main()
