"""Times the softmax cross-entropy kernels (csrc/xent.hip), loss + gradient from one call, against
`torch.nn.functional.cross_entropy` + autograd on the same device and the same tensors:

  rows     class-contiguous logits [64, 5] and [64, 256] (utterance level) and [73 138, 64] (frame level: the
           recurrent benchmarks' batch of 64 utterances), reduction 'mean' -- SoftmaxXentFunction forward + backward
           against cross_entropy(reduction='none').mean() and its backward;
  strided  class-strided logits [8, 256, 16 000] with a one-hot target of the same shape, shift 1 (the mu-law case of
           loss/OneHotCrossEntropyLoss.py) -- SoftmaxXentStridedFunction against target.max(dim=1), the two slices and
           cross_entropy on [B, C, T - 1], and its backward.

The two sides of a pair are measured alternately in one run, five repeats of `--iters` launches each; reported are the
median over the repeats' medians, the spread (min .. max of the repeats' medians), the byte floor -- the logits read
once and the gradient written once (the strided form also has to read the one-hot target once: reported as
`floor_with_target`) -- over the time as a fraction of the 8.0 TB/s HBM3E peak, and the ratio to torch (below 1:
faster).  For kernel-only times run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_xent.py`.

Usage: python scripts/bench_xent.py [--iters N] [--warmup W] [--repeats R]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idiaptts_amd.nn.functional import (SoftmaxXentFunction, SoftmaxXentStridedFunction,  # noqa: E402
                                        unit_gradient)

PEAK_HBM = 8.0e12                     # bytes / s
ROW_SHAPES = ((64, 5), (64, 256), (73138, 64))
STRIDED_SHAPE = (8, 256, 16000)


def _medians_ms(fns, iters, warmup, repeats):
    """per callable: (median of the repeats' medians, smallest, largest repeat median); launches alternate"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    meds = [[] for _ in fns]
    for _ in range(repeats):
        times = [[] for _ in fns]
        for _ in range(iters):
            for i, fn in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[i].append(a.elapsed_time(b))
        for i, t in enumerate(times):
            meds[i].append(float(np.median(t)))
    return [(float(np.median(m)), min(m), max(m)) for m in meds]


def _report(res, name, ours, yard, nbytes):
    res[name + "_ms"] = round(ours[0], 4)
    res[name + "_ms_spread"] = [round(ours[1], 4), round(ours[2], 4)]
    res[name + "_floor_bytes"] = int(nbytes)
    res[name + "_hbm_peak_frac"] = round(nbytes / (ours[0] * 1e-3) / PEAK_HBM, 4)
    res[name + "_torch_ms"] = round(yard[0], 4)
    res[name + "_torch_ms_spread"] = [round(yard[1], 4), round(yard[2], 4)]
    res[name + "_vs_torch"] = round(ours[0] / yard[0], 3)
    res[name + "_faster_beyond_spread"] = bool(ours[2] < yard[1])
    res[name + "_slower_beyond_spread"] = bool(ours[1] > yard[2])


def bench_rows(N, C, args):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N + C)
    x = (torch.randn(N, C, device=dev, generator=g) * 3).requires_grad_(True)
    t = torch.randint(0, C, (N,), device=dev, generator=g)
    w = torch.full((N,), 1.0 / N, device=dev)

    def ours():
        x.grad = None
        loss = SoftmaxXentFunction.apply(x, t, w, None, -100, False)
        loss.backward(gradient=unit_gradient(loss))          # (the trainers' start of backward: the factor is 1)

    def yard():
        x.grad = None
        torch.nn.functional.cross_entropy(x, t, reduction="none").mean().backward()

    ours()
    g_ours = x.grad.clone()
    yard()
    err = (g_ours - x.grad).abs().max().item()
    return _medians_ms([ours, yard], args.iters, args.warmup, args.repeats), 2 * 4 * N * C, err


def bench_strided(B, C, T, args):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(C + T)
    x = (torch.randn(B, C, T, device=dev, generator=g) * 3).requires_grad_(True)
    idx = torch.randint(0, C, (B, T), device=dev, generator=g)
    onehot = torch.zeros(B, C, T, device=dev).scatter_(1, idx[:, None, :], 1.0)
    w = torch.full((B * (T - 1),), 1.0 / (B * (T - 1)), device=dev)

    def ours():
        x.grad = None
        loss = SoftmaxXentStridedFunction.apply(x, onehot, w, None, -100, 1, False)
        loss.backward(gradient=unit_gradient(loss))

    def yard():
        x.grad = None
        targets = onehot.max(dim=1)[1]
        torch.nn.functional.cross_entropy(x[..., :-1], targets[..., 1:], reduction="none").mean().backward()

    ours()
    g_ours = x.grad.clone()
    yard()
    err = (g_ours - x.grad).abs().max().item()
    return _medians_ms([ours, yard], args.iters, args.warmup, args.repeats), 2 * 4 * B * C * T, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    for N, C in ROW_SHAPES:
        (ours, yard), nbytes, err = bench_rows(N, C, args)
        name = "rows_{}x{}".format(N, C)
        _report(res, name, ours, yard, nbytes)
        res[name + "_grad_max_diff_to_torch"] = err
    B, C, T = STRIDED_SHAPE
    (ours, yard), nbytes, err = bench_strided(B, C, T, args)
    name = "strided_{}x{}x{}".format(B, C, T)
    _report(res, name, ours, yard, nbytes)
    res[name + "_floor_with_target_hbm_peak_frac"] = round(1.5 * nbytes / (ours[0] * 1e-3) / PEAK_HBM, 4)
    res[name + "_grad_max_diff_to_torch"] = err
    print(json.dumps(res))


if __name__ == "__main__":
    main()
