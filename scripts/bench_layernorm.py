"""Times the LayerNorm row kernels (csrc/layernorm.hip) against torch's own kernels on the same device: forward and
backward separately, with and without a fused Tanh (the yardstick then runs torch.tanh / its derivative as separate
kernels, as a LayerNorm group of the reference does).  Per variant: median of many launches after a warm-up (device
events around each launch, alternating the two implementations), milliseconds, the bytes the algorithm has to move
(forward: read x, write y; backward: read x and dy, and y under an activation, write dx) over that time as a
fraction of the 8.0 TB/s HBM3E peak, and the ratio to the yardstick (below 1: faster than torch).
For kernel-only times run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_layernorm.py`.

Usage: python scripts/bench_layernorm.py [--iters N] [--warmup W]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idiaptts_amd import ops  # noqa: E402

PEAK_HBM = 8.0e12                     # bytes / s
ROWS = 32 * 1600                      # a batch of 32 utterances of 8 s at 5 ms frames
WIDTHS = (512, 1024, 67)              # two hidden widths and the output width


def _median_ms(fns, iters, warmup):
    """the medians of the callables' launch times, taken alternately"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    out = []
    for t in times:
        t.sort()
        out.append((t[len(t) // 2], t[len(t) // 10], t[len(t) * 9 // 10]))
    return out


def bench_width(D, tanh, iters, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(D)
    x = torch.randn(ROWS, D, device=dev, generator=g) + 3
    gamma = 1 + 0.1 * torch.randn(D, device=dev, generator=g)
    beta = torch.randn(D, device=dev, generator=g)
    dy = torch.randn(ROWS, D, device=dev, generator=g)
    act = ops.ACT_TANH if tanh else ops.ACT_NONE
    y, mean, rstd = ops.layer_norm_fwd(x, gamma, beta, 1e-5, act)
    out, dx = torch.empty_like(x), torch.empty_like(x)

    def ours_fwd():
        ops.layer_norm_fwd(x, gamma, beta, 1e-5, act, out=out)

    def ours_bwd():
        ops.layer_norm_bwd(dy, x, mean, rstd, gamma, y=y, act=act, dx=dx)

    def torch_fwd():
        z = torch.nn.functional.layer_norm(x, (D,), gamma, beta, 1e-5)
        return torch.tanh(z) if tanh else z

    # the yardstick's backward through autograd on a graph built once
    xg, gg, bg = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    z = torch.nn.functional.layer_norm(xg, (D,), gg, bg, 1e-5)
    yt = torch.tanh(z) if tanh else z

    def torch_bwd():
        torch.autograd.grad(yt, (xg, gg, bg), dy, retain_graph=True)

    err = (torch_fwd() - y).abs().max().item()
    (f_ours, f_torch), (b_ours, b_torch) = (_median_ms(pair, iters, warmup)
                                            for pair in ((ours_fwd, torch_fwd), (ours_bwd, torch_bwd)))
    bytes_fwd = 2.0 * ROWS * D * 4
    bytes_bwd = (4.0 if tanh else 3.0) * ROWS * D * 4
    res = dict(rows=ROWS, D=D, act="Tanh" if tanh else None, max_abs_diff_to_torch=err)
    for name, ours, yard, nbytes in (("fwd", f_ours, f_torch, bytes_fwd), ("bwd", b_ours, b_torch, bytes_bwd)):
        res[name + "_ms"] = round(ours[0], 4)
        res[name + "_ms_p10_p90"] = [round(ours[1], 4), round(ours[2], 4)]
        res[name + "_hbm_peak_frac"] = round(nbytes / (ours[0] * 1e-3) / PEAK_HBM, 3)
        res[name + "_torch_ms"] = round(yard[0], 4)
        res[name + "_torch_ms_p10_p90"] = [round(yard[1], 4), round(yard[2], 4)]
        res[name + "_vs_torch"] = round(ours[0] / yard[0], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_layernorm.py needs a GPU: nothing is measured without one")
    for D in WIDTHS:
        for tanh in (False, True):
            print(json.dumps(bench_width(D, tanh, args.iters, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
