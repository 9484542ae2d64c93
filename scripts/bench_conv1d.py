"""Times the Conv1d implicit-GEMM kernels (csrc/conv1d.hip) against a yardstick at the same FLOPs: an explicit im2col
([B*T_out, Kw*Cin], zero at the utterance edges) followed by the dense-layer GEMMs itts_linear_fwd /
itts_linear_bwd_input / itts_linear_bwd_weight.  Per product: median of many launches after a warm-up (CUDA events
around each launch), TFLOP/s and the fraction of the 157.3 TFLOP/s fp32-matrix peak.  For kernel-only times run it
under `rocprofv3 --kernel-trace --stats -- python scripts/bench_conv1d.py`.

Usage: python scripts/bench_conv1d.py [--iters N] [--warmup W]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idiaptts_amd import ops  # noqa: E402

PEAK_TFLOPS = 157.3
SHAPES = [   # name, B, T, Cin, Cout, Kw
    ("512x512_k5", 32, 1600, 512, 512, 5),
    ("425x512_k5", 32, 1600, 425, 512, 5),
    ("409x16_k3", 32, 1600, 409, 16, 3),
]


def _median_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    times.sort()
    return times[len(times) // 2]


def im2col(x, Kw, pad, dil):
    """[B, T, C] -> [B*T_out, Kw*C] tap-major, zero outside each utterance"""
    B, T, C = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, pad, pad))
    T_out = T + 2 * pad - dil * (Kw - 1)
    return torch.cat([xp[:, k * dil:k * dil + T_out] for k in range(Kw)], dim=2).reshape(B * T_out, Kw * C)


def bench_shape(name, B, T, Cin, Cout, Kw, iters, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    pad, dil = (Kw - 1) // 2, 1
    x = torch.randn(B, T, Cin, device=dev, generator=g)
    w = torch.randn(Cout, Cin, Kw, device=dev, generator=g) / (Cin * Kw) ** 0.5
    b = torch.randn(Cout, device=dev, generator=g)
    T_out = T + 2 * pad - dil * (Kw - 1)
    dz = torch.randn(B, T_out, Cout, device=dev, generator=g)
    flops = 2.0 * B * T_out * Cout * Cin * Kw
    wt = w.permute(0, 2, 1).reshape(Cout, Kw * Cin).contiguous()
    xcol = im2col(x, Kw, pad, dil)
    dz2 = dz.reshape(B * T_out, Cout)
    res = {}
    runs = {
        "fwd": lambda: ops.conv1d_fwd(x, w, b, pad, dil, True),
        "bwd_input": lambda: ops.conv1d_bwd_input(dz, w, T, pad, dil, True),
        "bwd_weight": lambda: ops.conv1d_bwd_weight(dz, x, Kw, pad, dil, True),
        "yard_fwd_gemm": lambda: ops.linear_fwd(xcol, wt, b),
        "yard_bwd_input_gemm": lambda: ops.linear_bwd_input(dz2, wt),
        "yard_bwd_weight_gemm": lambda: ops.linear_bwd_weight(dz2, xcol),
        "yard_im2col": lambda: im2col(x, Kw, pad, dil),
    }
    for key, fn in runs.items():
        us = _median_us(fn, iters, warmup)
        res[key + "_us"] = round(us, 2)
        if key != "yard_im2col":
            tf = flops / us * 1e-6
            res[key + "_tflops"] = round(tf, 2)
            res[key + "_peak_frac"] = round(tf / PEAK_TFLOPS, 3)
    for p in ("fwd", "bwd_input", "bwd_weight"):
        res[p + "_vs_gemm"] = round(res[p + "_us"] / res["yard_{}_gemm_us".format(p)], 3)
        res[p + "_vs_gemm_plus_im2col"] = round(res[p + "_us"] / (res["yard_{}_gemm_us".format(p)]
                                                                 + res["yard_im2col_us"]), 3)
    res.update(shape=name, B=B, T=T, Cin=Cin, Cout=Cout, Kw=Kw, gflop=round(flops * 1e-9, 2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    for spec in SHAPES:
        print(json.dumps(bench_shape(*spec, iters=args.iters, warmup=args.warmup)), flush=True)


if __name__ == "__main__":
    main()
