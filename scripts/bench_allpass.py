"""Times the all-pass warping kernels (csrc/allpass.hip): forward alone and forward + backward, at the two sizes a
VTLN model uses -- 60 coefficients with deltas and delta-deltas (D = 180) and 30 static coefficients (D = 30) -- on a
batch of 32 utterances of 1 600 frames.  Beside each time:
  * the floor of the bytes the operation has to move at the 8.0 TB/s HBM3E peak (forward: read x, write y, 2 M D 4
    bytes; forward + backward: that plus read x and dy, write dx, 5 M D 4 bytes; alpha and dalpha are noise);
  * a torch evaluation on the same device with the reference's data flow (layers/AllPassWarp.py): a [N, N, 2N] table
    of polynomial coefficients in float32 (built here by running the recursion on coefficient vectors), powers of
    alpha by cumprod, one einsum into a [M, N, N] tensor of warp matrices, one bmm per block, autograd through all
    of it for the backward.  At N = 60 the table does not fit float32 and that evaluation returns NaN (as the
    reference does); its time is still the time of that data flow.
Per variant: median (and 10th / 90th percentile) of the launches' device-event times after a warm-up, the two
implementations alternating.  For kernel-only times: `rocprofv3 --kernel-trace --stats -- python
scripts/bench_allpass.py`.

Usage: python scripts/bench_allpass.py [--iters 50] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idiaptts_amd.nn.functional import AllPassWarpFunction  # noqa: E402

PEAK_HBM = 8.0e12                     # bytes / s
ROWS = 32 * 1600
SHAPES = ((60, 180), (30, 30))        # (N, D)


def coefficient_table(N):
    """[N, N, 2N] float64: the polynomial in alpha of every entry of the warp matrix, by the recursion
    W[r][c] = W[r-1][c-1] + alpha (W[r-1][c] - W[r][c-1]) on coefficient vectors"""
    table = np.zeros((N, N, 2 * N))
    table[0, 0, 0] = 1.0
    for r in range(1, N):
        table[r, 0, 1:] = table[r - 1, 0, :-1]
        for c in range(1, N):
            table[r, c] = table[r - 1, c - 1]
            table[r, c, 1:] += (table[r - 1, c] - table[r, c - 1])[:-1]
    return table


def materialising_forward(table, x, alpha, N):
    """the reference's flow: powers, einsum to [M, N, N], halve, bmm per block, double (on a copy of x)"""
    M, D = x.shape
    a = alpha.reshape(M, 1)
    powers = torch.cat([torch.ones_like(a), a.expand(M, 2 * N - 1).cumprod(dim=-1)], dim=-1)
    warp = torch.einsum("ijk,lk->lij", table, powers)
    x = x.clone().view(M, 1, D)
    x[:, :, 0:3 * N:N] /= 2.
    out = torch.empty_like(x)
    for b in range(D // N):
        out[:, :, b * N:(b + 1) * N] = torch.bmm(x[:, :, b * N:(b + 1) * N], warp)
    out[:, :, 0:3 * N:N] *= 2.
    return out.view(M, D)


def _median_ms(fns, iters, warmup):
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


def bench_shape(N, D, iters, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N)
    x = torch.randn(ROWS, D, device=dev, generator=g)
    dy = torch.randn(ROWS, D, device=dev, generator=g)
    alpha = (torch.rand(ROWS, 1, device=dev, generator=g) - 0.5) * 0.4
    with np.errstate(over="ignore"):
        table = torch.from_numpy(coefficient_table(N).astype(np.float32)).to(dev)
    xg, ag = x.clone().requires_grad_(True), alpha.clone().requires_grad_(True)

    def ours_fwd():
        with torch.no_grad():
            AllPassWarpFunction.apply(x, alpha, None, None, N)

    def theirs_fwd():
        with torch.no_grad():
            materialising_forward(table, x, alpha, N)

    def ours_both():
        xg.grad = ag.grad = None
        AllPassWarpFunction.apply(xg, ag, None, None, N).backward(dy)

    def theirs_both():
        xg.grad = ag.grad = None
        materialising_forward(table, xg, ag, N).backward(dy)

    for what, fns, nbytes in (("forward", (ours_fwd, theirs_fwd), 2 * ROWS * D * 4),
                              ("forward+backward", (ours_both, theirs_both), 5 * ROWS * D * 4)):
        (ours, lo, hi), (theirs, tlo, thi) = _median_ms(fns, iters, warmup)
        floor_ms = nbytes / PEAK_HBM * 1e3
        print(json.dumps({"bench": "allpass", "what": what, "N": N, "D": D, "rows": ROWS, "iters": iters,
                          "ms": round(ours, 4), "ms_p10": round(lo, 4), "ms_p90": round(hi, 4),
                          "bytes_floor_ms": round(floor_ms, 4), "times_floor": round(ours / floor_ms, 1),
                          "materialising_ms": round(theirs, 4), "materialising_ms_p10": round(tlo, 4),
                          "materialising_ms_p90": round(thi, 4),
                          "materialised_bytes": ROWS * N * N * 4,
                          "ratio_to_materialising": round(ours / theirs, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_allpass.py needs a GPU: nothing is measured without one")
    for N, D in SHAPES:
        bench_shape(N, D, args.iters, args.warmup)


if __name__ == "__main__":
    main()
