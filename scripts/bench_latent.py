"""Times the utterance-embedding kernels (csrc/latent.hip) against the reference's torch expressions on the same
device, forward + backward each:

  pooling    PoolMean and PoolLast of a padded batch of 64 utterances / 73 138 frames (the recurrent benchmarks' batch:
             lengths rint(200 * U(2, 10)), seed 1234 + 7) at widths 512 and 67, batch_first -- ops.time_pool_fwd + _bwd
             against `x.sum(1, keepdim=True) / lengths` (rnn_dyn/Pooling.py:55-64) resp. the index select (:42-44)
             and autograd's backward of either (for the sum an expanded view: torch writes no dx there, the kernel
             writes every position), and the forward alone on both sides;
  VAE        reparameterisation + KL on hidden [64, 1, 2 * 64] -- VAEReparamFunction + VAEKLDFunction and their one
             backward kernel each against rnn_dyn/VAE.py:19-27 + loss/VAEKLDLoss.py:56-58 ('mean_per_frame' on [B, 1, 1]
             values) and autograd.

The two sides of a pair are measured alternately in one run, five repeats of `--iters` launches each; reported are
the median over the repeats' medians, the spread (min .. max of the repeats' medians), the bytes the algorithm has to
move over the time as a fraction of the 8.0 TB/s HBM3E peak, and the ratio to torch (below 1: faster).
For kernel-only times run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_latent.py`.

Usage: python scripts/bench_latent.py [--iters N] [--warmup W] [--repeats R]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idiaptts_amd import ops  # noqa: E402
from idiaptts_amd.nn.functional import VAEKLDFunction, VAEReparamFunction  # noqa: E402

PEAK_HBM = 8.0e12                     # bytes / s
UTTERANCES = 64
WIDTHS = (512, 67)
LATENT = 64


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
    res[name + "_hbm_peak_frac"] = round(nbytes / (ours[0] * 1e-3) / PEAK_HBM, 4)
    res[name + "_torch_ms"] = round(yard[0], 4)
    res[name + "_torch_ms_spread"] = [round(yard[1], 4), round(yard[2], 4)]
    res[name + "_vs_torch"] = round(ours[0] / yard[0], 3)
    res[name + "_faster_beyond_spread"] = bool(ours[2] < yard[1])
    res[name + "_slower_beyond_spread"] = bool(ours[1] > yard[2])


def bench_pool(D, mean, args):
    dev = torch.device("cuda:0")
    lengths = np.rint(200.0 * np.random.default_rng(1234 + 7).uniform(2.0, 10.0, size=UTTERANCES)).astype(np.int64)
    T, B = int(lengths.max()), len(lengths)
    g = torch.Generator(device=dev).manual_seed(D)
    x = torch.randn(B, T, D, device=dev, generator=g)
    x[torch.arange(T, device=dev)[None, :] >= torch.as_tensor(lengths, device=dev)[:, None]] = 0.0
    lens = torch.as_tensor(lengths, device=dev)
    dy = torch.randn(B, D, device=dev, generator=g)
    mode = ops.POOL_MEAN if mean else ops.POOL_LAST

    def ours():                       # both sides allocate their outputs on every call, as the autograd nodes do
        y = ops.time_pool_fwd(x, lens, True, mode)
        ops.time_pool_bwd(dy, lens, T, True, mode)
        return y

    xg = x.clone().requires_grad_(True)
    flens = lens.view(B, 1, 1).float()
    batch_idx, last_idx = torch.arange(B, device=dev), lens - 1
    dy3 = dy.unsqueeze(1)

    def torch_flow():
        if mean:
            yt = xg.sum(1, keepdim=True) / flens
        else:
            yt = xg[batch_idx, last_idx].unsqueeze(dim=1)
        torch.autograd.grad(yt, xg, dy3)
        return yt

    def ours_fwd():
        ops.time_pool_fwd(x, lens, True, mode)

    def torch_fwd():
        with torch.no_grad():
            return xg.sum(1, keepdim=True) / flens if mean else xg[batch_idx, last_idx].unsqueeze(dim=1)

    err = (torch_flow().squeeze(1) - ours()).abs().max().item()
    t_ours, t_torch, f_ours, f_torch = _medians_ms((ours, torch_flow, ours_fwd, torch_fwd), args.iters, args.warmup,
                                                   args.repeats)
    seg, split, _ = ops.time_pool_plan(B, T, D)
    res = dict(kernel="pool_mean" if mean else "pool_last", B=B, T=T, D=D, frames=int(lengths.sum()),
               segments=seg, time_split=split, max_abs_diff_to_torch=err)
    # byte floor: MEAN reads the padded batch once; both modes write every position of dx once
    nbytes = (2.0 if mean else 1.0) * B * T * D * 4 + 3.0 * B * D * 4
    _report(res, "fwd_bwd", t_ours, t_torch, nbytes)
    # the forward alone as well: autograd's gradient of the torch expressions is an expanded view (MEAN) or an
    # index_put into zeros (LAST); the kernel's backward writes every position of dx
    _report(res, "fwd", f_ours, f_torch, (1.0 if mean else 0.0) * B * T * D * 4 + 2.0 * B * D * 4)
    return res


def bench_vae(args):
    dev = torch.device("cuda:0")
    B, L = UTTERANCES, LATENT
    g = torch.Generator(device=dev).manual_seed(3)
    hidden = (0.5 * torch.randn(B, 1, 2 * L, device=dev, generator=g)).requires_grad_(True)
    eps = torch.randn(B, 1, L, device=dev, generator=g)
    gz = torch.randn(B, 1, L, device=dev, generator=g)
    w = torch.full((B,), 1.0 / B, device=dev)

    def ours():
        z, mu, lv = VAEReparamFunction.apply(hidden, eps)
        loss = VAEKLDFunction.apply(mu, lv, w, False)
        torch.autograd.grad((loss, z), hidden, (torch.ones_like(loss), gz))
        return z, loss

    def torch_flow():
        mu, lv = torch.split(hidden, L, dim=2)
        z = eps * torch.exp(0.5 * lv) + mu
        kl = 0.5 * (torch.exp(lv) + mu ** 2 - 1. - lv).sum(dim=-1, keepdim=True)
        loss = (kl.sum(dim=(0, 1)) / B).mean()
        torch.autograd.grad((loss, z), hidden, (torch.ones_like(loss), gz))
        return z, loss

    (z1, l1), (z2, l2) = ours(), torch_flow()
    err = max((z1 - z2).abs().max().item(), abs(float(l1.detach()) - float(l2.detach())))
    t_ours, t_torch = _medians_ms((ours, torch_flow), args.iters, args.warmup, args.repeats)
    res = dict(kernel="vae_reparam_kld", M=B, L=L, max_abs_diff_to_torch=err)
    # byte floor: forward reads h and eps, writes z; KL reads h, writes two gradients; backward reads dz, both
    # KL gradients, h and eps, writes dh
    nbytes = (2 + 1 + 1) * B * L * 4 + (2 + 2) * B * L * 4 + (1 + 2 + 2 + 1 + 2) * B * L * 4
    _report(res, "fwd_bwd", t_ours, t_torch, nbytes)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_latent.py needs a GPU: nothing is measured without one")
    for D in WIDTHS:
        for mean in (True, False):
            print(json.dumps(bench_pool(D, mean, args)), flush=True)
    print(json.dumps(bench_vae(args)), flush=True)


if __name__ == "__main__":
    main()
