"""Times the raw-waveform kernels (csrc/mol.hip):

  mol      the discretized mixture-of-logistics loss, forward plus gradient from one call, at [8, 30, 16 000] (ten
           mixtures on one second of 16 kHz audio) and [8, 3, 16 000] (one mixture), shift 1, 65 536 classes,
           log_scale_min log(1e-14), hinge on -- MolLossFunction forward + backward against the reference's flow
           restated in torch on the same device and the same tensors (the slices, some thirty [B, T, K] temporaries
           and as many autograd nodes) and its backward;
  onehot   the mu-law one-hot targets of 8 signals of 16 000 samples (mu = 255) in one launch, against companding and
           a scatter into zeros in torch on the device;
  linear   sample_linearly_batch of 8 utterances of 200 frames with 80 features, multiplier 80 (5 ms frames to
           16 kHz), against torch.nn.functional.interpolate(mode="linear", align_corners=True), which computes the
           same grid in float32.

The two sides of a pair are measured alternately in one run, five repeats of `--iters` launches each; reported are the
median over the repeats' medians, the spread, the byte floor (the inputs read once, the outputs written once) over
the time as a fraction of the 8.0 TB/s HBM3E peak, and the ratio to torch (below 1: faster).

Usage: python scripts/bench_mol.py [--iters N] [--warmup W] [--repeats R]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idiaptts_amd import ops  # noqa: E402
from idiaptts_amd.misc.utils import sample_linearly_batch  # noqa: E402
from idiaptts_amd.nn.functional import MolLossFunction, unit_gradient  # noqa: E402

PEAK_HBM = 8.0e12                     # bytes / s
MOL_SHAPES = ((8, 30, 16000), (8, 3, 16000))
NUM_CLASSES, LOG_SCALE_MIN = 65536, math.log(1e-14)
DEV = torch.device("cuda:0")


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


def torch_flow(x, y, shift, num_classes, log_scale_min):
    """the reference's forward in torch ops (blended conditions, two-sigmoid difference, hinge), mean over frames"""
    inp, tgt = x[..., :-shift], y[..., shift:]
    K = inp.shape[1] // 3
    yh = inp.transpose(1, 2)
    logit, mean = yh[..., :K], yh[..., K:2 * K]
    ls = torch.clamp(yh[..., 2 * K:], min=log_scale_min)
    yy = tgt.transpose(1, 2).expand_as(mean)
    c = yy - mean
    inv = torch.exp(-ls)
    plus_in = inv * (c + 1. / (num_classes - 1))
    min_in = inv * (c - 1. / (num_classes - 1))
    cdf_delta = torch.sigmoid(plus_in) - torch.sigmoid(min_in)
    mid_in = inv * c
    log_pdf_mid = mid_in - ls - 2. * F.softplus(mid_in)
    c3 = (cdf_delta > 1e-5).float()
    o3 = c3 * torch.log(torch.clamp(cdf_delta, min=1e-12)) + (1. - c3) * (log_pdf_mid - np.log((num_classes - 1) / 2))
    c2 = (yy > 0.999).float()
    o2 = c2 * -F.softplus(min_in) + (1. - c2) * o3
    c1 = (yy < -0.999).float()
    lp = c1 * (plus_in - F.softplus(plus_in)) + (1. - c1) * o2
    lp = lp + F.log_softmax(logit, -1)
    m = lp.max(dim=-1, keepdim=True).values
    nll = -(m[..., 0] + torch.log(torch.exp(lp - m).sum(dim=-1)))
    nll = nll + torch.clamp(-inp[:, 2 * K:, :] - math.log(num_classes), min=0.0).sum(dim=1)
    return nll.mean()


def bench_mol(B, C, T, args):
    g = torch.Generator(device=DEV).manual_seed(C + T)
    x = torch.randn(B, C, T, device=DEV, generator=g)
    x[:, C // 3:2 * C // 3] *= 0.6
    x[:, 2 * C // 3:] = 1.5 * x[:, 2 * C // 3:] - 3.0
    x.requires_grad_(True)
    y = torch.rand(B, 1, T, device=DEV, generator=g) * 1.98 - 0.99
    w = torch.full((B * (T - 1),), 1.0 / (B * (T - 1)), device=DEV)

    def ours():
        x.grad = None
        loss = MolLossFunction.apply(x, y, w, NUM_CLASSES, LOG_SCALE_MIN, 1, True, False)
        loss.backward(gradient=unit_gradient(loss))

    def yard():
        x.grad = None
        torch_flow(x, y, 1, NUM_CLASSES, LOG_SCALE_MIN).backward()

    ours()
    g_ours = x.grad.clone()
    yard()
    rel = ((g_ours - x.grad).norm() / x.grad.norm()).item()
    nbytes = 4 * (2 * B * C * T + B * T + B * (T - 1))          # x, grad, y, w
    return _medians_ms([ours, yard], args.iters, args.warmup, args.repeats), nbytes, rel


def bench_onehot(args, n_signals=8, n=16000, mu=255):
    g = torch.Generator(device=DEV).manual_seed(1)
    x = (torch.randn(n_signals * n, device=DEV, generator=g, dtype=torch.float64) * 0.3).clamp(-1.0, 0.99)
    begins, lengths = [s * n for s in range(n_signals)], [n] * n_signals
    out = torch.empty((n_signals * n, mu + 1), dtype=torch.float32, device=DEV)

    def ours():
        ops.mulaw_onehot(x, begins, lengths, mu, out=out)

    def yard():
        idx = ((torch.sign(x) * torch.log(1 + mu * x.abs()) / math.log(1 + mu) + 1.0) * (mu / 2.0)).long()
        return torch.zeros((x.numel(), mu + 1), dtype=torch.float32, device=DEV).scatter_(1, idx[:, None], 1.0)

    ours()
    same = bool(torch.equal(out, yard()))
    nbytes = 8 * x.numel() + 4 * out.numel()
    return _medians_ms([ours, yard], args.iters, args.warmup, args.repeats), nbytes, same


def bench_linear(args, n_utts=8, T=200, D=80, m=80):
    g = torch.Generator(device=DEV).manual_seed(2)
    samples = [torch.randn(T, D, device=DEV, generator=g) for _ in range(n_utts)]
    stacked = torch.stack(samples).transpose(1, 2).contiguous()          # [n, D, T] for interpolate

    def ours():
        return sample_linearly_batch(samples, m)

    def yard():
        return F.interpolate(stacked, size=m * T, mode="linear", align_corners=True).transpose(1, 2).contiguous()

    diff = (torch.stack(ours()) - yard()).abs().max().item()
    nbytes = 4 * n_utts * T * D * (1 + m)
    return _medians_ms([ours, yard], args.iters, args.warmup, args.repeats), nbytes, diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    for B, C, T in MOL_SHAPES:
        (ours, yard), nbytes, rel = bench_mol(B, C, T, args)
        name = "mol_{}x{}x{}".format(B, C, T)
        _report(res, name, ours, yard, nbytes)
        res[name + "_grad_rel_diff_to_torch"] = rel
    (ours, yard), nbytes, same = bench_onehot(args)
    _report(res, "onehot_8x16000_mu255", ours, yard, nbytes)
    res["onehot_8x16000_mu255_equals_torch"] = same
    (ours, yard), nbytes, diff = bench_linear(args)
    _report(res, "linear_8x200x80_m80", ours, yard, nbytes)
    res["linear_8x200x80_m80_max_diff_to_torch"] = diff
    print(json.dumps(res))


if __name__ == "__main__":
    main()
