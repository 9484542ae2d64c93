"""Times the self-attention kernels (csrc/attention.hip) and a whole nn.TransformerEncoderLayer block against torch on
the same device and tensors:

  core    64 utterances / 73 138 frames padded to 1 977 (the recurrent benchmarks' batch: lengths
          rint(200 * U(2, 10)), seed 1234 + 7), d_model 512 / 8 heads and d_model 256 / 4 heads, float32 --
          ops.attention_forward and forward + ops.attention_backward, masked (keys = each utterance's length) and
          unmasked (keys = all 1 977 positions), against torch.nn.functional.scaled_dot_product_attention in float32
          with the same boolean mask and autograd's gradients.  Algorithmic FLOPs: 4 H dh sum_b T klen_b forward,
          10 H dh sum_b T klen_b backward (five products; the kernels run seven), as a share of the
          157.3 TFLOP/s fp32-MFMA peak.
  block   idiaptts_amd.nn.TransformerEncoderLayer against torch.nn.TransformerEncoderLayer with the same weights,
          dim_feedforward 4 * d_model, dropout 0, masked, forward (no_grad) and forward + backward.

The two sides of a pair are measured alternately in one run, `--repeats` repeats of `--iters` launches each, HIP
events around every call; reported are the median over the repeats' medians, the spread and the ratio to torch
(below 1: faster).  One JSON line per measurement.

Usage: python scripts/bench_attention.py [--iters N] [--warmup W] [--repeats R] [--skip-block]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idiaptts_amd import ops  # noqa: E402
from idiaptts_amd.nn import TransformerEncoderLayer  # noqa: E402

PEAK_MFMA_F32 = 157.3e12              # FLOP / s
UTTERANCES = 64
SHAPES = ((512, 8), (256, 4))         # d_model, heads


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


def _report(res, name, ours, yard, flops=None):
    res[name + "_ms"] = round(ours[0], 4)
    res[name + "_ms_spread"] = [round(ours[1], 4), round(ours[2], 4)]
    if flops is not None:
        res[name + "_tflops"] = round(flops / (ours[0] * 1e-3) / 1e12, 2)
        res[name + "_mfma_peak_frac"] = round(flops / (ours[0] * 1e-3) / PEAK_MFMA_F32, 4)
    res[name + "_torch_ms"] = round(yard[0], 4)
    res[name + "_torch_ms_spread"] = [round(yard[1], 4), round(yard[2], 4)]
    res[name + "_vs_torch"] = round(ours[0] / yard[0], 3)
    res[name + "_faster_beyond_spread"] = bool(ours[2] < yard[1])
    res[name + "_slower_beyond_spread"] = bool(ours[1] > yard[2])


def batch_lengths():
    rng = np.random.default_rng(1234 + 7)
    return np.rint(200.0 * rng.uniform(2.0, 10.0, size=UTTERANCES)).astype(np.int64)


def bench_core(D, H, masked, args):
    dev = torch.device("cuda:0")
    lengths = batch_lengths()
    B, T, dh = UTTERANCES, int(lengths.max()), D // H
    g = torch.Generator(device=dev).manual_seed(D + masked)
    qkv = torch.randn(B, T, 3 * D, device=dev, generator=g)
    do = torch.randn(B, T, D, device=dev, generator=g)
    keys = lengths if masked else np.full(B, T)
    klen = torch.as_tensor(keys, dtype=torch.int32, device=dev) if masked else None
    pairs = float(T) * float(keys.sum())
    o, lse = ops.attention_forward(qkv, H, klen)

    def ours_fwd():
        return ops.attention_forward(qkv, H, klen)

    def ours_both():
        out, stat = ops.attention_forward(qkv, H, klen)
        return ops.attention_backward(do, qkv, out, stat, H, klen)

    # the yardstick on the same tensors: [B, H, T, dh] views of qkv, a boolean key mask broadcast over heads and queries
    leaf = qkv.clone().requires_grad_(True)
    mask = (torch.arange(T, device=dev)[None, :] < torch.as_tensor(keys, device=dev)[:, None])[:, None, None, :] \
        if masked else None

    def sdpa(src):
        q, k, v = (t.reshape(B, T, H, dh).transpose(1, 2) for t in src.split(D, dim=2))
        return torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2).reshape(B, T, D)

    def torch_fwd():
        with torch.no_grad():
            return sdpa(qkv)

    def torch_both():
        return torch.autograd.grad(sdpa(leaf), leaf, do)

    valid = (torch.arange(T, device=dev)[None, :] < torch.as_tensor(lengths, device=dev)[:, None])[..., None]
    err = ((torch_fwd() - o) * valid).abs().max().item()
    err_grad = ((torch_both()[0] - ours_both()) * valid).abs().max().item()
    fwd, both = (_medians_ms(pair, args.iters, args.warmup, args.repeats)
                 for pair in ((ours_fwd, torch_fwd), (ours_both, torch_both)))
    res = dict(kernel="attention", B=B, T=T, D=D, H=H, dh=dh, masked=bool(masked), frames=int(lengths.sum()),
               key_query_pairs=pairs, max_abs_diff_to_torch=err, max_abs_grad_diff_to_torch=err_grad)
    _report(res, "fwd", fwd[0], fwd[1], 4.0 * H * dh * pairs)
    _report(res, "fwd_bwd", both[0], both[1], 14.0 * H * dh * pairs)
    return res


def bench_block(D, H, args):
    dev = torch.device("cuda:0")
    lengths = batch_lengths()
    B, T = UTTERANCES, int(lengths.max())
    torch.manual_seed(D)
    yard = torch.nn.TransformerEncoderLayer(D, H, 4 * D, dropout=0.0, batch_first=True).to(dev).train()
    own = TransformerEncoderLayer(D, H, 4 * D, dropout=0.0, batch_first=True).to(dev).train()
    own.load_state_dict(yard.state_dict())
    g = torch.Generator(device=dev).manual_seed(D)
    x = torch.randn(B, T, D, device=dev, generator=g)
    dy = torch.randn(B, T, D, device=dev, generator=g)
    lens = torch.as_tensor(lengths, device=dev)
    klen = lens.to(torch.int32)
    pad = ~(torch.arange(T, device=dev)[None, :] < lens[:, None])

    def ours_fwd():
        with torch.no_grad():
            return own(x, klen, mask_padding=True)

    def torch_fwd():
        with torch.no_grad():
            return yard(x, src_key_padding_mask=pad)

    def ours_both():
        own.zero_grad(set_to_none=True)
        own(x, klen, mask_padding=True).backward(dy)

    def torch_both():
        yard.zero_grad(set_to_none=True)
        yard(x, src_key_padding_mask=pad).backward(dy)

    err = ((ours_fwd() - torch_fwd()) * ~pad[..., None]).abs().max().item()
    fwd, both = (_medians_ms(pair, args.iters, args.warmup, args.repeats)
                 for pair in ((ours_fwd, torch_fwd), (ours_both, torch_both)))
    res = dict(kernel="transformer_encoder_layer", B=B, T=T, D=D, H=H, F=4 * D, masked=True,
               frames=int(lengths.sum()), max_abs_diff_to_torch=err)
    _report(res, "fwd", fwd[0], fwd[1])
    _report(res, "fwd_bwd", both[0], both[1])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-block", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention.py needs a GPU: nothing is measured without one")
    for D, H in SHAPES:
        times = {}
        for masked in (True, False):
            res = bench_core(D, H, masked, args)
            times[masked] = res
            print(json.dumps(res), flush=True)
        print(json.dumps(dict(kernel="attention", D=D, H=H,
                              masked_over_unmasked_fwd=round(times[True]["fwd_ms"] / times[False]["fwd_ms"], 3),
                              masked_over_unmasked_fwd_bwd=round(times[True]["fwd_bwd_ms"] / times[False]["fwd_bwd_ms"], 3),
                              keys_masked_over_unmasked=round(times[True]["key_query_pairs"]
                                                              / times[False]["key_query_pairs"], 3))), flush=True)
        if not args.skip_block:
            print(json.dumps(bench_block(D, H, args)), flush=True)


if __name__ == "__main__":
    main()
