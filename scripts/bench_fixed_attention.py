"""Times the fixed-attention kernels (csrc/fixed_attention.hip) against the reference's torch flow on the same device,
and the iterative pass of the decoder:

  attention  64 utterances / 73 138 frames padded to 1 977 (the recurrent benchmarks' batch: lengths
             rint(200 * U(2, 10)), seed 1234 + 7; padded to 1 980 for n = 5, a multiple of the step), 150 phonemes, 512
             channels, hard matrices of random durations, n_frames_per_step 1 and 5 -- ops.fixed_attention (+
             ops.fixed_attention_bwd) against `A.view(B, T / n, n, P).mean(2)` + `torch.bmm` (FixedAttention.py:30-38)
             and autograd's gradient of the encoder output, forward alone and forward + backward.
  decoding   milliseconds per step of the iterative pass (inference, no target) of the autoregressive decoder of the
             tests' fixture at width 512 -- pre-net 2 x Linear 512 ReLU, Linear 512 ReLU + LSTM 512, one projection
             of 5 frames x 3 -- at 1 and 64 rows over 200 frames (40 steps, one attention launch in front).

The two sides of a pair are measured alternately in one run, `--repeats` repeats of `--iters` launches each, HIP
events around every call; reported are the median over the repeats' medians, the spread, the bytes the algorithm has
to move over the time as a fraction of the 8.0 TB/s HBM3E peak, and the ratio to torch (below 1: faster).
For kernel-only times run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_fixed_attention.py`.

Usage: python scripts/bench_fixed_attention.py [--iters N] [--warmup W] [--repeats R] [--skip-decoding]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idiaptts_amd import ops  # noqa: E402
from idiaptts_amd.src.neural_networks.pytorch.models import enc_dec_dyn, rnn_dyn  # noqa: E402

PEAK_HBM = 8.0e12                     # bytes / s
UTTERANCES, PHONEMES, CHANNELS = 64, 150, 512


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


def hard_matrices(lengths, T, P, rng):
    """[B, T, P]: every utterance's frames dealt to its P phonemes in order (random durations, some of them zero)"""
    A = np.zeros((len(lengths), T, P), dtype=np.float32)
    for b, n in enumerate(lengths):
        A[b, np.arange(n), np.sort(rng.integers(0, P, size=n))] = 1.0
    return A


def bench_attention(n, args):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1234 + 7)
    lengths = np.rint(200.0 * rng.uniform(2.0, 10.0, size=UTTERANCES)).astype(np.int64)
    B, P, C = UTTERANCES, PHONEMES, CHANNELS
    T = -(-int(lengths.max()) // n) * n
    K = T // n
    A = torch.as_tensor(hard_matrices(lengths, T, P, rng), device=dev)
    g = torch.Generator(device=dev).manual_seed(n)
    enc = torch.randn(B, P, C, device=dev, generator=g)
    dctx = torch.randn(B, K, C, device=dev, generator=g)

    def ours():                       # both sides allocate their outputs on every call, as the autograd nodes do
        ctx, abar = ops.fixed_attention(A, enc, n)
        ops.fixed_attention_bwd(abar, dctx)
        return ctx

    def ours_fwd():
        return ops.fixed_attention(A, enc, n)[0]

    eg = enc.clone().requires_grad_(True)

    def torch_flow():
        ctx = torch.bmm(A.view(B, K, n, P).mean(dim=2), eg)
        torch.autograd.grad(ctx, eg, dctx)
        return ctx

    def torch_fwd():
        with torch.no_grad():
            return torch.bmm(A.view(B, K, n, P).mean(dim=2), eg)

    err = (torch_fwd() - ours_fwd()).abs().max().item()
    t_ours, t_torch, f_ours, f_torch = _medians_ms((ours, torch_flow, ours_fwd, torch_fwd), args.iters, args.warmup,
                                                   args.repeats)
    res = dict(kernel="fixed_attention", B=B, T=T, P=P, C=C, n=n, frames=int(lengths.sum()), max_abs_diff_to_torch=err,
               plan=ops.fixed_attention_plan(B, T, P, C, n))
    fwd_bytes = 4.0 * (B * T * P + B * K * P + B * K * C + B * P * C)       # A and enc read, Abar and ctx written
    bwd_bytes = 4.0 * (B * K * P + B * K * C + B * P * C)                   # Abar and dctx read, d_enc written
    res["fwd_floor_bytes"], res["bwd_floor_bytes"] = fwd_bytes, bwd_bytes
    _report(res, "fwd_bwd", t_ours, t_torch, fwd_bytes + bwd_bytes)
    _report(res, "fwd", f_ours, f_torch, fwd_bytes)
    return res


def decoder_config(width, n=5, acoustic=3):
    LC = rnn_dyn.Config.LayerConfig
    return enc_dec_dyn.Config(modules=[enc_dec_dyn.Config.DecoderConfig(
        attention_args={enc_dec_dyn.ATTENTION_GROUND_TRUTH: "attention_matrix"},
        attention_config=enc_dec_dyn.FIXED_ATTENTION, teacher_forcing_input_names=["acoustic_features"],
        config=rnn_dyn.Config(in_dim=2 * width, batch_first=True, layer_configs=[
            LC("Linear", out_dim=width, nonlin="ReLU"), LC("LSTM", out_dim=width)]),
        input_names=["phoneme_embeddings"], name="Decoder", n_frames_per_step=n, p_teacher_forcing=1.0,
        pre_net_config=rnn_dyn.Config(in_dim=acoustic, batch_first=True, layer_configs=[
            LC("Linear", out_dim=width, nonlin="ReLU", num_layers=2)]),
        projection_configs=[enc_dec_dyn.Config.ProjectionConfig(
            config=rnn_dyn.Config(in_dim=width, batch_first=True, layer_configs=[LC("Linear", out_dim=acoustic * n)]),
            name="AcousticFeaturesProjector", output_names=["pred_acoustic_features"], out_dim=acoustic,
            is_autoregressive_input=True)])])


def bench_decoding(B, args, width=512, T=200, P=30, n=5):
    dev = torch.device("cuda:0")
    torch.manual_seed(B)
    model = decoder_config(width, n).create_model().to(dev).eval()
    rng = np.random.default_rng(B)
    A = torch.as_tensor(hard_matrices([T] * B, T, P, rng), device=dev)
    enc = torch.randn(B, P, width, device=dev)

    def run():
        data = {"phoneme_embeddings": enc, "attention_matrix": A}
        lens = {"phoneme_embeddings": torch.full((B,), P), "attention_matrix": torch.full((B,), T)}
        maxs = {"phoneme_embeddings": torch.tensor(P), "attention_matrix": torch.tensor(T)}
        model.init_hidden(B)
        with torch.no_grad():
            model.inference(data, lens, maxs)
        return data["pred_acoustic_features"]

    for _ in range(2):
        out = run()
    assert tuple(out.shape) == (B, T, 3) and bool(torch.isfinite(out).all())
    times = []
    for _ in range(max(3, args.repeats)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    steps = T // n
    return dict(kernel="decoder_iterative_pass", B=B, width=width, frames=T, steps=steps,
                ms_per_step=round(float(np.median(times)) / steps, 4),
                ms_per_step_spread=[round(min(times) / steps, 4), round(max(times) / steps, 4)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-decoding", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fixed_attention.py needs a GPU: nothing is measured without one")
    for n in (1, 5):
        print(json.dumps(bench_attention(n, args)), flush=True)
    if not args.skip_decoding:
        for B in (1, 64):
            print(json.dumps(bench_decoding(B, args)), flush=True)


if __name__ == "__main__":
    main()
