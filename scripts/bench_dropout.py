"""Times dropout in the feed-forward acoustic model, 425 -> 512 -> 512 -> 187 on 32 utterances per step (bench.py's
model and batch):

  flat      the flat training step (native_ff.FlatFFModel.train_step) without dropout and with `hparams.dropout`'s
            layout, a dropout of p behind every layer; the masks are made in the GEMM epilogues (csrc/dropout.h)
  module    the module path -- RNNDyn in train() on the padded batch, masked MSE, backward, Adam -- with the same
            dropout: one chain node per group with the masks in the epilogues.  On a commit from before the fused
            dropout the same loop runs torch's nn.Dropout between per-layer nodes, which is what this script is
            there to compare with (it leaves the flat dropout configurations out there: that commit cannot run them)
  kernels   the products of the 512-wide hidden layer alone, with and without the rule in the epilogue

The configurations take turns round by round (the clock drifts over a run); per configuration the median over rounds
of the mean step time of a round, and the spread (max - min) over rounds.

Usage: python scripts/bench_dropout.py [--rounds R] [--steps K] [--p 0.1,0.5] [--skip-module]"""
import argparse
import inspect
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idiaptts_amd import ops  # noqa: E402
from idiaptts_amd.bench_support import make_ff_batch, pad_batch  # noqa: E402
from idiaptts_amd.native_ff import FlatFFModel  # noqa: E402

DIMS = (425, 512, 512, 187)
MODEL_TYPE = "RNNDYN-2_TANH_512-1_FC_187"


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(steps):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def module_step(p, dev, batches):
    from idiaptts_amd.src.neural_networks.pytorch.models import rnn_dyn
    hp = types.SimpleNamespace(model_type=MODEL_TYPE, batch_first=True, dropout=p)
    model = rnn_dyn.convert_legacy_to_config((DIMS[0],), hp).create_model().to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    padded = []
    for x, y, lengths in batches:
        lt = torch.as_tensor(lengths)
        mask = (torch.arange(int(lt.max()))[None, :] < lt[:, None]).unsqueeze(-1).float().to(dev)
        padded.append((pad_batch(x, lt).contiguous(), pad_batch(y, lt).contiguous(), mask, lt, float(lt.sum())))

    def step(i):
        x, y, mask, lt, n = padded[i % len(padded)]
        pred, _ = model(x, seq_lengths_input=lt, max_length_inputs=x.shape[1])
        loss = (((pred - y) ** 2) * mask).sum() / (n * DIMS[-1])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--ramp-steps", type=int, default=100)
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--p", default="0.1,0.5")
    ap.add_argument("--skip-module", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ps = [float(v) for v in args.p.split(",")]
    fused = "dropouts" in inspect.signature(FlatFFModel.__init__).parameters
    raw = [make_ff_batch(args.utts, seed=1000 * b, device=dev) for b in range(4)]
    frames = sum(float(l.sum()) for _, _, l in raw) / len(raw)

    configs = {}
    flat_ps = [0.0] + (ps if fused else [])
    for p in flat_ps:
        model = FlatFFModel(DIMS, device=dev, seed=0, **({"dropouts": (p, p, p)} if fused else {}))
        batches = []
        for x, y, lengths in raw:
            xp = model.pack_input(x)
            batches.append((xp, y, torch.ones(xp.shape[0], dtype=torch.uint8, device=dev), float(lengths.sum())))

        def step(i, model=model, batches=batches):
            x, y, valid, nv = batches[i % len(batches)]
            model.train_step(x, y, valid, nv, lr=1e-3)
        configs["flat p={}".format(p)] = step
    if not args.skip_module:
        for p in [0.0] + ps:
            configs["module p={}".format(p)] = module_step(p, dev, raw)

    times = {n: [] for n in configs}
    for _ in range(args.rounds):
        for n, step in configs.items():
            timed(step, args.ramp_steps)
            times[n].append(timed(step, args.steps))
    med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    out = {"model": "425 -> 512 (Tanh) -> 512 (Tanh) -> 187, dropout behind every layer", "fused_dropout": fused,
           "valid_frames_per_step": frames, "ms_per_step_median": med,
           "ms_per_step_spread": {n: max(t) - min(t) for n, t in times.items()}, "ms_per_step_rounds": times}
    out["ratio_to_flat_p0"] = {n: v / med["flat p=0.0"] for n, v in med.items()}

    if fused:
        # the hidden layer's products alone: forward with bias + Tanh, and both gradients in one launch
        M = raw[0][0].shape[0]
        g = torch.Generator().manual_seed(0)
        x = torch.rand(M, 512, generator=g).to(dev)
        w, b = ((torch.rand(512, 512, generator=g) - 0.5) / 16).to(dev), torch.zeros(512, device=dev)
        dz = (torch.rand(M, 512, generator=g) - 0.5).to(dev)
        y, dw, db, dx = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b), torch.empty_like(x)
        kernels = {}
        for p in [0.0] + ps:
            kernels["fwd p={}".format(p)] = lambda i, p=p: ops.linear_fwd_dropout(x, w, b, ops.ACT_TANH, p=p, seed=i,
                                                                                 salt=1, out=y)
            kernels["bwd p={}".format(p)] = lambda i, p=p: ops.linear_bwd_dropout(dz, x, w, dw, db, dx, yprev=x,
                                                                                 act_prev=ops.ACT_TANH, p=p, seed=i,
                                                                                 salt=0)
        kt = {n: [] for n in kernels}
        for _ in range(args.rounds):
            for n, fn in kernels.items():
                timed(fn, 300)
                kt[n].append(1e3 * timed(fn, 500))
        out["kernel_rows"] = M
        out["kernel_us_median"] = {n: sorted(t)[len(t) // 2] for n, t in kt.items()}
        out["kernel_us_spread"] = {n: max(t) - min(t) for n, t in kt.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
