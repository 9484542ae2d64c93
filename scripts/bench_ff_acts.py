"""Times the flat feed-forward training step (native_ff.FlatFFModel.train_step) of bench.py's model,
425 -> 512 -> 512 -> 187 on 32 utterances per step, with other hidden-layer activations than its Tanh: the
activation is fused into the GEMM epilogues (forward: act(z), backward: act'(y) through the stored output), so this
measures what the epilogue's arithmetic costs the step.  The configurations take turns round by round (the clock
drifts over a run); per configuration the median over rounds of the mean step time of a round.

Usage: python scripts/bench_ff_acts.py [--rounds R] [--steps K] [--acts Tanh,ELU,Sigmoid]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idiaptts_amd.bench_support import make_ff_batch  # noqa: E402
from idiaptts_amd.native_ff import FlatFFModel  # noqa: E402

DIMS = (425, 512, 512, 187)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--ramp-steps", type=int, default=100)
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--acts", default="Tanh,ELU,Sigmoid")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    names = args.acts.split(",")
    models = {n: FlatFFModel(DIMS, (n, n, None), device=dev, seed=0) for n in names}
    batches = []
    for b in range(4):
        x, y, lengths = make_ff_batch(args.utts, seed=1000 * b, device=dev)
        x = models[names[0]].pack_input(x)
        batches.append((x, y, torch.ones(x.shape[0], dtype=torch.uint8, device=dev), float(lengths.sum())))
    frames = sum(b[3] for b in batches) / len(batches)

    def run(model, n):
        for i in range(n):
            x, y, valid, nv = batches[i % len(batches)]
            model.train_step(x, y, valid, nv, lr=1e-3)

    times = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:
            run(models[n], args.ramp_steps)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            run(models[n], args.steps)
            b.record()
            b.synchronize()
            times[n].append(a.elapsed_time(b) / args.steps)
    out = {"model": "425 -> 512 (act) -> 512 (act) -> 187, flat train step", "valid_frames_per_step": frames,
           "ms_per_step_median": {n: sorted(t)[len(t) // 2] for n, t in times.items()},
           "ms_per_step_rounds": times}
    base = out["ms_per_step_median"][names[0]]
    out["ratio_to_" + names[0]] = {n: v / base for n, v in out["ms_per_step_median"].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
