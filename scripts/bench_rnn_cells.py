"""Forward + backward of ONE bidirectional recurrent layer per cell type on the step kernels: vanilla RNN (tanh), GRU and
LSTM at H = 256 and 512 on a batch of 64 LJSpeech-like utterances (2-10 s at 5 ms frames, zero-padded, 425 inputs).
Only the public idiaptts_amd.nn classes are used, so the same file times an older checkout of the package:

    python scripts/bench_rnn_cells.py [--package-root DIR] [--rounds 5] [--cells RNN,GRU,LSTM] [--sizes 256,512]

ITTS_RNN_PERSISTENT=0 keeps LSTM and GRU off their persistent kernels (and off the padding to 512 that goes with
them): every cell runs one launch per time step, which is what the comparison is about.  Method: every configuration
is warmed up, then the configurations are timed in turn, `rounds` times over (alternating, so that drift of the
machine hits all alike), each timing a window of device events around enough calls to last ~0.5 s and ending in a
synchronise; per configuration the median over the rounds and the spread (min .. max) are printed, one JSON line
each, then the ratios RNN / GRU and RNN / LSTM at each size."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

os.environ["ITTS_RNN_PERSISTENT"] = "0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cells", default="RNN,GRU,LSTM")
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--window-s", type=float, default=0.5)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch
    from idiaptts_amd import nn as inn

    if not torch.cuda.is_available():
        sys.exit("bench_rnn_cells: no GPU visible; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    in_dim = 425
    lengths = np.rint(200.0 * np.random.default_rng(1234 + 7).uniform(2.0, 10.0, size=args.utterances)).astype(np.int64)
    T, B = int(lengths.max()), len(lengths)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(T, B, in_dim, generator=gen)
    x[torch.arange(T)[:, None] >= torch.as_tensor(lengths)[None, :]] = 0.0
    x = x.to(dev).requires_grad_(True)
    lens = torch.as_tensor(lengths)
    print(json.dumps({"frames": int(lengths.sum()), "T": T, "B": B, "in_dim": in_dim,
                      "package": os.path.dirname(inn.__file__)}), flush=True)

    configs = []
    for H in [int(v) for v in args.sizes.split(",")]:
        for cell in args.cells.split(","):
            torch.manual_seed(0)
            layer = getattr(inn, cell)(in_dim, H, 1, bidirectional=True).to(dev)
            w = torch.randn(T, B, 2 * H, generator=gen).to(dev)
            configs.append({"cell": cell, "H": H, "layer": layer, "w": w, "ms": []})

    def call(c):
        out, _ = c["layer"](x, None, lens)
        (out * c["w"]).sum().backward()
        return out

    def window(c, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call(c)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    for c in configs:
        call(c)
        torch.cuda.synchronize()
        c["calls"] = max(2, int(round(args.window_s * 1e3 / window(c, 1))))
        c["checksum"] = float(call(c).detach().double().abs().sum())
    for _ in range(args.rounds):
        for c in configs:
            c["ms"].append(window(c, c["calls"]))
    med = {}
    for c in configs:
        med[(c["cell"], c["H"])] = statistics.median(c["ms"])
        print(json.dumps({"cell": c["cell"], "H": c["H"], "fwd_bwd_ms_median": round(med[(c["cell"], c["H"])], 3),
                          "min": round(min(c["ms"]), 3), "max": round(max(c["ms"]), 3), "rounds": args.rounds,
                          "calls_per_window": c["calls"], "abs_sum_out": c["checksum"]}), flush=True)
    for (cell, H), v in med.items():
        if cell == "RNN":
            print(json.dumps({"H": H, **{"RNN_over_" + o: round(v / med[(o, H)], 3) for o in ("GRU", "LSTM")
                                         if (o, H) in med}}), flush=True)


if __name__ == "__main__":
    main()
