"""Times the mel filter-bank inversion kernel (csrc/mel_inverse.hip): world.mel_inverse's device work.

Workloads: the mel filter banks (80 bands, float32, from the STFT kernel) of the 256 synthetic 16 kHz utterances of
scripts/bench_stft.py (n_fft 1024) and of a 32-utterance 48 kHz batch (n_fft 2048), all frames of a workload in one
launch.  Per workload: the device-event median of world.mel_inverse (the upload of the bands is not timed), frames/s,
the iterations the frames took (mean and max), and the paper model: 4 K fp64 FMA per iteration (A y and A^T r over
about 2 K nonzeros; the stopping tests add one iteration in CHECK) plus K n_mels FMA for the start, against the
78.6 TFLOP/s vector peak.  A one-core baseline of scipy.optimize.nnls (the exact solver) on a few frames, scaled to
the batch, gives the speed-up.  For kernel-only times run it under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_mel_inverse.py`.

Usage: python scripts/bench_mel_inverse.py [--iters N] [--warmup W]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from idiaptts_amd import world  # noqa: E402
from idiaptts_amd.synthetic_audio import make_audio_batch  # noqa: E402

FP64_PEAK = 78.6e12         # FLOP/s, fp64 vector peak


def _median_ms(fn, iters, warmup):
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
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def _bands(raws, fs, n_fft, n_mels, dev):
    hop = world.stft_hop(fs, 5)
    lens = [len(r) for r in raws]
    T = [world.stft_num_frames(n, n_fft, hop) for n in lens]
    x = torch.from_numpy(np.concatenate(raws).astype(np.float64)).to(dev)
    mel = world.stft_features(x, world.offsets(lens), world.offsets(T), [0] * len(raws), fs, "mfbanks", n_fft, hop,
                              n_mels=n_mels)
    torch.cuda.synchronize()
    return mel


def _scipy_s_per_frame(mel, fs, n_fft, n_frames=8):
    import scipy.optimize
    A = world.mel_basis_plain(fs, n_fft, mel.shape[1], np.float32).astype(np.float64)
    rows = mel[np.linspace(0, len(mel) - 1, n_frames).astype(int)].astype(np.float64)
    t0 = time.perf_counter()
    for b in rows:
        scipy.optimize.nnls(A, b)
    return (time.perf_counter() - t0) / n_frames


def bench(raws, fs, iters, warmup, n_mels=80):
    n_fft = 1024 if fs < 40000 else 2048
    K = n_fft // 2 + 1
    dev = torch.device("cuda")
    mel = _bands(raws, fs, n_fft, n_mels, dev)
    F = mel.shape[0]
    _, it = world.mel_inverse(mel, fs, n_fft, return_iters=True)
    it = it.cpu().numpy().astype(np.int64)
    checks = it // world.MEL_INVERSE_CHECK
    flop = 2.0 * (4 * K * (it.sum() + checks.sum()) + K * n_mels * F)
    ms = _median_ms(lambda: world.mel_inverse(mel, fs, n_fft), iters, warmup)
    res = {"fs": fs, "utterances": len(raws), "frames": F, "n_fft": n_fft, "n_mels": n_mels,
           "iterations_mean": float(it.mean()), "iterations_max": int(it.max()),
           "frames_at_cap": int((it >= world.MEL_INVERSE_CAP).sum()),
           "fp64_flop": float(flop), "fp64_bound_ms": flop / FP64_PEAK * 1e3,
           "ms": round(ms, 3), "frames_per_s": F / ms * 1e3, "fp64_TFLOP_per_s": flop / ms / 1e9}
    res["fraction_of_fp64_bound"] = res["fp64_bound_ms"] / ms
    s = _scipy_s_per_frame(mel.cpu().numpy(), fs, n_fft)
    res["scipy_nnls_one_core_s_per_frame"] = s
    res["scipy_nnls_one_core_s"] = s * F
    res["speedup_vs_scipy_one_core"] = s * F * 1e3 / ms
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mel_inverse.py measures the GPU kernel: no HIP device visible")
    out = {"metric": "mel_inverse",
           "mi_16k": bench(make_audio_batch(256, 16000, seed=0), 16000, args.iters, args.warmup),
           "mi_48k": bench(make_audio_batch(32, 48000, seed=1), 48000, args.iters, args.warmup)}
    for k in ("mi_16k", "mi_48k"):
        r = out[k]
        print("{}: {} frames, n_fft {}, {} bands; iterations mean {:.1f}, max {}, {} at the cap".format(
            k, r["frames"], r["n_fft"], r["n_mels"], r["iterations_mean"], r["iterations_max"], r["frames_at_cap"]))
        print("  {:9.3f} ms  {:.3g} frames/s  {:.2f} fp64 TFLOP/s  ({:.3f} ms fp64 bound, {:.3f} of it)".format(
            r["ms"], r["frames_per_s"], r["fp64_TFLOP_per_s"], r["fp64_bound_ms"], r["fraction_of_fp64_bound"]))
        print("  scipy nnls one core: {:.1f} ms/frame, {:.0f} s for the batch, speed-up {:.0f}x".format(
            r["scipy_nnls_one_core_s_per_frame"] * 1e3, r["scipy_nnls_one_core_s"], r["speedup_vs_scipy_one_core"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
