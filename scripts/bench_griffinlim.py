"""Times the Griffin-Lim kernel (csrc/griffinlim.hip): world.griffinlim_batch's device work.

Workloads: the 256 synthetic 16 kHz utterances of scripts/bench_stft.py (n_fft 1024, hop 80) and a 32-utterance
48 kHz batch (n_fft 2048, hop 240); float32 spectra (|STFT| of the audio), seeded random phases, n_iter 32 and 60.
Per workload and n_iter: the device-event median of ops.griffinlim (the n_iter + 1 launches; the upload of the
spectra and phases is not timed), the time per launch (the median over n_iter + 1 launches, the last of which does
only the inverse half), and the paper model per iteration: state traffic of
36 B per bin (S, angles in and out, tprev in and out, float32 state) against the 6.29 TB/s copy rate, and fp64
FLOP (2.5 N log2 N per real transform of N points: the forward transform of every frame plus the inverse
transforms of the tile and its halo) against the 78.6 TFLOP/s vector peak.  A one-core numpy baseline of the
same definition (tests/griffinlim_spec.py's formulas, a few utterances, scaled to the batch) gives the speed-up.
For kernel-only times run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_griffinlim.py`.

Usage: python scripts/bench_griffinlim.py [--iters N] [--warmup W]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from idiaptts_amd import lib, ops, world  # noqa: E402
from idiaptts_amd.synthetic_audio import make_audio_batch  # noqa: E402

COPY_BW = 6.29e12           # B/s, measured copy rate
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


def _spectra(raws, n_fft, hop):
    win = world.stft_window(n_fft)
    out = []
    for r in raws:
        y = np.pad(r, n_fft // 2, mode="reflect")
        T = 1 + (len(y) - n_fft) // hop
        fr = y[np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]]
        out.append(np.abs(np.fft.rfft(fr * win, axis=1)).astype(np.float32))
    return out


def _numpy_s_per_frame_iter(spectra, n_fft, hop):
    """one core: one Griffin-Lim iteration (istft, overlap-add, normalisation, stft, phase update) per utterance"""
    win = world.stft_window(n_fft)
    n = 0
    t0 = time.perf_counter()
    for S in spectra:
        T = S.shape[0]
        ang = np.exp(2j * np.pi * np.random.RandomState(0).rand(T, S.shape[1])).astype(np.complex64)
        fr = np.fft.irfft(S * ang, n=n_fft, axis=1) * win
        y = np.zeros(n_fft + hop * (T - 1))
        for t in range(T):
            y[t * hop:t * hop + n_fft] += fr[t]
        wss = np.zeros_like(y)
        for t in range(T):
            wss[t * hop:t * hop + n_fft] += win ** 2
        nz = wss > np.finfo(np.float32).tiny
        y[nz] /= wss[nz]
        y = np.pad(y[n_fft // 2:len(y) - n_fft // 2], n_fft // 2, mode="reflect")
        reb = np.fft.rfft(y[np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]] * win, axis=1)
        a = reb.astype(np.complex64) - 0.99 / 1.99 * ang
        (a / (np.abs(a) + 1e-38)).astype(np.complex64)
        n += T
    return (time.perf_counter() - t0) / n


def bench(raws, fs, iters, warmup):
    n_fft = 1024 if fs < 40000 else 2048
    hop = world.stft_hop(fs, 5)
    dev = torch.device("cuda")
    spectra = _spectra(raws, n_fft, hop)
    f_off = world.offsets([s.shape[0] for s in spectra])
    T, K = f_off[-1], n_fft // 2 + 1
    F = lib.load().itts_griffinlim_tile_frames(n_fft, hop)
    h = -(-n_fft // hop) - 1
    n_inv = sum(min(t, f1 + h) - max(0, f0 - h)
                for t in (s.shape[0] for s in spectra)
                for k in range(-(-t // F))
                for f0, f1 in [(k * t // -(-t // F), (k + 1) * t // -(-t // F))])
    flop_iter = 2.5 * n_fft * math.log2(n_fft) * (T + n_inv)
    bytes_iter = 36.0 * T * K
    S = torch.from_numpy(np.concatenate(spectra)).to(dev)
    phases = np.concatenate(world.griffinlim_init_phases([s.shape for s in spectra], "random",
                                                         np.random.RandomState(0), np.complex64))
    ang0 = torch.from_numpy(np.ascontiguousarray(phases)).to(dev)
    win = torch.from_numpy(np.array(world.stft_window(n_fft))).to(dev)
    res = {"fs": fs, "utterances": len(raws), "frames": T, "n_fft": n_fft, "hop": hop, "tile_frames": F, "halo": h,
           "inverse_frames_per_iter": n_inv, "bytes_per_iter": bytes_iter, "fp64_flop_per_iter": flop_iter,
           "bound_ms_per_iter": {"memory": bytes_iter / COPY_BW * 1e3, "fp64": flop_iter / FP64_PEAK * 1e3}}
    angles = ang0.clone()
    for n_iter in (32, 60):
        ms = _median_ms(lambda: ops.griffinlim(S, angles.copy_(ang0), f_off, n_fft, hop, "reflect", win, n_iter,
                                               0.99), iters, warmup)
        per = ms / (n_iter + 1)
        bound = max(res["bound_ms_per_iter"].values())
        res["n_iter_{}".format(n_iter)] = {"ms": round(ms, 3), "ms_per_iter": round(per, 4),
                                           "GB_per_s": bytes_iter / per / 1e6,
                                           "fp64_TFLOP_per_s": flop_iter / per / 1e9,
                                           "fraction_of_bound": bound / per}
    sub = spectra[:4]
    np_s = _numpy_s_per_frame_iter(sub, n_fft, hop)
    res["numpy_one_core_ms_per_iter"] = np_s * T * 1e3
    res["speedup_vs_numpy_one_core"] = np_s * T * 1e3 / res["n_iter_60"]["ms_per_iter"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_griffinlim.py measures the GPU kernel: no HIP device visible")
    out = {"metric": "griffinlim",
           "gl_16k": bench(make_audio_batch(256, 16000, seed=0), 16000, args.iters, args.warmup),
           "gl_48k": bench(make_audio_batch(32, 48000, seed=1), 48000, args.iters, args.warmup)}
    for k in ("gl_16k", "gl_48k"):
        r = out[k]
        print("{}: {} frames, n_fft {}, hop {}, tile {} + 2 x {} halo; bounds per iteration: memory {:.3f} ms, "
              "fp64 {:.3f} ms".format(k, r["frames"], r["n_fft"], r["hop"], r["tile_frames"], r["halo"],
                                      r["bound_ms_per_iter"]["memory"], r["bound_ms_per_iter"]["fp64"]))
        for n in (32, 60):
            m = r["n_iter_{}".format(n)]
            print("  n_iter {:2d}: {:9.3f} ms  {:7.4f} ms/iter  {:7.1f} GB/s  {:6.2f} fp64 TFLOP/s  {:.3f} of bound"
                  .format(n, m["ms"], m["ms_per_iter"], m["GB_per_s"], m["fp64_TFLOP_per_s"], m["fraction_of_bound"]))
        print("  numpy one core: {:.1f} ms/iter, speed-up {:.0f}x".format(r["numpy_one_core_ms_per_iter"],
                                                                       r["speedup_vs_numpy_one_core"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
