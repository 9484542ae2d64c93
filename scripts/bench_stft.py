"""Times the STFT feature kernel (csrc/stft.hip) and gen_data on STFT features.

Workloads: 256 synthetic 16 kHz utterances (synthetic_audio.make_audio_batch, 2-10 s) and a 32-utterance 48 kHz batch.
Per workload: device-event medians of world.stft_features in its three modes (amp_sp, log_amp_sp, mfbanks 80), with
frames/s, bytes/s (samples read once + rows written) and fp64 FLOP/s (2.5 N log2 N per real transform of N points,
the window and magnitudes not counted) computed from shapes; a one-core numpy baseline of the same definition
(tests/stft_spec.py's formulas, a subset of utterances, scaled to frames/s).  Then gen_data(sp_type="mfbanks")
against gen_data(sp_type="mcep") on the same 256 files (host clock, median of three passes after a warm-up).
For kernel-only times run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_stft.py`.

Usage: python scripts/bench_stft.py [--iters N] [--warmup W] [--no-gen-data]"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from idiaptts_amd import world  # noqa: E402
from idiaptts_amd.synthetic_audio import make_audio_batch  # noqa: E402


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


def _numpy_frames_per_s(raws, n_fft, hop, n_mels, fs):
    """one core, float64: frame, window, rfft, |.| / sqrt(K), mel projection"""
    win = world.stft_window(n_fft)
    basis = world.mel_basis(fs, n_fft, n_mels).astype(np.float64)
    t0 = time.perf_counter()
    n = 0
    for r in raws:
        y = np.pad(r, n_fft // 2, mode="reflect")
        T = 1 + (len(y) - n_fft) // hop
        fr = y[np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]]
        amp = np.abs(np.fft.rfft(fr * win, axis=1)) / np.sqrt(n_fft // 2 + 1)
        (basis @ amp.T).T.astype(np.float32)
        n += T
    return n / (time.perf_counter() - t0)


def bench_kernel(raws, fs, iters, warmup):
    n_fft = world.fs_to_frame_length(fs)
    hop = world.stft_hop(fs, 5)
    dev = torch.device("cuda")
    x_off = world.offsets([len(r) for r in raws])
    f_off = world.offsets([world.stft_num_frames(len(r), n_fft, hop) for r in raws])
    x = torch.from_numpy(np.concatenate(raws)).to(dev)
    T, K = f_off[-1], n_fft // 2 + 1
    flop = T * 2.5 * n_fft * math.log2(n_fft)
    res = {"fs": fs, "utterances": len(raws), "frames": T, "n_fft": n_fft, "hop": hop,
           "audio_s": x_off[-1] / fs, "fp64_flop_per_launch": flop}
    for mode, width, nbytes in (("amp_sp", K, 4), ("log_amp_sp", K, 4), ("mfbanks", 80, 4)):
        out = torch.empty((T, width), dtype=torch.float32, device=dev)
        ms = _median_ms(lambda: world.stft_features(x, x_off, f_off, [0] * len(raws), fs, mode, n_fft, hop,
                                                    n_mels=80, out=out), iters, warmup)
        moved = x_off[-1] * 8 + T * width * nbytes
        res[mode] = {"ms": round(ms, 4), "frames_per_s": T / ms * 1e3, "GB_per_s": moved / ms / 1e6,
                     "fp64_TFLOP_per_s": flop / ms / 1e9, "bytes": moved}
    sub = raws[:8]
    res["numpy_one_core_frames_per_s"] = _numpy_frames_per_s(sub, n_fft, hop, 80, fs)
    return res


def bench_gen_data(raws, fs):
    from scipy.io import wavfile
    from idiaptts_amd.src.data_preparation.world.WorldFeatLabelGen import WorldFeatLabelGen
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        wav_dir = os.path.join(tmp, "wav")
        os.makedirs(wav_dir)
        ids = ["utt{:04d}".format(i) for i in range(len(raws))]
        for n, r in zip(ids, raws):
            wavfile.write(os.path.join(wav_dir, n + ".wav"), fs, np.round(np.clip(r, -1, 1) * 32767).astype(np.int16))
        for sp_type, ncs in (("mfbanks", 80), ("mcep", 60), ("mfbanks", 80), ("mcep", 60)):
            gen = WorldFeatLabelGen(os.path.join(tmp, sp_type), add_deltas=True, num_coded_sps=ncs, sp_type=sp_type)
            times = []
            for _ in range(4):                  # the first pass warms the device tables up
                t0 = time.perf_counter()
                gen.gen_data(wav_dir, os.path.join(tmp, sp_type), "ids.txt", id_list=ids)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            res.setdefault(sp_type, []).append(float(np.median(times[1:])))
    return {k: {"ms_runs": v, "ms": min(v)} for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-gen-data", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stft.py measures the GPU kernel: no HIP device visible")
    raws16 = make_audio_batch(256, 16000, seed=0)
    raws48 = make_audio_batch(32, 48000, seed=1)
    out = {"metric": "stft_features", "kernel_16k": bench_kernel(raws16, 16000, args.iters, args.warmup),
           "kernel_48k": bench_kernel(raws48, 48000, args.iters, args.warmup)}
    if not args.no_gen_data:
        out["gen_data_16k_256utts_deltas"] = bench_gen_data(raws16, 16000)
    for k in ("kernel_16k", "kernel_48k"):
        r = out[k]
        print("{}: {} frames ({:.0f} s audio), n_fft {}".format(k, r["frames"], r["audio_s"], r["n_fft"]))
        for mode in ("amp_sp", "log_amp_sp", "mfbanks"):
            m = r[mode]
            print("  {:10s} {:8.3f} ms  {:7.1f} M frames/s  {:7.1f} GB/s  {:6.2f} fp64 TFLOP/s".format(
                mode, m["ms"], m["frames_per_s"] / 1e6, m["GB_per_s"], m["fp64_TFLOP_per_s"]))
        print("  numpy one core: {:.3f} M frames/s".format(r["numpy_one_core_frames_per_s"] / 1e6))
    if "gen_data_16k_256utts_deltas" in out:
        g = out["gen_data_16k_256utts_deltas"]
        print("gen_data 256 utts: mfbanks80 {:.1f} ms, mcep60 {:.1f} ms".format(g["mfbanks"]["ms"], g["mcep"]["ms"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
