"""Times the corpus audio preparation (csrc/audio_prep.hip, src/data_preparation/audio): the reference's four steps
in front of gen_data -- down_sampling, silence_remove, normalize_loudness, high_pass_filter -- on 256 synthetic
utterances (synthetic_audio.make_audio, 6.5625 s = 105 000 samples) at 16 kHz and 32 at 48 kHz.  It reports
  * the time of each step's kernels on the batch already on the device (median of device-event times after a
    warm-up), with the step's multiply-add and byte counts and the share of the bound they give: the fp64 vector peak
    for the filter and the resampler, the HBM peak for loudness and frame RMS;
  * the whole process_list of each class, wav files in, wav files out into an empty directory, file I/O included;
  * scipy / numpy on one core on the same inputs: scipy.signal.filtfilt, scipy.signal.resample_poly, the loudness
    lines of the reference and a strided-window frame RMS (what librosa.feature.rms computes).
One JSON line at the end.

Usage: python scripts/bench_audio_prep.py [--iters 10] [--warmup 2] [--utts16 256] [--utts48 32] [--no-scipy]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import scipy.signal
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idiaptts_amd import ops, synthetic_audio  # noqa: E402
from idiaptts_amd.src.data_preparation.audio import audio_batch, down_sampling  # noqa: E402
from idiaptts_amd.src.data_preparation.audio.AudioProcessing import AudioProcessing  # noqa: E402
from idiaptts_amd.src.data_preparation.audio.high_pass_filter import HighPassFilter  # noqa: E402
from idiaptts_amd.src.data_preparation.audio.normalize_loudness import LoudnessNormalizer  # noqa: E402
from idiaptts_amd.src.data_preparation.audio.silence_remove import SilenceRemover  # noqa: E402

PEAK_FP64 = 78.6e12     # flop / s, vector fp64
PEAK_HBM = 8.0e12       # bytes / s
SECONDS = 6.5625
NUMTAPS = 1001


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
    times.sort()
    return times[len(times) // 2]


def _wall(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def _entry(ms, flops, nbytes):
    out = {"kernel_ms": round(ms, 4), "gflop": round(flops / 1e9, 3), "mbytes": round(nbytes / 1e6, 2)}
    t_flop, t_byte = flops / PEAK_FP64 * 1e3, nbytes / PEAK_HBM * 1e3
    out["bound_ms"] = round(max(t_flop, t_byte), 4)
    out["bound_by"] = "fp64" if t_flop > t_byte else "hbm"
    out["share_of_bound"] = round(max(t_flop, t_byte) / ms, 3)
    return out


def kernels(signals, fs, target, iters, warmup):
    dev = torch.device("cuda")
    n_sig = len(signals)
    off = np.concatenate([[0], np.cumsum([len(s) for s in signals])]).astype(np.int64)
    total = int(off[-1])
    x = torch.from_numpy(np.concatenate(signals)).to(dev)
    res = {}
    taps = torch.from_numpy(HighPassFilter().filter_coefs(fs)).to(dev)
    pad = 3 * NUMTAPS
    # two passes of numtaps multiply-adds over n + padlen and n outputs; x in, the first pass out and in, y out
    res["filtfilt"] = _entry(_median_ms(lambda: ops.fir_filtfilt(x, off, taps), iters, warmup),
                             2.0 * NUMTAPS * (2 * total + n_sig * pad), 8.0 * (4 * total + 2 * n_sig * pad))
    # three reductions and the scaling read x, the last writes y
    res["loudness"] = _entry(_median_ms(lambda: ops.loudness_normalise(x, off, 0.1), iters, warmup), 7.0 * total,
                             8.0 * 5 * total)
    frame_length = AudioProcessing.fs_to_frame_length(fs)
    hop = int(fs / 1000 * 32)
    frames = ops.frame_rms_offsets(off, frame_length, hop)[-1]
    # every frame squares and sums frame_length samples; the samples are fetched from memory once
    res["frame_rms"] = _entry(_median_ms(lambda: ops.frame_rms(x, off, frame_length, hop), iters, warmup),
                              2.0 * frame_length * frames, 8.0 * (total + frames))
    if target != fs:
        up, down = down_sampling.resample_ratio(fs, target)
        rtaps = torch.from_numpy(down_sampling.resample_filter(up, down)).to(dev)
        n_out = ops.resample_out_offsets(off, up, down)[-1]
        per_out = -(-rtaps.numel() // up)
        res["resample_{}_to_{}".format(fs, target)] = _entry(
            _median_ms(lambda: ops.resample_poly(x, off, up, down, rtaps), iters, warmup), 2.0 * per_out * n_out,
            8.0 * (total + n_out))
    return res


def files(signals, fs, target):
    """process_list of each class, one run each, into empty directories"""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "wav")
        os.makedirs(src)
        ids = ["utt{:04d}".format(i) for i in range(len(signals))]
        for i, s in zip(ids, signals):
            audio_batch.write_pcm16(os.path.join(src, i + ".wav"), s, fs)
        runs = [("high_pass_filter", lambda d: HighPassFilter().process_list(ids, src, d)),
                ("normalize_loudness", lambda d: LoudnessNormalizer().process_list(ids, src, d)),
                ("silence_remove", lambda d: SilenceRemover().process_list(ids, src, d))]
        if target != fs:
            runs.append(("down_sampling", lambda d: down_sampling.downsample_list(ids, src, d, target)))
        for name, run in runs:
            out = os.path.join(tmp, name)
            stdout, sys.stdout = sys.stdout, open(os.devnull, "w")
            try:
                res[name + "_s"] = round(_wall(lambda: run(out)), 4)
            finally:
                sys.stdout.close()
                sys.stdout = stdout
            assert len(os.listdir(out)) == len(ids)
    return res


def one_core(signals, fs, target):
    torch.set_num_threads(1)
    b = HighPassFilter().filter_coefs(fs)
    frame_length = AudioProcessing.fs_to_frame_length(fs)
    hop = int(fs / 1000 * 32)

    def loudness():
        for s in signals:
            raw = s - s.mean()
            raw *= np.sqrt(len(raw) * 0.1 ** 2 / (raw ** 2).sum())

    def frame_rms():
        for s in signals:
            padded = np.pad(s, frame_length // 2)
            windows = np.lib.stride_tricks.sliding_window_view(padded, frame_length)[::hop]
            np.sqrt(np.mean(np.abs(windows) ** 2, axis=-1))

    res = {"filtfilt_s": round(_wall(lambda: [scipy.signal.filtfilt(b, [1], s) for s in signals]), 3),
           "loudness_s": round(_wall(loudness), 4), "frame_rms_s": round(_wall(frame_rms), 4)}
    if target != fs:
        res["resample_poly_s"] = round(_wall(lambda: [scipy.signal.resample_poly(s, target, fs) for s in signals]), 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--utts16", type=int, default=256)
    ap.add_argument("--utts48", type=int, default=32)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    result = {"seconds_per_utterance": SECONDS, "numtaps": NUMTAPS, "device": torch.cuda.get_device_name(0)}
    for fs, n_utts in ((16000, args.utts16), (48000, args.utts48)):
        signals = [synthetic_audio.make_audio(fs, SECONDS, i) for i in range(n_utts)]
        entry = {"utterances": n_utts, "samples": int(sum(len(s) for s in signals)),
                 "kernels": kernels(signals, fs, 16000, args.iters, args.warmup),
                 "process_list": files(signals, fs, 16000)}
        if not args.no_scipy:
            entry["one_core"] = one_core(signals, fs, 16000)
        result["fs_{}".format(fs)] = entry
        print("fs {}: {}".format(fs, json.dumps(entry)), file=sys.stderr)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
