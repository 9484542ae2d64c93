"""Times the vocoder's training path at the default WaveNetWrapper.Config (24 layers / 4 stacks, residual 512, gate 512,
skip 256, cin 80, 256 classes) on a synthetic corpus of 256 utterances of 6.6 s at 16 kHz (105 600 samples, 1 321
frames of 80 features each; 216 MB of samples and 108 MB of features on the device), B = 8, W = 8 000 and 16 000:

  kernel    (a) itts_vocoder_windows alone: median of 50 launches between HIP events, against its byte floor
            B W (mu + 1 + cin) 4 bytes written (172 MB at [8, 16 000]) over the 8.0 TB/s HBM3E peak; and the kernel's
            own time under `rocprofv3 --kernel-trace --stats`, in a run of its own (section kernel_prof)
  epoch     (b) ms per step of WaveNetVocoderTrainer.train over one epoch (32 steps), and
            (c) ms of the bare step -- forward, loss, backward, optimiser -- on one fixed batch in the same process
  readers   (d) ms to assemble one batch of the same windows on the stock reader path: RawWaveformLabelGen's
            whole-utterance one-hot to the host, sample_linearly of the whole conditioning, the cut to max_frames,
            prepare_batch, the transpose to [B, C, T] and the copy to the device

and reports (a) against its floor, (b) / (c) and (d) / (a).  Every section runs in a child process of its own under a
time limit; the first failure ends the run.  One JSON line.
Usage: python scripts/bench_vocoder_trainer.py [--utterances N] [--widths 8000,16000] [--section NAME]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM = 8.0e12
FS, FRAME_MS, M, CIN, MU, B = 16000, 5, 80, 80, 255, 8
N_SAMPLES = 105600                                    # 6.6 s
N_FRAMES = 1 + N_SAMPLES // M
SECTIONS = (("kernel", 300), ("kernel_prof", 300), ("epoch", 900), ("readers", 600))


def _signal(k):
    rng = np.random.default_rng(k)
    t = np.arange(N_SAMPLES) / FS
    x = 0.3 * np.sin(2 * np.pi * (110.0 + 3 * k) * t) * np.exp(-0.2 * t) + 0.02 * rng.standard_normal(N_SAMPLES)
    return np.round(np.clip(x, -1, 32767 / 32768) * 32768) / 32768


def _frames(k):
    return np.random.default_rng(1000 + k).standard_normal((N_FRAMES, CIN)).astype(np.float32)


def _readers():
    """the two readers of the trainer over the synthetic corpus, kept in memory: nothing is read from disk"""
    from idiaptts_amd.src.data_preparation.audio.RawWaveformLabelGen import RawWaveformLabelGen
    from idiaptts_amd.src.data_preparation.DataReaders import ReaderBase

    class Wave(RawWaveformLabelGen):
        def _file_path(self, file_path):
            return file_path

        def load(self, file_path):
            return _signal(int(file_path[1:]))

    class Frames(ReaderBase):
        def __init__(self, dir_labels=None, **kwargs):
            self._configure("mfbanks")

        def load(self, id_name):
            return _frames(int(id_name[1:]))

        def preprocess_sample(self, sample):
            return sample
    return Wave, Frames


def _trainer(args, W_sec, epochs):
    from idiaptts_amd.src.data_preparation.DataReaderConfig import DataReaderConfig
    from idiaptts_amd.src.model_trainers.WaveNetVocoderTrainer import WaveNetVocoderTrainer
    Wave, Frames = _readers()
    hp = WaveNetVocoderTrainer.create_hparams()
    hp.use_gpu, hp.out_dir, hp.model_name = True, tempfile.mkdtemp(prefix="bench_vocoder_"), "bench"
    hp.seed, hp.val_set_perc, hp.test_set_perc = 1, 1.0 / args.utterances, 0.0
    hp.batch_size_train, hp.batch_size_val, hp.epochs = B, B, epochs
    hp.max_input_train_sec, hp.max_input_test_sec = W_sec, W_sec
    hp.start_with_test, hp.log_memory_consumption, hp.save_final_model = False, False, False
    hp.optimiser_args = {"lr": 1e-3}
    hp.use_best_as_final_model, hp.epochs_per_test, hp.epochs_per_checkpoint = False, 1000, 1000
    configs = [DataReaderConfig(name="mfbanks", feature_type=Frames, output_names=["conditioning"]),
               DataReaderConfig(name="target", feature_type=Wave, frame_rate_output_Hz=FS, frame_size_ms=FRAME_MS,
                                mu=MU)]
    ids = ["u{}".format(k) for k in range(args.utterances + 1)]            # one of them is the validation set
    trainer = WaveNetVocoderTrainer(hp, ids, configs)
    trainer.init(hp)
    return trainer, hp


def _corpus(args):
    from idiaptts_amd.src.data_preparation.VocoderCorpus import VocoderCorpus
    Wave, Frames = _readers()
    wave = Wave(None, frame_rate_output_Hz=FS, frame_size_ms=FRAME_MS, mu=MU)
    wave._configure("target")
    frames = Frames()
    frames.output_names = ["conditioning"]
    return VocoderCorpus(wave, frames, ["u{}".format(k) for k in range(args.utterances)])


def _pairs(corpus, W, seed=0):
    from idiaptts_amd.src.data_preparation.VocoderCorpus import VocoderWindowSampler
    return VocoderWindowSampler(corpus, range(len(corpus)), W, seed=seed, batch_size=B).epoch_batches(0)[0]


def section_kernel(args, launches=50):
    import torch
    from idiaptts_amd import ops
    corpus = _corpus(args)
    res = {}
    for W in args.widths:
        rows, _ = corpus.window_rows(_pairs(corpus, W), W)
        target = torch.empty((B, MU + 1, W), dtype=torch.float32, device="cuda:0")
        cond = torch.empty((B, CIN, W), dtype=torch.float32, device="cuda:0")
        for _ in range(5):
            ops.vocoder_windows(corpus.d_x, corpus.d_feat, rows, W, M, MU, target=target, cond=cond)
        torch.cuda.synchronize()
        times = []
        for _ in range(launches):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            ops.vocoder_windows(corpus.d_x, corpus.d_feat, rows, W, M, MU, target=target, cond=cond)
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1))
        written = B * W * (MU + 1 + CIN) * 4
        ms = float(np.median(times))
        res[str(W)] = {"ms_median_of_{}".format(launches): round(ms, 4), "ms_min": round(min(times), 4),
                       "bytes_written": written, "floor_ms_at_peak": round(written / PEAK_HBM * 1e3, 4),
                       "fraction_of_hbm_peak": round(written / (ms * 1e-3) / PEAK_HBM, 3)}
    return res


def section_kernel_prof(args):
    """the kernel section again under rocprofv3, the profiler's own average of the kernel's time"""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"skipped": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="bench_vocoder_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "-d", out, "--output-format", "csv", "--", sys.executable,
           os.path.abspath(__file__), "--section", "kernel", "--utterances", str(args.utterances), "--widths",
           ",".join(str(w) for w in args.widths)]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=280)
    if child.returncode != 0:
        return {"failed": child.stdout[-400:]}
    res = {}
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                if "vocoder_windows_kernel" in row.get("Name", ""):
                    res = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                           "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2),
                           "note": "all widths of the kernel section together"}
    shutil.rmtree(out, ignore_errors=True)
    return res or {"failed": "no kernel_stats row for vocoder_windows_kernel"}


def section_epoch(args):
    import torch
    res = {}
    for W in args.widths:
        trainer, hp = _trainer(args, W / FS, epochs=1)
        steps = len(trainer.dataset_train.as_batch_loader(B, True))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trainer.train(hp)
        torch.cuda.synchronize()
        per_step = (time.perf_counter() - t0) * 1e3 / steps
        # (c) the bare step on one fixed batch, in the same process
        handler = trainer.model_handler
        data, lengths = trainer.corpus.batch(trainer.dataset_train.epoch_batches(0)[0], W)
        times = []
        for it in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            handler.process_batch(dict(data), dict(lengths), step=it, training=True, blocking=False)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        handler.finish_batches()
        bare = float(np.median(times[1:]))
        res[str(W)] = {"steps": steps, "trainer_ms_per_step": round(per_step, 2), "bare_step_ms": round(bare, 2),
                       "trainer_over_bare": round(per_step / bare, 4)}
        shutil.rmtree(hp.out_dir, ignore_errors=True)
        del trainer, handler, data
        torch.cuda.empty_cache()
    return res


def section_readers(args):
    """(d): the stock path for the windows of one batch"""
    import torch
    from idiaptts_amd.misc.utils import sample_linearly
    from idiaptts_amd.src.neural_networks.pytorch.ModularModelHandlerPyTorch import ModularModelHandlerPyTorch
    corpus = _corpus(argparse.Namespace(utterances=B, widths=args.widths))
    Wave, _ = _readers()
    wave = Wave(None, frame_rate_output_Hz=FS, frame_size_ms=FRAME_MS, mu=MU)
    wave._configure("target")
    res = {}
    for W in args.widths:
        pairs = _pairs(corpus, W)

        def assemble():
            items = []
            for s, a in pairs:
                onehot = wave.preprocess_sample(wave.load("u{}".format(s)))          # [N, 256] float32 on the host
                cond = sample_linearly(_frames(s), M)                                # [m T, 80] on the host
                items.append({"target": onehot[a:a + W], "conditioning": cond[a:a + W]})
            data, lengths = ModularModelHandlerPyTorch.prepare_batch(items, batch_first=True,
                                                                     mask_keys=("target",))
            out = {k: (v.transpose(1, 2).contiguous() if k != "target_mask" else v[:, 1:].contiguous()).to("cuda:0")
                   for k, v in data.items()}
            torch.cuda.synchronize()
            return out
        assemble()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            assemble()
            times.append((time.perf_counter() - t0) * 1e3)
        res[str(W)] = {"ms_per_batch": round(float(np.median(times)), 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--widths", default="8000,16000")
    ap.add_argument("--section", default=None)
    args = ap.parse_args()
    args.widths = [int(w) for w in args.widths.split(",")]
    if args.section:
        fn = {"kernel": section_kernel, "kernel_prof": section_kernel_prof, "epoch": section_epoch,
              "readers": section_readers}[args.section]
        print(json.dumps(fn(args)))
        return 0
    res = {"corpus": {"utterances": args.utterances, "samples_each": N_SAMPLES, "frames_each": N_FRAMES, "cin": CIN,
                      "mu": MU, "B": B}}
    for name, limit in SECTIONS:                         # a fresh process per section, each under its own time limit
        try:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--section", name] + sys.argv[1:],
                                   stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            res[name] = "time limit of {} s".format(limit)
            print(json.dumps(res))
            return 1
        if child.returncode != 0:
            res[name] = "exit status {}".format(child.returncode)
            print(json.dumps(res))
            return 1
        res[name] = json.loads(child.stdout.strip().splitlines()[-1])
        print(name, json.dumps(res[name]), file=sys.stderr, flush=True)
    for W in args.widths:
        a, d = res["kernel"][str(W)], res["readers"][str(W)]
        d["readers_over_kernel"] = round(d["ms_per_batch"] / a["ms_median_of_50"], 1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
