"""The training data of the sample-level vocoder as a device-resident store, and the sampler that cuts batches of
windows out of it with one kernel launch (ops.vocoder_windows, csrc/vocoder_batch.hip).

The stock reader path hands a whole utterance's [T, mu + 1] one-hot through the host (108 MB for 6.6 s at 16 kHz, mu
255) before `max_frames` cuts a window out of it; what a batch needs is a pure function of the samples, the frame-rate
conditioning and B pairs (utterance, start).  So the store keeps, per utterance s,
    x_s   float64 [N_s]        RawWaveformLabelGen.load_sample
    F_s   float32 [T_s, cin]   the conditioning reader's output after its normalisation, T_s >= 2
back to back in two device tensors, and five numbers: the sample offset, the usable range [lo_s, hi_s), the first
frame row and T_s.  With m = int(frame_rate_output_Hz / (1000 / frame_size_ms)) the conditioning at the sample rate is
U_s = sample_linearly(F_s, m), m T_s rows, never stored: sample i pairs with U_s[i] (alignment at the front), so
    lo_s = 0,  hi_s = min(N_s, m T_s);
with `silence_threshold_quantized` and a mu, (start, end) = RawWaveformLabelGen.start_and_end_indices of the
utterance's classes, computed once here, gives
    lo_s = start,  hi_s = min(end, m T_s):
samples and conditioning are trimmed together (the reference trims the samples alone, which shifts them against the
conditioning by `start`).  Without mu the threshold is ignored, as the reader ignores it.

A window (s, a, W) has len = min(W, hi_s - a) live columns and zeros behind them.  The sampler draws one window per
utterance and epoch -- training: a = lo_s + randint(0, max(1, (hi_s - lo_s) - W)), the rule of
PyTorchDatareadersDataset._match_max_frames; validation / test: a = lo_s, the same every epoch -- from a
torch.Generator of its own seeded with (seed, epoch): the same seed gives the same windows on any machine and torch's
global generator is not touched.  Batches are (data, lengths) pairs already on the device, which
ModularModelHandlerPyTorch.process_dataloader iterates as they are: no DeviceBatchCache, no threaded loader, no
resident_dataset path."""
import logging
import os

import numpy as np
import torch

from idiaptts_amd.src.data_preparation.audio.RawWaveformLabelGen import RawWaveformLabelGen


def in_to_out_multiplier(frame_rate_output_Hz, frame_size_ms):
    """samples per conditioning frame, as the reference's trainer computes it"""
    return int(frame_rate_output_Hz / (1000.0 / frame_size_ms))


def window_length(seconds, frame_size_ms, m):
    """W = int(frames per second * seconds) * m: whole frames"""
    return int(1000.0 / frame_size_ms * seconds) * m


def usable_range(n_samples, n_frames, m, trim=None):
    """[lo, hi) of an utterance with n_samples samples and n_frames conditioning frames (None: no conditioning);
    trim = (start, end) of the silence trim"""
    lo, hi = (0, n_samples) if trim is None else (int(trim[0]), int(trim[1]))
    if n_frames is not None:
        hi = min(hi, m * n_frames)
    return lo, hi


def _device_classes(x, mu):
    return RawWaveformLabelGen.mu_law_companding(x, mu)


class VocoderCorpus(object):
    """The store.  `wave_reader`: a RawWaveformLabelGen (its mu, silence_threshold_quantized, frame_rate_output_Hz and
    frame_size_ms apply); `cond_reader`: the conditioning reader, or None for a network without conditioning.
    Everything is loaded and checked before anything is written to the device; a refusal names the file.
    `encode(x, mu)`: the class indices for the silence trim (default: the device companding the reader uses);
    `upload=False` keeps the store on the host (tables and checks only)."""

    logger = logging.getLogger(__name__)
    FIELDS = ("sample_offset", "lo", "hi", "frame_row", "T")

    def __init__(self, wave_reader, cond_reader, id_list, device=None, upload=True, encode=None):
        self.id_list = list(id_list)
        self.mu = wave_reader.mu
        self.m = in_to_out_multiplier(wave_reader.frame_rate_output_Hz, wave_reader.frame_size_ms)
        if self.m < 1:
            raise ValueError("frame_rate_output_Hz = {} and frame_size_ms = {} give {} samples a frame.".format(
                wave_reader.frame_rate_output_Hz, wave_reader.frame_size_ms, self.m))
        self.target_name = wave_reader.output_names[0]
        self.cond_name = cond_reader.output_names[0] if cond_reader is not None else None
        threshold = wave_reader.silence_threshold_quantized if self.mu is not None else None
        encode = _device_classes if encode is None else encode
        signals, feats, table = [], [], []
        n_x = n_rows = 0
        self.cin = 0
        for id_name in self.id_list:
            path = wave_reader._file_path(id_name)
            x = np.ascontiguousarray(wave_reader.load(id_name), dtype=np.float64)   # (rate, channels: the reader's)
            T = None
            if cond_reader is not None:
                F = np.ascontiguousarray(cond_reader[id_name][self.cond_name], dtype=np.float32)
                if F.ndim != 2:
                    raise ValueError("{}: the conditioning of {} is {}-dimensional, not [T, cin].".format(
                        cond_reader.name, id_name, F.ndim))
                T = F.shape[0]
                if T < 2:
                    raise ValueError("{} has {} conditioning frame(s) ({}): linear interpolation needs at least 2."
                                     .format(id_name, T, path))
                if feats and F.shape[1] != self.cin:
                    raise ValueError("{} has {} conditioning features, the utterances before it {}.".format(
                        id_name, F.shape[1], self.cin))
                self.cin = F.shape[1]
                feats.append(F)
            trim = None
            if threshold is not None:
                try:
                    trim = RawWaveformLabelGen.start_and_end_indices(encode(x, self.mu), threshold)
                except AssertionError as e:
                    raise ValueError("{} has an empty usable range: {} (silence_threshold_quantized = {}).".format(
                        path, e, threshold))
            lo, hi = usable_range(len(x), T, self.m, trim)
            if hi - lo < 1:
                raise ValueError("{} has an empty usable range [{}, {}): {} samples, {} frames of {} samples{}."
                                 .format(path, lo, hi, len(x), T, self.m,
                                         "" if trim is None else ", silence trim {}".format(trim)))
            table.append((n_x, lo, hi, n_rows, 0 if T is None else T))
            signals.append(x)
            n_x += len(x)
            n_rows += 0 if T is None else T
        self.table = np.array(table, dtype=np.int64).reshape(-1, len(self.FIELDS))
        self.n_samples, self.n_rows = n_x, n_rows
        self.nbytes = 8 * n_x + 4 * n_rows * self.cin
        self.d_x = self.d_feat = None
        if upload:
            from idiaptts_amd import lib
            lib.require_gpu()
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            self.d_x = torch.from_numpy(np.concatenate(signals) if signals else np.zeros(0)).to(device)
            if self.cin > 0:
                self.d_feat = torch.from_numpy(np.concatenate(feats, axis=0)).to(device)
        self.logger.info("Vocoder corpus: {} utterances, {} samples, {} frames of {} features: {} bytes{}.".format(
            len(self.id_list), n_x, n_rows, self.cin, self.nbytes, " on " + str(device) if upload else " (host only)"))

    def __len__(self):
        return len(self.id_list)

    def index(self, id_name):
        return self.id_list.index(id_name)

    def window_rows(self, pairs, W):
        """host int64 [B, 5] for ops.vocoder_windows and the B lengths, of (utterance index, start) pairs"""
        rows = np.empty((len(pairs), 5), dtype=np.int64)
        for b, (s, a) in enumerate(pairs):
            off, lo, hi, row, T = self.table[s]
            if not lo <= a < hi:
                raise ValueError("Window start {} lies outside the usable range [{}, {}) of {}.".format(
                    a, lo, hi, self.id_list[s]))
            rows[b] = (off + a, min(W, hi - a), row, T, a)
        return rows, rows[:, 1].copy()

    def batch(self, pairs, W):
        """(data, lengths) of the windows, on the device: data[target] [B, C, W], data[conditioning] [B, cin, W]
        (absent without conditioning) and data[target + "_mask"] [B, W - 1, 1], the sequence mask without its first
        column: with shift=1 the losses score input column t against target column t + 1 and return W - 1 columns.
        lengths of the mask: len - 1, the scored columns."""
        from idiaptts_amd import ops
        if self.d_x is None:
            raise RuntimeError("The corpus was built with upload=False: it has no device tensors.")
        rows, lens = self.window_rows(pairs, W)
        target, cond = ops.vocoder_windows(self.d_x, self.d_feat, rows, W, self.m, self.mu)
        lens = torch.from_numpy(lens)
        scored = (lens - 1).to(target.device, non_blocking=True)
        mask = (torch.arange(W - 1, device=target.device)[None, :] < scored[:, None]).unsqueeze(-1).float()
        data = {self.target_name: target, self.target_name + "_mask": mask,
                "_id_list": [self.id_list[s] for s, _ in pairs]}
        lengths = {self.target_name: lens, self.target_name + "_mask": lens - 1}
        if cond is not None:
            data[self.cond_name] = cond
            lengths[self.cond_name] = lens
        return data, lengths


class VocoderWindowSampler(object):
    """One window per utterance and epoch over `utterances` (indices into the corpus), in batches.  What the trainer
    hands to the model handler in place of a dataset: `as_batch_loader` is the hook
    ModularModelHandlerPyTorch._get_dataloader looks for, and iterating yields (data, lengths) on the device.
    `epoch` counts the finished passes of a training sampler; set it when training continues from a checkpoint."""

    def __init__(self, corpus, utterances, W, seed=None, training=True, batch_size=1, shuffle=True):
        self.corpus = corpus
        self.utterances = [int(s) for s in utterances]
        self.W = int(W)
        if self.W < 1:
            raise ValueError("Window length W = {} is not positive.".format(W))
        # (without a seed: one drawn here, from the system, not from torch's global generator)
        self.seed = int.from_bytes(os.urandom(4), "little") if seed is None else int(seed)
        self.training = bool(training)
        self.batch_size, self.shuffle = int(batch_size), bool(shuffle)
        self.epoch = 0

    def as_batch_loader(self, batch_size, shuffle):
        self.batch_size, self.shuffle = int(batch_size), bool(shuffle)
        return self

    def epoch_windows(self, epoch):
        """the (utterance, start) pairs of an epoch in the order they are batched: a pure function of seed and epoch"""
        g = torch.Generator()
        g.manual_seed((self.seed * 1000003 + int(epoch)) % (2 ** 63))
        n = len(self.utterances)
        order = torch.randperm(n, generator=g).tolist() if self.shuffle else list(range(n))
        pairs = []
        for i in order:
            s = self.utterances[i]
            lo, hi = int(self.corpus.table[s, 1]), int(self.corpus.table[s, 2])
            a = lo
            if self.training:
                a += int(torch.randint(0, max(1, (hi - lo) - self.W), (1,), generator=g))
            pairs.append((s, a))
        return pairs

    def epoch_batches(self, epoch):
        pairs = self.epoch_windows(epoch)
        return [pairs[i:i + self.batch_size] for i in range(0, len(pairs), self.batch_size)]   # the short last one stays

    def __len__(self):
        return (len(self.utterances) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        epoch = self.epoch if self.training else 0
        for pairs in self.epoch_batches(epoch):
            yield self.corpus.batch(pairs, self.W)
        if self.training:
            self.epoch += 1
