"""What the four corpus preparation steps (down_sampling, silence_remove, normalize_loudness, high_pass_filter) share:
reading a list of wav files in batches capped by their total samples, and the one PCM-16 writer.

The reference reads each file with soundfile.read and writes it with soundfile.write(out_file, raw, samplerate=fs),
whose default subtype for .wav is PCM_16.  Here a list is planned from the wav headers (rate, channels, length), read
batch by batch with AudioProcessing.get_raw_batch, processed on the GPU as one ragged batch and written by write_pcm16.
A batch holds files of one sampling rate; the kernels give a signal the same bits alone and in any batch, so a file
processed in a list gives the same bytes as processed alone."""
import argparse
import ctypes
import logging
import os
import struct

import numpy as np
import scipy.io.wavfile
import torch

from .... import lib as _lib
from .AudioProcessing import AudioProcessing

MAX_BATCH_SAMPLES = 1 << 24         # 128 MB of float64 per batch on the device, and as much again for the result


def float_to_pcm16(waveform):
    """Samples in [-1, 1) as PCM-16: scaled by 2^15, rounded to nearest, clipped."""
    return np.clip(np.rint(np.asarray(waveform) * 32768.0), -32768, 32767).astype(np.int16)


def write_pcm16(file_path, waveform, fs):
    """soundfile.write(file_path, waveform, samplerate=fs) for a .wav path (default subtype PCM_16).  The directory
    has to exist."""
    scipy.io.wavfile.write(file_path, int(fs), float_to_pcm16(waveform))


def make_parent_dir(file_path):
    directory = os.path.dirname(file_path)
    if directory:
        os.makedirs(directory, exist_ok=True)


def wav_header(path):
    """(sampling rate, channels, samples per channel) from the RIFF header of a wav file: for the files the native
    reader (itts_wav_info) does not take, which is where the channel count matters.  A data chunk that claims more
    bytes than the file holds (streamed or truncated files) counts what is there."""
    file_size = os.path.getsize(path)
    with open(path, "rb") as f:
        riff = f.read(12)
        if len(riff) < 12 or riff[:4] != b"RIFF" or riff[8:12] != b"WAVE":
            raise ValueError("{} is not a RIFF/WAVE file".format(path))
        fs = channels = block_align = None
        while True:
            head = f.read(8)
            if len(head) < 8:
                raise ValueError("{} has no data chunk".format(path))
            tag, size = head[:4], struct.unpack("<I", head[4:])[0]
            if tag == b"fmt ":
                fmt = f.read(size + (size & 1))
                if len(fmt) < 16:
                    raise ValueError("{} has a truncated fmt chunk".format(path))
                _, channels, fs, _, block_align, _ = struct.unpack("<HHIIHH", fmt[:16])
            elif tag == b"data":
                if fs is None or not block_align or not channels:
                    raise ValueError("{} has no usable fmt chunk".format(path))
                return fs, channels, min(size, file_size - f.tell()) // block_align
            else:
                f.seek(size + (size & 1), os.SEEK_CUR)


def wav_layout(path):
    """(sampling rate, channels, samples per channel): from the native reader for the files it takes (mono; the
    length get_raw_batch will deliver), from the RIFF header for the others."""
    fs, n = ctypes.c_int(), ctypes.c_int64()
    rc = _lib.load().itts_wav_info(os.fsencode(path), ctypes.byref(fs), ctypes.byref(n))
    if rc == 0:
        return fs.value, 1, n.value
    if rc != -3:                                # not ITTS_E_UNSUPPORTED: a missing or broken file
        _lib.check(rc, "itts_wav_info")
    return wav_header(path)


def read_id_list(file_id_list):
    """The ids of a list file, one per line, surrounding blanks dropped."""
    with open(file_id_list) as f:
        return [line.strip(" \t\n\r") for line in f.readlines()]


def list_parser(description):
    """The command line the preparation steps share: -w / --dir_wav, -o / --dir_out, -f / --file_id_list, --format."""
    parser = argparse.ArgumentParser(description=description, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-w", "--dir_wav", type=str, dest="dir_wav", required=True,
                        help="directory the wav files are read from")
    parser.add_argument("-o", "--dir_out", type=str, dest="dir_out", required=True,
                        help="directory the processed files are written to, under the same names")
    parser.add_argument("-f", "--file_id_list", type=str, dest="file_id_list", required=True,
                        help="text file with one file id (name without extension) per line")
    parser.add_argument("--format", type=str, dest="format", required=False, default="wav",
                        help="file extension; only wav files are read")
    return parser


def run_command_line(parser, make_step, list_args=()):
    """Parses the command line, creates the output directory and runs make_step(args).process_list over the id list,
    handing on the parsed values named in list_args after the format."""
    logging.basicConfig(level=logging.DEBUG)
    args = parser.parse_args()
    id_list = read_id_list(args.file_id_list)
    os.makedirs(args.dir_out, exist_ok=True)
    make_step(args).process_list(id_list, args.dir_wav, args.dir_out, args.format,
                                 *[getattr(args, name) for name in list_args])


def plan_batches(files, dir_audio, average_channels=False, min_samples=0, min_samples_text=None, max_samples=None):
    """Consecutive runs of `files` (names relative to dir_audio) with one sampling rate and at most max_samples
    (default MAX_BATCH_SAMPLES) samples: a list of (file names, sampling rate).  Before anything is read or written
    this raises ValueError naming the file for a multi-channel file (unless average_channels), an empty one and one of
    at most min_samples samples (with min_samples_text, scipy's wording)."""
    if max_samples is None:
        max_samples = MAX_BATCH_SAMPLES
    batches, current, current_fs, current_n = [], [], None, 0
    for name in files:
        path = os.path.join(dir_audio, name)
        fs, channels, n = wav_layout(path)
        if channels != 1 and not average_channels:
            raise ValueError("{} has {} channels: this step takes mono files (the reference would filter along "
                             "the wrong axis)".format(path, channels))
        if n == 0:
            raise ValueError("{} holds no samples".format(path))
        if n <= min_samples:
            raise ValueError("{}: {} ({} samples)".format(path, min_samples_text, n))
        if current and (fs != current_fs or current_n + n > max_samples):
            batches.append((current, current_fs))
            current, current_n = [], 0
        current.append(name)
        current_fs, current_n = fs, current_n + n
    if current:
        batches.append((current, current_fs))
    return batches


def read_batch(names, dir_audio, average_channels=False):
    """(samples of all files back to back as float64, offsets [n + 1]) of one planned batch.  Multi-channel files are
    averaged to mono (librosa.load's mono=True) when average_channels."""
    paths = [os.path.join(dir_audio, name) for name in names]
    multi = {i for i, p in enumerate(paths) if wav_layout(p)[1] != 1} if average_channels else set()
    if not multi:
        samples, offsets, _ = AudioProcessing.get_raw_batch(paths)
        return np.asarray(samples), np.asarray(offsets, dtype=np.int64)
    signals = [None] * len(paths)
    mono = [i for i in range(len(paths)) if i not in multi]
    if mono:
        samples, offsets, _ = AudioProcessing.get_raw_batch([paths[i] for i in mono])
        for k, i in enumerate(mono):
            signals[i] = samples[offsets[k]:offsets[k + 1]]
    for i in multi:
        signals[i] = AudioProcessing.read_wav(paths[i])[0].mean(axis=1)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in signals])]).astype(np.int64)
    return np.concatenate(signals), offsets


def to_device(samples):
    _lib.require_gpu()
    return torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float64)).to(torch.device("cuda"))


def split(array, offsets):
    return [array[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def process_list(files, dir_audio, dir_out, step, precheck=None, **plan_args):
    """Runs step(samples, offsets, fs, paths) -> list of float64 signals over the planned batches of `files` and
    writes each result to dir_out under its name.  precheck(samples, offsets, paths) may refuse a batch by raising:
    it sees every batch before the first file is written (a list planned into several batches is read once more for
    that).  Returns the results of the last batch (process_file: the batch of one)."""
    batches = plan_batches(files, dir_audio, **plan_args)

    def read(names):
        samples, offsets = read_batch(names, dir_audio)
        paths = [os.path.join(dir_audio, name) for name in names]
        if precheck is not None:
            precheck(samples, offsets, paths)
        return samples, offsets, paths

    if precheck is not None and len(batches) > 1:
        for names, _ in batches:
            read(names)
    results = []
    for names, fs in batches:
        samples, offsets, paths = read(names)
        results = step(samples, offsets, fs, paths)
        for name, raw in zip(names, results):
            out_file = os.path.join(dir_out, name)
            make_parent_dir(out_file)
            write_pcm16(out_file, raw, fs)
    return results
