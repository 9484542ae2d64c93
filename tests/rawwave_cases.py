"""Shared by tests/test_rawwave_host.py and tests/test_gpu_rawwave.py: numpy restatements of the reference's mu-law
companding (data_preparation/audio/RawWaveformLabelGen.py:164-173; the module itself needs pydub to import) and a
PCM-16 wav writer for the tests' own files.  Nothing here touches a GPU."""
import numpy as np
import scipy.io.wavfile

MUS = (255, 1023, 65535)


def pcm16_values():
    """all 65 536 PCM-16 values as load_sample delivers them: float64 in [-1, 1)"""
    return np.arange(-32768, 32768, dtype=np.float64) / 32768.0


def mulaw_before_truncation(raw, mu):
    return ((np.sign(raw) * np.log(1 + mu * np.abs(raw)) / np.log(1 + mu)) + 1.0) * (mu / 2.0)


def mulaw_encode(raw, mu):
    return mulaw_before_truncation(raw, mu).astype(np.int64)


def mulaw_decode(index, mu):
    raw = index / (mu / 2) - 1
    return np.sign(raw) / mu * (np.power(1.0 + mu, np.abs(raw)) - 1.0)


def write_wav(path, n, seed, fs=16000, amplitude=0.6):
    """a decaying two-tone signal with a little noise, as PCM-16: returns the int16 samples"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = amplitude * np.exp(-3.0 * t) * (np.sin(2 * np.pi * 220.0 * t) + 0.5 * np.sin(2 * np.pi * 1330.0 * t + seed))
    pcm = np.clip(np.round((x / 1.5 + 0.01 * rng.standard_normal(n)) * 32768.0), -32768, 32767).astype(np.int16)
    scipy.io.wavfile.write(path, fs, pcm)
    return pcm
