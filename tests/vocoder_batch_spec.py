"""A numpy restatement of what a batch of vocoder training windows holds (csrc/vocoder_batch.hip,
data_preparation/VocoderCorpus.py), shared by tests/test_vocoder_trainer_config.py, tests/test_gpu_vocoder_batch.py
and tests/test_gpu_vocoder_trainer.py.  It is built from what other tests already pin: rawwave_cases.mulaw_encode,
scipy's interp1d at numpy.linspace, RawWaveformLabelGen.start_and_end_indices (a host function) and plain slicing.
Nothing here touches a GPU."""
import numpy as np
from scipy.interpolate import interp1d

import rawwave_cases as rc
from idiaptts_amd.src.data_preparation.audio.RawWaveformLabelGen import RawWaveformLabelGen


def multiplier(frame_rate_output_Hz, frame_size_ms):
    return int(frame_rate_output_Hz / (1000 / frame_size_ms))


def window_length(seconds, frame_size_ms, m):
    return int(1000 / frame_size_ms * seconds) * m


def upsampled(F, m):
    """U = sample_linearly(F, m) as scipy computes it: float64 [m T, cin]"""
    T = len(F)
    return interp1d(np.arange(0.0, T), F, axis=0)(np.linspace(0.0, T - 1, m * T))


def usable_range(x, T, m, mu=None, silence_threshold_quantized=None):
    """[lo, hi) of an utterance: samples x, T conditioning frames (None: no conditioning)"""
    lo, hi = 0, len(x)
    if silence_threshold_quantized is not None and mu is not None:
        lo, hi = RawWaveformLabelGen.start_and_end_indices(rc.mulaw_encode(x, mu), silence_threshold_quantized)
    if T is not None:
        hi = min(hi, m * T)
    return lo, hi


def window(x, F, m, mu, a, W, hi):
    """(target [C, W] float32, classes or None, cond [cin, W] float64 of interp1d or None, len) of the window that
    starts at sample a of the utterance (x, F) whose usable range ends at hi"""
    n = min(W, hi - a)
    assert n >= 1
    seg = x[a:a + n]
    if mu:
        classes = rc.mulaw_encode(seg, mu)
        target = np.zeros((mu + 1, W), dtype=np.float32)
        target[classes, np.arange(n)] = 1.0
    else:
        classes = None
        target = np.zeros((1, W), dtype=np.float32)
        target[0, :n] = seg.astype(np.float32)
    cond = None
    if F is not None and F.shape[1] > 0:
        cond = np.zeros((F.shape[1], W), dtype=np.float64)
        cond[:, :n] = upsampled(F, m)[a:a + n].T
    return target, classes, cond, n


def first_and_last_rows(F, m, a, n):
    """columns of a window that are row 0 or row m T - 1 of the up-sampled utterance: there the kernel returns the
    input's first / last row exactly; everywhere else it is within one float32 ulp of interp1d's value (the criterion
    of tests/test_gpu_rawwave.py)"""
    last = m * len(F) - 1
    return [j for j in range(n) if a + j in (0, last)]


def cond_within_criterion(got, F, m, a, n, ref):
    """got [cin, W] float32 against ref = window(...)[2]: exact at the utterance's first and last row, one float32 ulp
    of interp1d's float32 value elsewhere, zeros past n"""
    got = np.asarray(got)
    assert (got[:, n:] == 0).all()
    ref32 = ref[:, :n].astype(np.float32)
    edge = first_and_last_rows(F, m, a, n)
    for j in edge:
        assert np.array_equal(got[:, j], F[0] if a + j == 0 else F[-1])
    inner = np.array([j for j in range(n) if j not in edge], dtype=np.int64)
    if inner.size:
        g, r = got[:, inner].astype(np.float64), ref32[:, inner].astype(np.float64)
        assert (np.abs(g - r) <= np.spacing(np.abs(ref32[:, inner])).astype(np.float64)).all()
    return True
