"""Numpy restatements of the four corpus preparation steps, written per output sample or frame from their formulas
(not scipy's code path: no lfilter, no upfirdn, no np.convolve).  The tests compare the kernels and scipy against
these; the filter designs (firls, firwin) are scipy's, as in the package."""
import math
from math import gcd

import numpy as np
import scipy.signal


# ------------------------------------------------------------------------------------------------ zero-phase FIR
def filtfilt_spec(b, x):
    """scipy.signal.filtfilt(b, [1], x), padtype "odd", padlen 3 * len(b): the odd extension, a forward pass in which
    everything before the first value equals it (lfilter_zi's start for an FIR filter), the same pass over the
    reversed result, reversed again, the extension stripped.  Tap k ascending for every output."""
    b = np.asarray(b, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    K, n = len(b), len(x)
    L = 3 * K
    if n <= L:
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % L)
    ext = np.concatenate([2 * x[0] - x[L:0:-1], x, 2 * x[-1] - x[-2:-L - 2:-1]])

    def one_pass(v):
        idx = np.arange(len(v))
        y = np.zeros(len(v))
        for k in range(K):
            y += b[k] * v[np.maximum(idx - k, 0)]
        return y

    y = one_pass(ext)
    y = one_pass(y[::-1])[::-1]
    return y[L:-L]


def filtfilt_bound(b, x):
    """16 * numtaps * 2**-53 * (sum|b|)**2 * max|x|: two passes of numtaps-term sums over an extension of at most
    three times the signal's peak."""
    b = np.asarray(b, dtype=np.float64)
    return 16 * len(b) * 2.0 ** -53 * np.abs(b).sum() ** 2 * np.abs(x).max()


# ------------------------------------------------------------------------------------------------ resampling
def resample_filter(up, down):
    """(up, down) reduced by their gcd and scipy.signal.resample_poly's default filter for them, times up."""
    g = gcd(int(up), int(down))
    up, down = int(up) // g, int(down) // g
    max_rate = max(up, down)
    half = 10 * max_rate
    h = scipy.signal.firwin(2 * half + 1, 1.0 / max_rate, window=("kaiser", 5.0)) * up
    return up, down, h


def resample_spec(x, up, down):
    """y[m] = sum_k h[k] xu[m down + half - k], xu = x with up - 1 zeros between its samples, zeros outside,
    ceil(n up / down) outputs: the taps of output m's phase against the samples they meet."""
    x = np.asarray(x, dtype=np.float64)
    up, down, h = resample_filter(up, down)
    K, n = len(h), len(x)
    half = (K - 1) // 2
    n_out = -(-n * up // down)
    y = np.zeros(n_out)
    for m in range(n_out):
        a = m * down + half
        p, i0 = a % up, a // up
        j = np.arange((K - 1 - p) // up + 1)
        i = i0 - j
        ok = (i >= 0) & (i < n)
        y[m] = math.fsum(h[p + j[ok] * up] * x[i[ok]])
    return y


def resample_bound(x, up, down):
    """16 * K * 2**-53 * S * max|x|, K the taps per output, S the largest per-phase sum|h|."""
    up, down, h = resample_filter(up, down)
    K = -(-len(h) // up)
    S = max(np.abs(h[p::up]).sum() for p in range(up))
    return 16 * K * 2.0 ** -53 * S * np.abs(x).max()


# ------------------------------------------------------------------------------------------------ loudness
def loudness_spec(x, ref_rms=0.1):
    """(x - mean) * sqrt(n ref_rms^2 / sum((x - mean)^2)), both sums exact (math.fsum)."""
    x = np.asarray(x, dtype=np.float64)
    c = x - math.fsum(x) / len(x)
    return c * math.sqrt(len(x) * ref_rms ** 2 / math.fsum(c * c))


# ------------------------------------------------------------------------------------------------ frame RMS, trim
def frame_rms_spec(x, frame_length, hop, pad_mode="constant"):
    """librosa.feature.rms(y=x, frame_length, hop_length, center=True, pad_mode): frame f covers the padded samples
    f hop .. f hop + frame_length - 1."""
    xp = np.pad(np.asarray(x, dtype=np.float64), frame_length // 2, mode=pad_mode)
    n_frames = 1 + (len(xp) - frame_length) // hop
    return np.array([math.sqrt(math.fsum(xp[f * hop:f * hop + frame_length] ** 2) / frame_length)
                     for f in range(n_frames)])


def trim_indices_spec(rms, n, hop, top_db, margin_db=1e-6):
    """librosa.effects.trim's (start, end) from the frame RMS: dB relative to the loudest frame, non-silent above
    -top_db.  Asserts that no frame lies within margin_db of the threshold (an index that hangs on a rounding proves
    nothing)."""
    rms = np.asarray(rms, dtype=np.float64)
    db = 10.0 * np.log10(np.maximum(1e-10, rms ** 2))
    db = db - 10.0 * np.log10(max(1e-10, rms.max() ** 2))
    assert np.all(np.abs(db + abs(top_db)) > margin_db), "a frame sits on the threshold"
    nonzero = np.flatnonzero(db > -abs(top_db))
    if nonzero.size == 0:
        return 0, 0
    return int(nonzero[0]) * hop, min(n, (int(nonzero[-1]) + 1) * hop)


def keep_slice_spec(n, fs, indices, min_silence_ms):
    """The reference's own trimming behind librosa's indices: (start_frame, end_frame) of raw[start_frame:end_frame]
    and which of its two warnings it logs."""
    trim_start = indices[0] / fs * 1000
    trim_end = (n - indices[1]) / fs * 1000
    warn_start = trim_start < min_silence_ms
    trim_start = 0 if warn_start else trim_start - min_silence_ms
    warn_end = trim_end < min_silence_ms
    trim_end = 0 if warn_end else trim_end - min_silence_ms
    return int(trim_start * fs / 1000), int(-trim_end * fs / 1000 - 1), warn_start, warn_end


def silence_remove_spec(x, fs, frame_length, min_silence_ms=200, silence_threshold_db=-50, hop_size_ms=None,
                        pad_mode="constant"):
    """SilenceRemover.process_file on samples: the kept samples and the slice."""
    if hop_size_ms is None:
        hop_size_ms = min(min_silence_ms, 32)
    hop = int(fs / 1000 * hop_size_ms)
    rms = frame_rms_spec(x, frame_length, hop, pad_mode)
    indices = trim_indices_spec(rms, len(x), hop, abs(silence_threshold_db))
    start, end, _, _ = keep_slice_spec(len(x), fs, indices, min_silence_ms)
    return np.asarray(x)[start:end], (start, end)


# ------------------------------------------------------------------------------------------------ output
def pcm16_spec(y):
    """What a float signal becomes in a PCM-16 wav file (soundfile's default subtype for .wav)."""
    return np.clip(np.rint(np.asarray(y, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def pcm16_near_boundary(y, tol):
    """Where y * 32768 lies within tol * 32768 of a rounding boundary (k + 0.5): there a result within tol of y may
    round to the neighbouring integer."""
    v = np.asarray(y, dtype=np.float64) * 32768.0
    return np.abs(v - np.floor(v) - 0.5) <= tol * 32768.0


# ------------------------------------------------------------------------------------------------ inputs
def speech_like(n, fs, seed, lead=0, tail=0, level=0.1, floor=1e-5):
    """`lead` samples of faint noise, n - lead - tail samples of a loud harmonic signal with noise, `tail` samples of
    faint noise: the loud part lies 80 dB above the floor, so no frame of it or of the silences comes near a -50 dB
    threshold except the few that straddle an edge (trim_indices_spec asserts the margin)."""
    rng = np.random.default_rng(seed)
    x = floor * rng.standard_normal(n)
    m = n - lead - tail
    t = np.arange(m) / fs
    x[lead:lead + m] = level * (np.sin(2 * np.pi * 180.0 * t) + 0.5 * np.sin(2 * np.pi * 1230.0 * t + 1.0)
                                + 0.3 * rng.standard_normal(m))
    return x
