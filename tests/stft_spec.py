"""float64 numpy restatement of the reference's STFT features (the test oracle of the STFT kernel).

The reference computes them with librosa (AudioProcessing.py:156-226, :334-339, WorldFeatLabelGen.py:865-874),
passing every parameter explicitly:
  amp_sp     = |librosa.stft(raw, n_fft, hop, win_length, "hann", center, pad_mode)| / sqrt(n_fft // 2 + 1), [T, K]
  mfbanks    = librosa.filters.mel(sr=fs, n_fft=n_fft, n_mels=n) @ amp_sp.T, transposed, float32
  log_amp_sp = 20 log10(max(1e-5, float32 amp_sp))
librosa is not a dependency; this module restates those definitions from their published form (numpy only)."""
import numpy as np


def window(n_fft, win_length=None):
    """Periodic Hann window of win_length points (scipy.signal.get_window("hann", fftbins=True)), zero-padded to
    n_fft and centred (librosa.util.pad_center).  A window of one point is 1 (scipy's rule for every window)."""
    win_length = n_fft if win_length is None else win_length
    n = np.arange(win_length)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length) if win_length > 1 else np.ones(1)
    lpad = (n_fft - win_length) // 2
    return np.pad(w, (lpad, n_fft - win_length - lpad))


def frames(raw, n_fft, hop, center=True, pad_mode="reflect"):
    """[T, n_fft] frames of librosa.stft (centre padding n_fft // 2 on each side with np.pad)."""
    y = np.asarray(raw, dtype=np.float64)
    if center:
        y = np.pad(y, n_fft // 2, mode=pad_mode)
    n = 1 + (len(y) - n_fft) // hop
    idx = np.arange(n)[:, None] * hop + np.arange(n_fft)[None, :]
    return y[idx]


def amp_sp(raw, n_fft, hop, win_length=None, center=True, pad_mode="reflect"):
    """float64 [T, n_fft // 2 + 1]"""
    spec = np.fft.rfft(frames(raw, n_fft, hop, center, pad_mode) * window(n_fft, win_length)[None, :], axis=1)
    return np.abs(spec) / np.sqrt(n_fft // 2 + 1)


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mels = f / f_sp
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    log_t = f >= min_log_hz
    return np.where(log_t, min_log_mel + np.log(np.where(log_t, f, min_log_hz) / min_log_hz) / logstep, mels)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    freqs = f_sp * m
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    log_t = m >= min_log_mel
    return np.where(log_t, min_log_hz * np.exp(logstep * (np.where(log_t, m, min_log_mel) - min_log_mel)), freqs)


def mel_points(fs, n_mels):
    """The n_mels + 2 band edges f[i] in Hz (librosa.mel_frequencies, fmin 0, fmax fs / 2)."""
    return mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(fs / 2.0), n_mels + 2))


def mel_basis(fs, n_fft, n_mels):
    """librosa.filters.mel defaults (Slaney scale and norm): float32 [n_mels, K], triangles stored into float32,
    then multiplied in place by the float64 factors 2 / (f[i+2] - f[i])."""
    fft_f = np.fft.rfftfreq(n_fft, 1.0 / fs)
    f = mel_points(fs, n_mels)
    w = np.zeros((n_mels, n_fft // 2 + 1), dtype=np.float32)
    for i in range(n_mels):
        rise = (fft_f - f[i]) / (f[i + 1] - f[i])
        fall = (f[i + 2] - fft_f) / (f[i + 2] - f[i + 1])
        w[i] = np.maximum(0.0, np.minimum(rise, fall))
    w *= (2.0 / (f[2:] - f[:-2]))[:, None]
    return w


def mfbanks(raw, fs, n_fft, hop, n_mels, win_length=None):
    a = amp_sp(raw, n_fft, hop, win_length)
    return (mel_basis(fs, n_fft, n_mels).astype(np.float64) @ a.T).T.astype(np.float32)


def log_amp_sp(raw, n_fft, hop, win_length=None):
    a = amp_sp(raw, n_fft, hop, win_length).astype(np.float32)
    return 20 * np.log10(np.maximum(np.float32(1e-5), a))


def trim_front(n_stft, n_world):
    """trim_to_shortest (reference WorldFeatLabelGen.py:891-907) of an STFT stream against WORLD's frame count:
    frames dropped in front."""
    return (n_stft - n_world) // 2
