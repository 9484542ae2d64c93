"""float64 numpy restatement of librosa.griffinlim as the reference calls it (the test oracle of griffinlim.hip).

librosa 0.7 - 0.9 with center=True, length=None, the "hann" window (AudioProcessing.py:279-289, Synthesiser.py:320-351):
  rebuilt = 0
  repeat n_iter times:
      tprev   = rebuilt
      rebuilt = stft(istft(S * angles))
      angles  = rebuilt - momentum / (1 + momentum) * tprev
      angles /= |angles| + eps                                  (eps: tiny of the state's real type)
  return istft(S * angles)
Spectra are [T, K] here (librosa's S transposed).  With c64=True `S * angles`, `rebuilt` and `angles` are rounded
to complex64 where librosa stores them for float32 spectra and the output to float32; the transforms, the
overlap-add and the normalisation stay float64 (as in the kernel).  librosa is not a dependency; this module
restates its definitions on tests/stft_spec.py's window and frames."""
import numpy as np

import stft_spec


def window_sumsquare(win, n_frames, hop, n_fft):
    """librosa.filters.window_sumsquare: the squared window added at every frame's offset, frames in ascending
    order, float64 [n_fft + hop (n_frames - 1)]."""
    x = np.zeros(n_fft + hop * (n_frames - 1))
    w2 = win ** 2
    for t in range(n_frames):
        x[t * hop:t * hop + n_fft] += w2
    return x


def istft(X, hop, n_fft, win_length=None):
    """librosa.istft(center=True, length=None) of X [T, K]: irfft of each frame times the window, overlap-add in
    ascending frame order, division by the window sum-square where it exceeds float32's tiny, n_fft // 2 samples
    trimmed from each end: hop (T - 1) samples."""
    win = stft_spec.window(n_fft, win_length)
    T = X.shape[0]
    frames = np.fft.irfft(X, n=n_fft, axis=1) * win[None, :]
    y = np.zeros(n_fft + hop * (T - 1))
    for t in range(T):
        y[t * hop:t * hop + n_fft] += frames[t]
    wss = window_sumsquare(win, T, hop, n_fft)
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    return y[n_fft // 2:len(y) - n_fft // 2]


def stft(y, hop, n_fft, win_length=None, pad_mode="reflect"):
    """librosa.stft(center=True) as [T, K] complex128."""
    win = stft_spec.window(n_fft, win_length)
    return np.fft.rfft(stft_spec.frames(y, n_fft, hop, True, pad_mode) * win[None, :], axis=1)


def init_phases(shape, random_state):
    """librosa's random initial phases for a [T, K] spectrum: exp(2j pi rng.rand(K, T)), transposed."""
    T, K = shape
    rng = np.random.RandomState(random_state) if isinstance(random_state, int) else random_state
    return np.exp(2j * np.pi * rng.rand(K, T)).T


def griffinlim(S, angles, n_iter, hop, win_length=None, pad_mode="reflect", momentum=0.99, c64=False,
               return_state=False):
    """S [T, K] amplitudes, angles [T, K] initial phases -> waveform of hop (T - 1) samples."""
    S = np.asarray(S, dtype=np.float64)
    n_fft = 2 * (S.shape[1] - 1)
    rnd = (lambda z: z.astype(np.complex64).astype(np.complex128)) if c64 else (lambda z: z)
    eps = np.finfo(np.float32 if c64 else np.float64).tiny
    c = momentum / (1 + momentum)
    angles = rnd(np.asarray(angles, dtype=np.complex128))
    rebuilt = 0.0
    for _ in range(n_iter):
        tprev = rebuilt
        inverse = istft(rnd(S * angles), hop, n_fft, win_length)
        rebuilt = rnd(stft(inverse, hop, n_fft, win_length, pad_mode))
        a = rebuilt - c * tprev
        angles = rnd(a / (np.abs(a) + eps))
    y = istft(rnd(S * angles), hop, n_fft, win_length)
    if c64:
        y = y.astype(np.float32)
    return (y, angles) if return_state else y


def spectral_convergence(S, y, hop, win_length=None, pad_mode="reflect"):
    """||S - |stft(y)|||_F / ||S||_F for S [T, K]."""
    S = np.asarray(S, dtype=np.float64)
    n_fft = 2 * (S.shape[1] - 1)
    return np.linalg.norm(S - np.abs(stft(np.asarray(y, np.float64), hop, n_fft, win_length, pad_mode))) \
        / np.linalg.norm(S)
