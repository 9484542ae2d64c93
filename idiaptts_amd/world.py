"""Batched, GPU-resident WORLD feature path (the MI355X-native fast path behind the drop-in shims).

analysis : wav(s) -> DIO -> StoneMask -> CheapTrick (+ fused SPTK mcep) / D4C (+ coded bap)
STFT     : wav(s) -> amplitude spectrum / its dB form / mel filter banks (librosa's STFT features, stft.hip)
Griffin-Lim: amplitude spectra -> waveforms (librosa.griffinlim, griffinlim.hip)
mel inverse: mel filter banks -> amplitude spectra (librosa's NNLS mel_to_stft, mel_inverse.hip)
synthesis: (f0, sp, ap) -> WORLD synthesis -> float32 (+ de-pre-emphasis)
Utterances are concatenated and processed by single launches; only the small per-frame features
(f0, mcep, bap) travel back to the host unless the spectral envelope is asked for.
"""
import functools

import numpy as np
import torch

from . import lib as _lib
from . import ops


def _device(device):
    _lib.require_gpu()
    return torch.device(device if device is not None else "cuda")


_side_streams = {}


def _side_stream(dev):
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _side_streams:
        # (stream priorities: this stack has two levels, default and high -- measured, the side stream high or not
        # makes no difference to where the two streams' kernels end: scripts/r5_job36.sh)
        _side_streams[key] = torch.cuda.Stream(device=dev)
    return _side_streams[key]


def num_frames(n, fs, hop_ms=5.0):
    return int(_lib.load().itts_world_num_frames(int(n), int(fs), float(hop_ms)))


def offsets(lengths):
    off = [0]
    for n in lengths:
        off.append(off[-1] + int(n))
    return off


def lf0_vuv_from_f0(f0, f0_silence_threshold=30, lf0_zero=0, device=None):
    """WorldFeatLabelGen.world_extract_features :798-802 (float32 log, threshold,
    interpolate_lin) for one contour: (lf0 [T, 1] f32, vuv [T, 1] f32)."""
    dev = _device(device)
    f0 = np.ascontiguousarray(f0, dtype=np.float64).reshape(-1)
    lf0, vuv = ops.lf0_vuv(torch.from_numpy(f0).to(dev), [0, len(f0)], f0_silence_threshold,
                           lf0_zero)
    return lf0.cpu().numpy()[:, None], vuv.cpu().numpy()[:, None]


def estimate_f0(x, x_off, f_off, fs, hop_ms=5.0, f0_method="dio"):
    """The F0 stage: "dio" = pyworld.wav2world's DIO + StoneMask (what the reference extracts with,
    WorldFeatLabelGen.py:792-793); "harvest" = pyworld.harvest (no StoneMask pass: Harvest refines
    its own candidates).  Both share the frame grid int(1000 n / fs / hop) + 1."""
    if f0_method == "dio":
        return ops.stonemask(x, x_off, ops.dio(x, x_off, f_off, fs, hop_ms), f_off, fs, hop_ms)
    if f0_method == "harvest":
        return ops.harvest(x, x_off, f_off, fs, hop_ms)
    raise NotImplementedError("Unknown F0 estimator {} (dio, harvest).".format(f0_method))


def analyse_batch(raws, fs, hop_ms=5.0, n_fft=None, want_sp=True, want_ap=False,
                  mcep_order=None, mcep_alpha=None, want_bap=True, device=None, f0_method="dio",
                  amplitude=False, lf0_params=None):
    """raws: list of float64 waveforms (already pre-emphasised). Returns a list of dicts with
    f0 [T] f64, and optionally sp [T,K] f64 (power; with `amplitude` its square root, taken on the device),
    ap [T,K] f64, mcep [T,order+1] f32, bap [T,nap] f32; with lf0_params = (f0_silence_threshold, lf0_zero)
    also lf0 / vuv [T, 1] f32 (WorldFeatLabelGen.py:798-802) from the contour while it is still on the device."""
    dev = _device(device)
    L = _lib.load()
    n_fft = n_fft or L.itts_cheaptrick_fft_size(int(fs), 71.0)
    x_off = offsets([len(r) for r in raws])
    f_off = offsets([num_frames(len(r), fs, hop_ms) for r in raws])
    x = torch.from_numpy(np.ascontiguousarray(np.concatenate(raws), dtype=np.float64)).to(dev)
    f0 = estimate_f0(x, x_off, f_off, fs, hop_ms, f0_method)
    sp = mc = ap = bap = None
    # CheapTrick/mcep and D4C only share their inputs: run D4C on a side stream so the two
    # occupancy-bound kernels overlap
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev)
    if want_ap or want_bap:
        side.wait_stream(main)
        with torch.cuda.stream(side):
            ap, bap = ops.d4c(x, x_off, f0, f_off, fs, hop_ms, n_fft, want_ap=want_ap,
                              want_bap=torch.float32 if want_bap else None)
    if want_sp or mcep_order is not None:
        sp, mc, _ = ops.cheaptrick_mcep(x, x_off, f0, f_off, fs, hop_ms, n_fft, want_sp=want_sp,
                                        order=mcep_order, alpha=mcep_alpha)
    lf0 = vuv = None
    if lf0_params is not None:
        lf0, vuv = ops.lf0_vuv(f0, f_off, lf0_params[0], lf0_params[1])
    if amplitude and sp is not None:
        ops.sqrt_inplace(sp)
    if want_ap or want_bap:
        main.wait_stream(side)
        for t in (x, f0):
            t.record_stream(side)
    f0 = f0.cpu().numpy()
    lf0 = lf0.cpu().numpy() if lf0 is not None else None
    vuv = vuv.cpu().numpy() if vuv is not None else None
    sp = sp.cpu().numpy() if sp is not None else None
    mc = mc.cpu().numpy() if mc is not None else None
    ap = ap.cpu().numpy() if ap is not None else None
    bap = bap.cpu().numpy() if bap is not None else None
    out = []
    for u in range(len(raws)):
        a, b = f_off[u], f_off[u + 1]
        out.append({"f0": f0[a:b],
                    "lf0": lf0[a:b, None] if lf0 is not None else None,
                    "vuv": vuv[a:b, None] if vuv is not None else None,
                    "sp": sp[a:b] if sp is not None else None,
                    "ap": ap[a:b] if ap is not None else None,
                    "mcep": mc[a:b] if mc is not None else None,
                    "bap": bap[a:b] if bap is not None else None})
    return out


# ------------------------------------------------------------------------------------------ STFT features
STFT_SP_TYPES = ("mfbanks", "amp_sp", "log_amp_sp")


def fs_to_frame_length(fs):
    return int(_lib.load().itts_cheaptrick_fft_size(int(fs), 71.0))


def stft_hop(fs, hop_ms):
    """hop_length of the reference's librosa calls: int(hop_size_ms / 1000. * fs) (AudioProcessing.py:180)."""
    return int(hop_ms / 1000. * fs)


def check_stft_args(n_fft, window="hann", pad_mode="reflect"):
    """What the STFT kernel covers; anything else raises before any device work."""
    if n_fft not in (1024, 2048):
        raise NotImplementedError("STFT n_fft={} is not implemented (1024, 2048).".format(n_fft))
    if window != "hann":
        raise NotImplementedError("STFT window {!r} is not implemented ('hann').".format(window))
    if pad_mode not in ("reflect", "constant"):
        raise NotImplementedError("STFT pad_mode {!r} is not implemented ('reflect', 'constant').".format(pad_mode))


def stft_num_frames(n, n_fft, hop, center=True):
    """Frames of librosa.stft: 1 + n // hop with the centre padding, 1 + (n - n_fft) // hop without."""
    if center:
        return 1 + int(n) // hop
    if n < n_fft:
        raise ValueError("center=False needs at least n_fft={} samples, got {}.".format(n_fft, n))
    return 1 + (int(n) - n_fft) // hop


@functools.lru_cache(maxsize=None)
def stft_window(n_fft, win_length=None, window="hann"):
    """librosa.stft's window: scipy.signal.get_window(window, win_length, fftbins=True), zero-padded to n_fft
    and centred (librosa.util.pad_center).  float64 [n_fft], read-only."""
    import scipy.signal
    win_length = n_fft if win_length is None else int(win_length)
    if not 0 < win_length <= n_fft:
        raise ValueError("win_length={} must be in (0, n_fft={}].".format(win_length, n_fft))
    w = np.asarray(scipy.signal.get_window(window, win_length, fftbins=True), dtype=np.float64)
    lpad = (n_fft - win_length) // 2
    out = np.zeros(n_fft)
    out[lpad:lpad + win_length] = w
    out.setflags(write=False)
    return out


def hz_to_mel(f):
    """Slaney mel scale (librosa.hz_to_mel, htk=False): linear below 1 kHz at 200/3 Hz per mel, logarithmic
    above with step log(6.4) / 27."""
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep,
                    f / f_sp)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (np.maximum(m, min_log_mel) - min_log_mel)),
                    f_sp * m)


@functools.lru_cache(maxsize=None)
def mel_basis(fs, n_fft, n_mels):
    """librosa.filters.mel(sr=fs, n_fft=n_fft, n_mels=n_mels) with its defaults (fmin 0, fmax fs / 2, Slaney
    scale, norm="slaney"): triangles computed in float64 and stored into float32, then scaled in place by the
    float64 Slaney factors 2 / (f[i+2] - f[i]) -- float32 [n_mels, n_fft // 2 + 1], rounded twice like librosa's."""
    n_mels = int(n_mels)
    fftfreqs = np.fft.rfftfreq(n=n_fft, d=1.0 / fs)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(float(fs) / 2), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    weights = np.zeros((n_mels, n_fft // 2 + 1), dtype=np.float32)
    for i in range(n_mels):
        weights[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, np.newaxis]
    weights.setflags(write=False)
    return weights


@functools.lru_cache(maxsize=None)
def mel_tables(fs, n_fft, n_mels):
    """The kernel's form of mel_basis: per filter (first bin, bins, first weight) of its contiguous support,
    int32 [3 n_mels], and the weights of all supports back to back, float32."""
    basis = mel_basis(fs, n_fft, n_mels)
    tab, ws = [], []
    pos = 0
    for row in basis:
        nz = np.flatnonzero(row)
        k0, n = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if len(nz) else (0, 0)
        tab += [k0, n, pos]
        ws.append(row[k0:k0 + n])
        pos += n
    return np.asarray(tab, dtype=np.int32), np.concatenate(ws).astype(np.float32)


_stft_device_tables = {}


def _stft_table(key, build, dev):
    k = key + (dev.index if dev.index is not None else torch.cuda.current_device(),)
    t = _stft_device_tables.get(k)
    if t is None:
        t = _stft_device_tables[k] = tuple(torch.from_numpy(np.array(a, order="C")).to(dev) for a in build())
    return t


def stft_features(x, x_off, f_off, first, fs, sp_type, n_fft, hop, n_mels=None, win_length=None,
                  center=True, pad_mode="reflect", out=None):
    """The STFT feature rows of utterances stored back to back in the float64 device tensor x: row f_off[u] + i is
    frame first[u] + i of utterance u.  sp_type "amp_sp" (float32; "amp_sp_f64": float64), "log_amp_sp" or
    "mfbanks" (n_mels bands)."""
    check_stft_args(n_fft, "hann", pad_mode)
    dev = x.device
    (window,) = _stft_table(("window", n_fft, win_length), lambda: (stft_window(n_fft, win_length),), dev)
    pad = pad_mode if center else None
    if sp_type == "mfbanks":
        tab, w = _stft_table(("mel", fs, n_fft, n_mels), lambda: mel_tables(fs, n_fft, n_mels), dev)
        return ops.mel_filterbank(x, x_off, f_off, first, n_fft, hop, pad, window, tab, w, n_mels, out=out)
    return ops.stft_amp(x, x_off, f_off, first, n_fft, hop, pad, window, kind=sp_type, out=out)


def mel_project(amp_sp, fs, n_fft, n_mels):
    """mel_basis @ amp_sp.T, transposed, float32, for a given amplitude spectrum [T, n_fft // 2 + 1] on the device."""
    tab, w = _stft_table(("mel", fs, n_fft, n_mels), lambda: mel_tables(fs, n_fft, n_mels), amp_sp.device)
    return ops.mel_project(amp_sp, tab, w, n_mels)


# ------------------------------------------------------------------------------------------ mel inverse
MEL_INVERSE_TOL = 1e-6      # KKT stopping threshold, relative to max |A^T b|
MEL_INVERSE_CAP = 1024      # iteration cap
MEL_INVERSE_CHECK = 16      # iterations between stopping tests
MEL_INVERSE_MAX_MELS = 256


def mel_basis_plain(fs, n_fft, n_mels, dtype=np.float32):
    """librosa.filters.mel(sr=fs, n_fft=n_fft, n_mels=n_mels, norm=None, dtype=dtype): the Slaney-scale triangles
    computed in float64 and stored as `dtype`, without the Slaney factors of mel_basis.  [n_mels, n_fft // 2 + 1]"""
    n_mels = int(n_mels)
    fftfreqs = np.fft.rfftfreq(n=n_fft, d=1.0 / fs)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(float(fs) / 2), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    weights = np.zeros((n_mels, n_fft // 2 + 1), dtype=dtype)
    for i in range(n_mels):
        weights[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    return weights


def check_mel_inverse_args(n_fft, n_mels):
    """What mel_inverse.hip covers; anything else raises before any device work."""
    if n_fft not in (1024, 2048):
        raise NotImplementedError("mel inversion n_fft={} is not implemented (1024, 2048).".format(n_fft))
    if not 1 <= int(n_mels) <= MEL_INVERSE_MAX_MELS:
        raise NotImplementedError("mel inversion n_mels={} is not implemented (1 .. {}).".format(
            n_mels, MEL_INVERSE_MAX_MELS))


@functools.lru_cache(maxsize=None)
def mel_inverse_tables(fs, n_fft, n_mels, dtype=np.float32):
    """The kernel's form of the norm=None basis A (mel_basis_plain, values rounded to `dtype` -- float32 or
    float64 -- then used in float64), over KP = 64 ceil(K / 64) bins, zero beyond K:
      bin_j  int32 [KP]       m1 + 1, where m1, m1 + 1 are the filters the bin lies in (m1 = -1: only filter 0;
                              bins in no filter carry the previous bin's m1 with zero weights, so m1 never falls)
      bin_w  float64 [KP, 2]  A[m1, k], A[m1 + 1, k] (0 outside the basis)
      filt   int32 [n_mels, 3]  sb, eb, ea: filter m's bins are [sb, eb) (m1 = m - 1) and [eb, ea) (m1 = m)
      pinv_t float64 [n_mels, KP]  np.linalg.pinv(A)^T (librosa's start)
    and 1 / lambda_max(A A^T).  Raises NotImplementedError when a bin lies in more than two filters or in two
    that are not adjacent."""
    check_mel_inverse_args(n_fft, n_mels)
    dtype = np.dtype(dtype)
    A = mel_basis_plain(fs, n_fft, n_mels, dtype).astype(np.float64)
    n_mels, K = A.shape
    KP = 64 * ((K + 63) // 64)
    bin_j = np.zeros(KP, dtype=np.int32)
    bin_w = np.zeros((KP, 2), dtype=np.float64)
    m1 = -1
    for k in range(K):
        nz = np.flatnonzero(A[:, k])
        if len(nz) > 2 or (len(nz) == 2 and nz[1] != nz[0] + 1):
            raise NotImplementedError("mel inversion: bin {} lies in filters {} (at most two adjacent ones are "
                                      "implemented).".format(k, list(nz)))
        if len(nz) == 2:
            m = int(nz[0])
        elif len(nz) == 1:          # as the lower filter after a bin of the same pair, else as the upper one
            m = int(nz[0]) if m1 >= nz[0] else int(nz[0]) - 1
        else:
            m = m1
        if m < m1:
            raise NotImplementedError("mel inversion: the filters of bin {} fall below those of bin {}."
                                      .format(k, k - 1))
        m1 = m
        bin_w[k] = (A[m1, k] if m1 >= 0 else 0.0, A[m1 + 1, k] if m1 + 1 < n_mels else 0.0)
        bin_j[k] = m1 + 1
    j = bin_j[:K] - 1
    filt = np.zeros((n_mels, 3), dtype=np.int32)
    for m in range(n_mels):
        filt[m] = (np.searchsorted(j, m - 1, "left"), np.searchsorted(j, m, "left"), np.searchsorted(j, m, "right"))
    pinv_t = np.zeros((n_mels, KP))
    pinv_t[:, :K] = np.linalg.pinv(A).T
    # a bin in no filter (0 Hz, the Nyquist bin) is a zero column of A and a zero row of pinv(A); the SVD leaves
    # 1e-17 there, which no iteration would move (its gradient is 0): all-negative bands would not invert to 0
    pinv_t[:, :K][:, ~A.any(axis=0)] = 0.0
    inv_l = 1.0 / float(np.linalg.eigvalsh(A @ A.T)[-1])
    return bin_j, bin_w, filt, pinv_t, inv_l


def mel_inverse(mel, fs, n_fft, tol=MEL_INVERSE_TOL, max_iter=MEL_INVERSE_CAP, return_iters=False):
    """NNLS inversion of the mel filter banks mel [F, n_mels] (float32 or float64 rows on the device; the frames
    of any number of utterances) -> K x [F, n_fft // 2 + 1] on the device, float32 for float32 input, else float64:
    librosa.feature.inverse.mel_to_stft(mel.T, sr=fs, n_fft=n_fft, power=1.0, norm=None).T * K as the reference's
    mfbanks_to_amp_sp computes it, on mel_inverse.hip's FISTA iteration (tests/mel_inverse_spec.py).  With
    return_iters also the int32 [F] iterations each frame took."""
    if mel.dim() != 2:
        raise ValueError("mel must be [frames, n_mels]")
    check_mel_inverse_args(n_fft, mel.shape[1])
    max_iter = int(max_iter)
    if max_iter < 0:
        raise ValueError("max_iter={} must not be negative".format(max_iter))
    if not tol >= 0:
        raise ValueError("tol={} must not be negative".format(tol))
    if mel.dtype not in (torch.float32, torch.float64):
        mel = mel.to(torch.float64)
    dtype = np.float32 if mel.dtype == torch.float32 else np.float64
    n_mels = int(mel.shape[1])
    bin_j, bin_w, filt, pinv_t, inv_l = mel_inverse_tables(fs, n_fft, n_mels, dtype)
    dev = mel.device
    tabs = _stft_table(("mel_inverse", fs, n_fft, n_mels, np.dtype(dtype).name),
                       lambda: (bin_j, bin_w, filt, pinv_t), dev)
    if mel.shape[0] > 0 and mel.stride(1) != 1:
        mel = mel.contiguous()
    iters = torch.empty(mel.shape[0], dtype=torch.int32, device=dev) if return_iters else None
    out = ops.mel_inverse(mel, n_fft, *tabs, inv_l, tol, max_iter, MEL_INVERSE_CHECK, mel.dtype, iters)
    return (out, iters) if return_iters else out


# ------------------------------------------------------------------------------------------ Griffin-Lim
def griffinlim_args(n_bins, n_frames, hop_length=None, win_length=None, window="hann", center=True, length=None,
                    pad_mode="reflect", momentum=0.99, init="random", random_state=None):
    """librosa.griffinlim's argument handling for spectra of n_bins bins and the given frame counts, restricted to
    what griffinlim.hip covers; raises before any device work.  Returns (n_fft, hop_length, win_length, rng)."""
    n_fft = 2 * (int(n_bins) - 1)
    if n_fft not in (1024, 2048):
        raise NotImplementedError("Griffin-Lim n_fft={} is not implemented (1024, 2048).".format(n_fft))
    if window != "hann":
        raise NotImplementedError("Griffin-Lim window {!r} is not implemented ('hann').".format(window))
    if not center:
        raise NotImplementedError("Griffin-Lim center=False is not implemented.")
    if length is not None:
        raise NotImplementedError("Griffin-Lim length={} is not implemented (None).".format(length))
    check_stft_args(n_fft, window, pad_mode)
    win_length = n_fft if win_length is None else int(win_length)
    hop_length = win_length // 4 if hop_length is None else int(hop_length)
    if not 0 < win_length <= n_fft:
        raise ValueError("win_length={} must be in (0, n_fft={}].".format(win_length, n_fft))
    if not 0 < hop_length <= n_fft // 2:
        raise NotImplementedError("Griffin-Lim hop_length={} is not implemented (1 .. n_fft / 2 = {})."
                                  .format(hop_length, n_fft // 2))
    if momentum > 1:
        import warnings
        warnings.warn("Momentum {} > 1 can be unstable. Proceed with caution.".format(momentum))
    elif momentum < 0:
        raise ValueError("griffinlim() called with momentum={} < 0".format(momentum))
    if init not in ("random", None):
        raise ValueError("init={} must either None or 'random'".format(init))
    for t in n_frames:
        if t < 2:
            raise ValueError("Griffin-Lim needs at least 2 frames, got {} (the signal would be empty).".format(t))
    if random_state is None:
        rng = np.random
    elif isinstance(random_state, (int, np.integer)) and not isinstance(random_state, bool):
        rng = np.random.RandomState(seed=int(random_state))
    elif isinstance(random_state, np.random.RandomState):
        rng = random_state
    else:
        raise ValueError("Unsupported random_state={!r}".format(random_state))
    return n_fft, hop_length, win_length, rng


def griffinlim_init_phases(shapes, init, rng, dtype=np.complex128):
    """The initial phases of librosa.griffinlim, [T, K] per spectrum of shape (T, K): exp(2j pi rng.rand(K, T)),
    drawn in librosa's [K, T] order, one spectrum after the other from the same rng, stored as `dtype`; all ones
    for init=None."""
    out = []
    for T, K in shapes:
        if init is None:
            out.append(np.ones((T, K), dtype=dtype))
        else:
            out.append(np.exp(2j * np.pi * rng.rand(K, T)).astype(dtype).T)
    return out


def griffinlim_batch(spectra, n_iter=32, hop_length=None, win_length=None, window="hann", center=True, length=None,
                     pad_mode="reflect", momentum=0.99, init="random", random_state=None, device=None):
    """librosa.griffinlim of every amplitude spectrum in `spectra` (list of [T_u, K] arrays: librosa's S
    transposed) in one batched run of griffinlim.hip, one launch per iteration.  float32 spectra keep a complex64
    phase state and give float32 waveforms, anything else float64.  The random initial phases are drawn utterance
    by utterance in the given order from one rng (the reference's per-utterance loop with the same seed).
    Returns one waveform of hop (T_u - 1) samples per spectrum."""
    spectra = [np.asarray(sp) for sp in spectra]
    if not spectra:
        return []
    if any(sp.ndim != 2 or sp.shape[1] != spectra[0].shape[1] for sp in spectra):
        raise ValueError("spectra must be [T, K] arrays with the same K")
    n_fft, hop, win_length, rng = griffinlim_args(spectra[0].shape[1], [sp.shape[0] for sp in spectra],
                                                  hop_length, win_length, window, center, length, pad_mode,
                                                  momentum, init, random_state)
    n_iter = int(n_iter)
    if n_iter < 0:
        raise ValueError("n_iter={} must not be negative".format(n_iter))
    f32 = all(sp.dtype in (np.float16, np.float32) for sp in spectra)
    real, cplx = (np.float32, np.complex64) if f32 else (np.float64, np.complex128)
    phases = griffinlim_init_phases([sp.shape for sp in spectra], init, rng, cplx)
    dev = _device(device)
    f_off = offsets([sp.shape[0] for sp in spectra])
    S = torch.from_numpy(np.ascontiguousarray(np.concatenate(spectra), dtype=real)).to(dev)
    angles = torch.from_numpy(np.ascontiguousarray(np.concatenate(phases))).to(dev)
    (win,) = _stft_table(("window", n_fft, win_length), lambda: (stft_window(n_fft, win_length),), dev)
    y = ops.griffinlim(S, angles, f_off, n_fft, hop, pad_mode, win, n_iter, momentum).cpu().numpy()
    y_off = offsets([hop * (sp.shape[0] - 1) for sp in spectra])
    return [y[y_off[u]:y_off[u + 1]] for u in range(len(spectra))]


def griffinlim(S, n_iter=32, hop_length=None, win_length=None, window="hann", center=True, length=None,
               pad_mode="reflect", momentum=0.99, init="random", random_state=None, device=None):
    """librosa.griffinlim(S, ...) for one amplitude spectrum S [K, T] (librosa's orientation), on the GPU."""
    S = np.asarray(S)
    if S.ndim != 2:
        raise ValueError("S must be [n_fft // 2 + 1, T]")
    return griffinlim_batch([S.T], n_iter, hop_length, win_length, window, center, length, pad_mode, momentum,
                            init, random_state, device)[0]


def _extract_cmp_stft(x, x_off, fs, hop_ms, n_fft, sp_type, n_mels, win_length_ms, world_streams,
                      f0_silence_threshold, lf0_zero, add_deltas, f0_method):
    """extract_cmp_batch for the STFT sp_types (x already on the device)."""
    dev = x.device
    hop = stft_hop(fs, hop_ms)
    win_length = None if win_length_ms is None else int(win_length_ms / 1000. * fs)
    lens = [b - a for a, b in zip(x_off[:-1], x_off[1:])]
    t_stft = [stft_num_frames(n, n_fft, hop) for n in lens]
    if world_streams:
        t_world = [num_frames(n, fs, hop_ms) for n in lens]
        if any(a < b for a, b in zip(t_stft, t_world)):
            raise NotImplementedError("STFT hop {} gives fewer frames than WORLD's {} ms grid.".format(hop, hop_ms))
        first = [(a - b) // 2 for a, b in zip(t_stft, t_world)]      # trim_to_shortest: diff // 2 in front
        f_off = offsets(t_world)
    else:
        first = [0] * len(lens)
        f_off = offsets(t_stft)
    main = torch.cuda.current_stream(dev)
    if world_streams:
        f0 = estimate_f0(x, x_off, f_off, fs, hop_ms, f0_method)
        side = _side_stream(dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            _, bap = ops.d4c(x, x_off, f0, f_off, fs, hop_ms, n_fft, want_ap=False, want_bap=torch.float32)
            lf0, vuv = ops.lf0_vuv(f0, f_off, f0_silence_threshold, lf0_zero)
    sp = stft_features(x, x_off, f_off, first, fs, sp_type, n_fft, hop, n_mels, win_length)
    if world_streams:
        main.wait_stream(side)
        for t in (x, f0, bap, lf0, vuv):
            t.record_stream(side)
            t.record_stream(main)
    else:       # WORLD does not run: the columns of its streams are left at zero (gen_data writes none of them)
        n_rows = f_off[-1]
        lf0 = torch.zeros(n_rows, dtype=torch.float32, device=dev)
        vuv = torch.zeros(n_rows, dtype=torch.float32, device=dev)
        bap = torch.zeros((n_rows, _lib.load().itts_num_aperiodicities(int(fs))), dtype=torch.float32, device=dev)
    return ops.assemble_cmp(sp, lf0, vuv, bap, f_off, add_deltas=add_deltas), f_off


class StreamStats(object):
    """Normalisation sums of the continuous streams (coded sp, lf0, bap) of a feature matrix,
    accumulated on the device over the batches of a gen_data run (fp64, fixed summation order):
    what MeanCovarianceExtractor / MeanStdDevExtractor.add_sample gather utterance by utterance
    (misc/normalisation/*.py).  `columns`: {stream name: (first column, width)}."""

    def __init__(self, columns, want_cov):
        self.columns = dict(columns)
        self.want_cov = bool(want_cov)
        self.count = 0
        self.sums = {}

    def add(self, cmp_dev):
        for name, (c0, w) in self.columns.items():
            if w == 0:
                continue
            acc = self.sums.get(name)
            if acc is None:
                self.sums[name] = ops.feature_stats(cmp_dev, c0, w, self.want_cov)
            else:
                ops.feature_stats(cmp_dev, c0, w, self.want_cov, sums=acc[0], second=acc[1])
        self.count += int(cmp_dev.shape[0])

    def store(self, name, extractor):
        """Hands the sums of one stream to an extractor (adds to what it already holds)."""
        if name not in self.sums:
            return
        first, second = (t.cpu().numpy() for t in self.sums[name])
        extractor.add_sums(self.count, first[None, :] if self.want_cov else first, second)


def extract_cmp_batch(raws, fs, hop_ms=5.0, n_fft=None, mcep_order=59, mcep_alpha=None,
                      f0_silence_threshold=30, lf0_zero=0, add_deltas=True, device=None,
                      mgc_gamma=None, f0_method="dio", sp_type=None, num_coded_sps=None, win_length_ms=None,
                      world_streams=True):
    """wav(s) -> the `[T, 3*(ncs+1+nb)+1]` feature matrix of the reference's gen_data in one go,
    everything on the device: DIO + StoneMask, D4C -> coded bap, CheapTrick -> mcep, lf0 / V-UV
    with interpolate_lin, deltas and the stream layout (WorldFeatLabelGen.py:778-807, 809-889,
    1121-1172).  Returns (cmp [Ttot, W] f32 on the device, frame offsets [U+1]).
    sp_type "mfbanks" (num_coded_sps bands), "amp_sp" or "log_amp_sp" put librosa's STFT features where the
    mel-cepstra go (WorldFeatLabelGen.py:865-874; CheapTrick and mcep do not run): with `world_streams` trimmed
    to the WORLD frame count like trim_to_shortest (:891-907), without them WORLD does not run at all and the
    lf0 / vuv / bap columns are zeros."""
    if sp_type in STFT_SP_TYPES:
        n_fft = n_fft or fs_to_frame_length(fs)
        check_stft_args(n_fft)
    dev = _device(device)
    L = _lib.load()
    n_fft = n_fft or L.itts_cheaptrick_fft_size(int(fs), 71.0)
    if isinstance(raws, tuple):       # (samples of all utterances back to back, sample offsets)
        samples, x_off = raws
        x_off = [int(o) for o in x_off]
    else:
        x_off = offsets([len(r) for r in raws])
        samples = np.concatenate(raws) if len(raws) else np.empty(0)
    if isinstance(samples, torch.Tensor):     # float64 samples of gen_data's readers: page-locked (fetched asynchronously)
        x = samples if samples.is_cuda else samples.to(dev, non_blocking=True)     # or uploaded by the reader already
    else:
        x = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float64)).to(dev)
    if sp_type in STFT_SP_TYPES:
        return _extract_cmp_stft(x, x_off, fs, hop_ms, n_fft, sp_type, num_coded_sps, win_length_ms,
                                 world_streams, f0_silence_threshold, lf0_zero, add_deltas, f0_method)
    f_off = offsets([num_frames(b - a, fs, hop_ms) for a, b in zip(x_off[:-1], x_off[1:])])
    f0 = estimate_f0(x, x_off, f_off, fs, hop_ms, f0_method)
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        _, bap = ops.d4c(x, x_off, f0, f_off, fs, hop_ms, n_fft, want_ap=False,
                         want_bap=torch.float32)
        lf0, vuv = ops.lf0_vuv(f0, f_off, f0_silence_threshold, lf0_zero)
    if mgc_gamma is None or mgc_gamma == 0.0:
        _, mc, _ = ops.cheaptrick_mcep(x, x_off, f0, f_off, fs, hop_ms, n_fft, want_sp=False,
                                       order=mcep_order, alpha=mcep_alpha)
    else:       # sp_type "mgc": mel-generalized cepstrum of the CheapTrick envelope
        sp, _, _ = ops.cheaptrick_mcep(x, x_off, f0, f_off, fs, hop_ms, n_fft, want_sp=True)
        mc = ops.mgcep(sp, mcep_order, mcep_alpha, mgc_gamma, input_is_power=True)
    main.wait_stream(side)
    for t in (x, f0, bap, lf0, vuv):
        t.record_stream(side)
        t.record_stream(main)
    return ops.assemble_cmp(mc, lf0, vuv, bap, f_off, add_deltas=add_deltas), f_off


def synthesise_features(f0, f_off, fs, n_fft, mc=None, alpha=None, sp=None, bap=None, ap=None, hop_ms=5.0,
                        preemphasis=0.0, dtype=torch.float32):
    """Device tensors in, waveform out: f0 [Ttot] f64 of utterances stored back to back, the envelope as mel-cepstra
    `mc` [Ttot, order + 1] f64 (with `alpha`) or as power spectra `sp`, the aperiodicity coded (`bap`) or decoded (`ap`).
    What has to be decoded first -- mc -> sp (WorldFeatLabelGen.py:925 through mgc2sp), bap -> ap (:940-941) -- runs on
    the side stream WHILE the synthesis works through everything it does on f0 alone (per-sample phase, pulse positions,
    noise): the two [Ttot, K] arrays are only needed by the pulse kernel.  Returns (y [Ytot], y_off)."""
    dev = f0.device
    main = torch.cuda.current_stream(dev)
    ready = ap_ready = None
    y_off = ops.synth_offsets(f_off, fs, hop_ms)      # (host work first: nothing between the two streams' launches)
    if mc is not None or ap is None:
        side = _side_stream(dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            # (the envelope first -- the kernel of the unvoiced pulses waits for it alone --, the decode behind it with
            # an event of its own for the kernel of the voiced ones)
            if mc is not None:
                sp = ops.mgc2sp(mc, alpha, n_fft, want_pow=True)
            ready = torch.cuda.Event()
            ready.record(side)
            if ap is None:
                ap = ops.decode_aperiodicity(bap, fs, n_fft, voiced_f0=f0)      # (only the rows a voiced pulse reads)
                ap_ready = torch.cuda.Event()
                ap_ready.record(side)
        for t in (mc, bap, f0):
            if t is not None:
                t.record_stream(side)
    return ops.world_synthesize(f0, sp, ap, f_off, fs, hop_ms, preemphasis, dtype=dtype, spectra_ready=ready,
                                y_off=y_off, ap_ready=ap_ready)


def synthesise_batch(f0s, sps, baps, fs, n_fft, hop_ms=5.0, preemphasis=0.0, device=None,
                     out_dtype=np.float64, sp_is_amplitude=False):
    """f0s: list of [T] f64; sps: list of [T,K] f64 POWER spectra -- or, with `sp_is_amplitude`, amplitude spectra
    of any float type, widened and squared on the device after the upload (np.square(amp_sp, dtype=float64) of
    WorldFeatLabelGen.py:925: the same bits) --; baps: list of [T,nap] f64 coded
    aperiodicity. Returns list of waveforms (float32 samples; float64 container when
    out_dtype is float64, like scipy.signal.lfilter gives the reference)."""
    dev = _device(device)
    f_off = offsets([len(f) for f in f0s])
    f0 = torch.from_numpy(np.ascontiguousarray(np.concatenate(f0s), dtype=np.float64)).to(dev)
    if sp_is_amplitude:
        host = sps[0] if len(sps) == 1 else np.concatenate(sps)
        sp = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
        if sp.dtype != torch.float64:
            sp = sp.double()
        ops.square_inplace(sp)
    else:
        sp = torch.from_numpy(np.ascontiguousarray(np.concatenate(sps), dtype=np.float64)).to(dev)
    bap = torch.from_numpy(np.ascontiguousarray(np.concatenate(baps), dtype=np.float64)).to(dev)
    y, y_off = synthesise_features(f0, f_off, fs, n_fft, sp=sp, bap=bap, hop_ms=hop_ms, preemphasis=preemphasis,
                                   dtype=torch.float64 if out_dtype == np.float64 else torch.float32)
    y = y.cpu().numpy()
    return [y[y_off[u]:y_off[u + 1]] for u in range(len(f0s))]
