"""Thin tensor-level wrappers over the C ABI (torch is used for device memory and streams only).

Every function takes CUDA(HIP) tensors, passes raw device pointers + the current HIP stream to
libidiaptts_amd.so and raises on any failure.  Nothing here computes on the CPU.
"""
import collections
import contextlib
import ctypes
import threading

import torch

from . import lib as _lib

# activation codes of the dense layers (ITTS_ACT_* in include/idiaptts_amd.h)
ACT_NONE, ACT_TANH, ACT_RELU = 0, 1, 2
(ACT_SIGMOID, ACT_LOGSIGMOID, ACT_SOFTPLUS, ACT_SOFTSIGN, ACT_LEAKY_RELU, ACT_ELU, ACT_CELU, ACT_SELU, ACT_HARDTANH,
 ACT_RELU6, ACT_HARDSIGMOID) = range(3, 14)
# the torch.nn module each code stands for (with its default arguments): FFWrapper's `nonlin` names
ACT_TORCH_NAME = {ACT_TANH: "Tanh", ACT_RELU: "ReLU", ACT_SIGMOID: "Sigmoid", ACT_LOGSIGMOID: "LogSigmoid",
                  ACT_SOFTPLUS: "Softplus", ACT_SOFTSIGN: "Softsign", ACT_LEAKY_RELU: "LeakyReLU", ACT_ELU: "ELU",
                  ACT_CELU: "CELU", ACT_SELU: "SELU", ACT_HARDTANH: "Hardtanh", ACT_RELU6: "ReLU6",
                  ACT_HARDSIGMOID: "Hardsigmoid"}
# lower-case names (and None / "none" / "linear": no activation) -> code
ACT_BY_NAME = {None: ACT_NONE, "none": ACT_NONE, "linear": ACT_NONE}
ACT_BY_NAME.update({name.lower(): code for code, name in ACT_TORCH_NAME.items()})
CONV_ACTS = (ACT_NONE, ACT_TANH, ACT_RELU)     # what the Conv1d kernels fuse


def act_code(act, allowed=None, where="Linear"):
    """ops.ACT_* of an activation name (any case) or code; NotImplementedError naming it when it is not one of
    `allowed` (default: every code)"""
    code = act if isinstance(act, int) else ACT_BY_NAME.get(act.lower() if isinstance(act, str) else act)
    if code is None or code not in (allowed if allowed is not None else range(ACT_HARDSIGMOID + 1)):
        raise NotImplementedError("{} activation {!r} is not implemented".format(where, act))
    return code


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    # (the raw handle straight from the runtime: `torch.cuda.current_stream().cuda_stream` builds a Stream object
    # on every call, 12 us of the host's ~40 per launch on the module path)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _need(t, dtype, name):
    if not t.is_cuda:
        raise _lib.IttsError("{} must live on the GPU (no CPU fallback)".format(name))
    if t.dtype != dtype:
        raise TypeError("{} must be {}, got {}".format(name, dtype, t.dtype))


def _rows(t, name):
    """2-D view contract: unit stride on the last dim, arbitrary row stride."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("{} must be 2-D with contiguous rows".format(name))
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


# ---------------------------------------------------------------------------------------- MLPG
class MlpgPlan(object):
    """What `mlpg_generation` works out from the offsets alone (checks, longest length, the one-pass kernel's table in
    launch order), prepared once for callers that solve over the same utterances again -- the streams of a batch, a
    fixed validation set: a planned call then does nothing on the host but launch (40-50 us of a 260-us lone call
    otherwise).  The scratch buffer of the largest call so far is kept as well."""

    def __init__(self, offsets):
        L = _lib.load()
        offs = _lib.offsets_array(offsets)
        self.n_utts = len(offs) - 1
        self.t_total = int(offs[self.n_utts]) if self.n_utts >= 0 else 0
        handle = ctypes.c_void_p()
        _lib.check(L.itts_mlpg_plan_create(offs, self.n_utts, ctypes.byref(handle)), "itts_mlpg_plan_create")
        self._handle = handle
        self._scratch = None

    def scratch(self, nbytes, device):
        if self._scratch is None or self._scratch.numel() < nbytes or self._scratch.device != device:
            self._scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device)
        return self._scratch

    def close(self):
        handle, self._handle = self._handle, None
        if handle is not None:
            if torch.cuda.is_available():
                torch.cuda.synchronize()          # (launches read the plan's table in place)
            _lib.load().itts_mlpg_plan_destroy(handle)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def mlpg_generation(feat, variances, dim, offsets, col0=0, out=None, ocol0=0, plan=None):
    """Batched MLPG (misc/mlpg.py:94-127). feat [Ttot, >=col0+3*dim] f64 -- or f32, the acoustic model's own output
    type: widened in the solve's loads, the result is that of the f64 rows --, variances [3*dim] f64,
    offsets: python list of U+1 frame offsets (ignored with `plan`, an MlpgPlan made from them). Returns out
    [Ttot, dim] f64 (or writes into out)."""
    L = _lib.load()
    f32 = feat.dtype == torch.float32
    _need(feat, torch.float32 if f32 else torch.float64, "feat")
    _need(variances, torch.float64, "variances")
    ld = _rows(feat, "feat")
    t_total = plan.t_total if plan is not None else int(offsets[-1])
    if feat.shape[0] != t_total:
        raise ValueError("offsets[-1] != number of rows")
    if out is None:
        out = torch.empty((t_total, dim), dtype=torch.float64, device=feat.device)
    _need(out, torch.float64, "out")
    ldo = _rows(out, "out")
    nbytes = (L.itts_mlpg_scratch_bytes_f32 if f32 else L.itts_mlpg_scratch_bytes)(t_total, dim)
    if not variances.is_contiguous():
        variances = variances.contiguous()
    if plan is not None:
        scratch = plan.scratch(nbytes, feat.device)
        _lib.check(L.itts_mlpg_generation_planned(plan._handle, _ptr(feat), 1 if f32 else 0, ld, col0, dim,
                                                  _ptr(variances), _ptr(out), ldo, ocol0, _ptr(scratch), _stream()),
                   "itts_mlpg_generation_planned")
        return out
    scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=feat.device)
    offs = _lib.offsets_array(offsets)
    entry = L.itts_mlpg_generation_f32 if f32 else L.itts_mlpg_generation
    _lib.check(entry(_ptr(feat), ld, col0, dim, _ptr(variances),
                     offs, len(offsets) - 1, _ptr(out), ldo, ocol0,
                     _ptr(scratch), _stream()), "itts_mlpg_generation")
    return out


def mlpg_adjoint(gout, variances, dim, offsets, gcol0=0, out=None, col0=0, plan=None):
    """The gradient with respect to the static / delta / delta-delta means from the gradient with respect to the
    trajectory (itts_mlpg_adjoint): gout [Ttot, >= gcol0 + dim] f32 or f64, variances [3*dim] f64, offsets / plan as
    for `mlpg_generation`.  Writes columns col0 .. col0 + 3*dim - 1 of `out` (f32 or f64, nothing else of it is
    touched) and returns it; without `out` a [Ttot, 3*dim] tensor of gout's dtype."""
    L = _lib.load()
    if gout.dtype not in (torch.float32, torch.float64):
        raise TypeError("gout must be float32 or float64, got {}".format(gout.dtype))
    _need(gout, gout.dtype, "gout")
    _need(variances, torch.float64, "variances")
    if variances.numel() != 3 * dim:
        raise ValueError("variances must hold 3 * dim = {} values, got {}".format(3 * dim, variances.numel()))
    ldg = _rows(gout, "gout")
    t_total = plan.t_total if plan is not None else int(offsets[-1])
    if gout.shape[0] != t_total:
        raise ValueError("offsets[-1] != number of rows")
    if gcol0 < 0 or gout.shape[1] < gcol0 + dim:
        raise ValueError("gout has no columns {} .. {}".format(gcol0, gcol0 + dim - 1))
    if out is None:
        out = torch.empty((t_total, 3 * dim), dtype=gout.dtype, device=gout.device)
    if out.dtype not in (torch.float32, torch.float64):
        raise TypeError("out must be float32 or float64, got {}".format(out.dtype))
    _need(out, out.dtype, "out")
    ldo = _rows(out, "out")
    if out.shape[0] != t_total or col0 < 0 or out.shape[1] < col0 + 3 * dim:
        raise ValueError("out must hold {} rows and columns {} .. {}".format(t_total, col0, col0 + 3 * dim - 1))
    nbytes = L.itts_mlpg_adjoint_scratch_bytes(t_total, dim)
    if not variances.is_contiguous():
        variances = variances.contiguous()
    g32, o32 = int(gout.dtype == torch.float32), int(out.dtype == torch.float32)
    if plan is not None:
        scratch = plan.scratch(nbytes, gout.device)
        _lib.check(L.itts_mlpg_adjoint_planned(plan._handle, _ptr(gout), g32, ldg, gcol0, dim, _ptr(variances),
                                               _ptr(out), o32, ldo, col0, _ptr(scratch), _stream()),
                   "itts_mlpg_adjoint_planned")
        return out
    scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=gout.device)
    offs = _lib.offsets_array(offsets)
    _lib.check(L.itts_mlpg_adjoint(_ptr(gout), g32, ldg, gcol0, dim, _ptr(variances), offs, len(offsets) - 1,
                                   _ptr(out), o32, ldo, col0, _ptr(scratch), _stream()), "itts_mlpg_adjoint")
    return out


# the form a call solves in (ITTS_MLPG_FORM_*, include/idiaptts_amd.h): one of the three solves, or-ed with flags
MLPG_SWEEPS, MLPG_STREAM, MLPG_RING, MLPG_SOLVE_MASK = 1, 2, 3, 3
MLPG_WIDE, MLPG_F32_ROWS, MLPG_NT_IN, MLPG_WIDENED_COPY = 4, 8, 16, 32
_FORCE_OFF, _FORCE_ON = 1, 2
_MLPG_SOLVES = {None: 0, "auto": 0, "stream": MLPG_STREAM, "ring": MLPG_RING}
_MLPG_WIDTHS = {None: 0, "auto": 0, "narrow": _FORCE_OFF, "wide": _FORCE_ON}
_MLPG_NT = {None: 0, "auto": 0, False: _FORCE_OFF, True: _FORCE_ON}


def mlpg_form_name(form):
    """'ring wide f32', 'stream f32 widened', ... for a form code."""
    if form <= 0:
        return "none" if form == 0 else "invalid"
    words = [{MLPG_SWEEPS: "sweeps", MLPG_STREAM: "stream", MLPG_RING: "ring"}[form & MLPG_SOLVE_MASK]]
    for bit, word in ((MLPG_WIDE, "wide"), (MLPG_F32_ROWS, "f32"), (MLPG_NT_IN, "nt-in"),
                      (MLPG_WIDENED_COPY, "widened")):
        if form & bit:
            words.append(word)
    return " ".join(words)


def mlpg_choose_form(n_utts, dim, t_max, t_total, rows_f32=False):
    """The form `mlpg_generation` takes for such a batch under the current override (itts_mlpg_choose_form)."""
    form = _lib.load().itts_mlpg_choose_form(n_utts, dim, t_max, t_total, 1 if rows_f32 else 0)
    if form < 0:
        _lib.check(form, "itts_mlpg_choose_form")
    return form


def mlpg_last_form():
    """The form of this thread's last `mlpg_generation` call (0: none, or nothing to solve)."""
    return _lib.load().itts_mlpg_last_form()


@contextlib.contextmanager
def mlpg_forced(solve=None, width=None, nt=None):
    """Forces parts of the choice of form for the calls inside (process-wide); the previous override comes back on
    exit.  solve: None / "auto", "stream", "ring"; width: None / "auto", "narrow", "wide"; nt: None / "auto", False,
    True (non-temporal input loads of the float64 ring).  None leaves that part to the library."""
    L = _lib.load()
    prev = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int()]
    _lib.check(L.itts_mlpg_get_override(*[ctypes.byref(p) for p in prev]), "itts_mlpg_get_override")
    try:
        codes = (_MLPG_SOLVES[solve], _MLPG_WIDTHS[width], _MLPG_NT[nt])
    except KeyError:
        raise ValueError("mlpg_forced(solve={!r}, width={!r}, nt={!r})".format(solve, width, nt))
    _lib.check(L.itts_mlpg_set_override(*codes), "itts_mlpg_set_override")
    try:
        yield
    finally:
        _lib.check(L.itts_mlpg_set_override(*[p.value for p in prev]), "itts_mlpg_set_override")


def mlpg_adjoint_choose_form(n_utts, dim, t_max, t_total):
    """The form `mlpg_adjoint` takes for such a batch under the adjoint's override: MLPG_SWEEPS or MLPG_STREAM
    (itts_mlpg_adjoint_choose_form)."""
    form = _lib.load().itts_mlpg_adjoint_choose_form(n_utts, dim, t_max, t_total)
    if form < 0:
        _lib.check(form, "itts_mlpg_adjoint_choose_form")
    return form


def mlpg_adjoint_last_form():
    """The form of this thread's last `mlpg_adjoint` call (0: none, or nothing to solve)."""
    return _lib.load().itts_mlpg_adjoint_last_form()


@contextlib.contextmanager
def mlpg_adjoint_forced(form):
    """Forces the form of the `mlpg_adjoint` calls inside, whatever their lengths (process-wide; the forward's override
    is another word); the previous value comes back on exit.  form: None / 0 / "auto", MLPG_SWEEPS / "sweeps",
    MLPG_STREAM / "stream"."""
    L = _lib.load()
    code = {None: 0, "auto": 0, "sweeps": MLPG_SWEEPS, "stream": MLPG_STREAM}.get(form, form)
    if isinstance(code, bool) or code not in (0, MLPG_SWEEPS, MLPG_STREAM):
        raise ValueError("mlpg_adjoint_forced({!r})".format(form))
    prev = L.itts_mlpg_adjoint_get_override()
    _lib.check(L.itts_mlpg_adjoint_set_override(code), "itts_mlpg_adjoint_set_override")
    try:
        yield
    finally:
        _lib.check(L.itts_mlpg_adjoint_set_override(prev), "itts_mlpg_adjoint_set_override")


def lf0_vuv(f0, offsets, f0_silence_threshold=30.0, lf0_zero=0.0):
    """f0 [Ttot] f64 -> (lf0 [Ttot] f32 interpolated, vuv [Ttot] f32): WorldFeatLabelGen.py:798-802
    (float32 log, threshold, interpolate_lin) per utterance."""
    L = _lib.load()
    _need(f0, torch.float64, "f0")
    f0 = f0.contiguous()
    lf0 = torch.empty(f0.shape[0], dtype=torch.float32, device=f0.device)
    vuv = torch.empty_like(lf0)
    _lib.check(L.itts_lf0_vuv(_ptr(f0), _lib.offsets_array(offsets), len(offsets) - 1,
                              float(f0_silence_threshold), float(lf0_zero), _ptr(lf0), _ptr(vuv),
                              _stream()), "itts_lf0_vuv")
    return lf0, vuv


# ----------------------------------------------------------------------------------------- STFT
STFT_PAD = {None: 0, "reflect": 1, "constant": 2}     # pad_mode of librosa.stft; None: center=False
STFT_KIND = {"amp_sp": 0, "amp_sp_f64": 1, "log_amp_sp": 2}


def _stft_offsets(x_off, f_off, first):
    return _lib.offsets_array(x_off), _lib.offsets_array(f_off), _lib.offsets_array(first)


def stft_amp(x, x_off, f_off, first, n_fft, hop, pad, window, kind="amp_sp", out=None):
    """|librosa.stft| / sqrt(n_fft // 2 + 1) of the float64 samples x (utterances at x_off), one row per frame:
    row f_off[u] + i is STFT frame first[u] + i of utterance u.  pad: None (center=False), "reflect" or
    "constant"; window: float64 [n_fft] on the device.  kind "amp_sp" (float32), "amp_sp_f64" or "log_amp_sp"
    (20 log10(max(1e-5, amplitude)), float32).  Returns [f_off[-1], n_fft // 2 + 1]."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    _need(window, torch.float64, "window")
    K = n_fft // 2 + 1
    if out is None:
        out = torch.empty((int(f_off[-1]), K), device=x.device,
                          dtype=torch.float64 if kind == "amp_sp_f64" else torch.float32)
    _need(out, torch.float64 if kind == "amp_sp_f64" else torch.float32, "out")
    xo, fo, fi = _stft_offsets(x_off, f_off, first)
    _lib.check(L.itts_stft(_ptr(x), xo, fo, fi, len(x_off) - 1, int(n_fft), int(hop), STFT_PAD[pad], _ptr(window),
                           STFT_KIND[kind], _ptr(out), _rows(out, "out"), _stream()), "itts_stft")
    return out


def mel_filterbank(x, x_off, f_off, first, n_fft, hop, pad, window, mel_tab, mel_w, n_mels, out=None):
    """mel_basis @ stft_amp(...).T per frame, float32 [f_off[-1], n_mels], with the spectrum kept on the chip.
    mel_tab int32 [3 n_mels] (first bin, bins, first weight per filter) and mel_w float32: world.mel_tables."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    _need(window, torch.float64, "window")
    _need(mel_tab, torch.int32, "mel_tab")
    _need(mel_w, torch.float32, "mel_w")
    if out is None:
        out = torch.empty((int(f_off[-1]), n_mels), device=x.device, dtype=torch.float32)
    _need(out, torch.float32, "out")
    xo, fo, fi = _stft_offsets(x_off, f_off, first)
    _lib.check(L.itts_stft_mel(_ptr(x), xo, fo, fi, len(x_off) - 1, int(n_fft), int(hop), STFT_PAD[pad],
                               _ptr(window), _ptr(mel_tab), _ptr(mel_w), int(n_mels), _ptr(out), _rows(out, "out"),
                               _stream()), "itts_stft_mel")
    return out


def griffinlim(S, angles, f_off, n_fft, hop, pad, window, n_iter, momentum):
    """librosa.griffinlim on the amplitude spectra S [f_off[-1], n_fft // 2 + 1] (float32 or float64) of utterances
    stored back to back, from the initial phases `angles` (complex64 / complex128 of S's precision, same shape;
    overwritten).  pad: "reflect" or "constant"; window: float64 [n_fft] on the device.  Returns the waveforms
    back to back, hop (T_u - 1) samples each, in S's dtype."""
    L = _lib.load()
    f64 = S.dtype == torch.float64
    _need(S, torch.float64 if f64 else torch.float32, "S")
    _need(angles, torch.complex128 if f64 else torch.complex64, "angles")
    _need(window, torch.float64, "window")
    K = n_fft // 2 + 1
    rows = int(f_off[-1])
    if tuple(S.shape) != (rows, K) or tuple(angles.shape) != (rows, K) or not (S.is_contiguous()
                                                                              and angles.is_contiguous()):
        raise ValueError("S and angles must be contiguous [{}, {}]".format(rows, K))
    ang_b = torch.empty_like(angles)
    tprev = torch.empty_like(angles)
    y = torch.empty(sum((b - a - 1) * int(hop) for a, b in zip(f_off[:-1], f_off[1:])), dtype=S.dtype,
                    device=S.device)
    _lib.check(L.itts_griffinlim(_ptr(S), _ptr(angles), _ptr(ang_b), _ptr(tprev), _lib.offsets_array(f_off),
                                 len(f_off) - 1, int(n_fft), int(hop), STFT_PAD[pad], _ptr(window), int(n_iter),
                                 float(momentum), int(f64), _ptr(y), _stream()), "itts_griffinlim")
    return y


def mel_inverse(mel, n_fft, bin_j, bin_w, filt, pinv_t, inv_lipschitz, tol, max_iter, check_every, out_dtype,
                iters=None):
    """NNLS inversion of the mel filter banks mel [F, n_mels] (float32 or float64 rows) on the tables of
    world.mel_inverse_tables -> K x [F, n_fft // 2 + 1] in out_dtype (float32 / float64).  iters: an int32 [F]
    tensor that receives the iterations each frame took, or None."""
    L = _lib.load()
    if mel.dtype not in (torch.float32, torch.float64):
        raise TypeError("mel must be float32 or float64, got {}".format(mel.dtype))
    _need(mel, mel.dtype, "mel")
    _need(bin_j, torch.int32, "bin_j")
    _need(bin_w, torch.float64, "bin_w")
    _need(filt, torch.int32, "filt")
    _need(pinv_t, torch.float64, "pinv_t")
    ld = _rows(mel, "mel")
    F, n_mels = mel.shape
    K = n_fft // 2 + 1
    out = torch.empty((F, K), dtype=out_dtype, device=mel.device)
    if iters is not None:
        _need(iters, torch.int32, "iters")
        if iters.numel() != F or not iters.is_contiguous():
            raise ValueError("iters must be a contiguous int32 tensor of {} elements".format(F))
    _lib.check(L.itts_mel_inverse(_ptr(mel), F, n_mels, ld, int(mel.dtype == torch.float64), int(n_fft), _ptr(bin_j),
                                  _ptr(bin_w), _ptr(filt), _ptr(pinv_t), float(inv_lipschitz), float(tol),
                                  int(max_iter), int(check_every), _ptr(out), K, int(out_dtype == torch.float64),
                                  _ptr(iters), _stream()), "itts_mel_inverse")
    return out


def mel_project(amp, mel_tab, mel_w, n_mels, out=None):
    """The mel projection of a given amplitude spectrum amp [T, K] float64 -> float32 [T, n_mels]."""
    L = _lib.load()
    _need(amp, torch.float64, "amp")
    _need(mel_tab, torch.int32, "mel_tab")
    _need(mel_w, torch.float32, "mel_w")
    if out is None:
        out = torch.empty((amp.shape[0], n_mels), device=amp.device, dtype=torch.float32)
    _lib.check(L.itts_mel_project(_ptr(amp), amp.shape[0], amp.shape[1], _rows(amp, "amp"), _ptr(mel_tab),
                                  _ptr(mel_w), int(n_mels), _ptr(out), _rows(out, "out"), _stream()),
               "itts_mel_project")
    return out


def sqrt_inplace(x):
    """x <- sqrt(x) for a contiguous float64 tensor (IEEE square roots: numpy's bits)."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    assert x.is_contiguous()
    _lib.check(L.itts_sqrt_inplace_f64(_ptr(x), x.numel(), _stream()), "itts_sqrt_inplace_f64")
    return x


def square_inplace(x):
    """x <- x * x for a contiguous float64 tensor (one IEEE product per value: numpy's bits)."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    assert x.is_contiguous()
    _lib.check(L.itts_square_inplace_f64(_ptr(x), x.numel(), _stream()), "itts_square_inplace_f64")
    return x


def interpolate_lin_f32(x, offsets):
    """interpolate_lin (misc/utils.py:40-86) on float32 contours stored back to back:
    (interpolated [Ttot], vuv [Ttot])."""
    L = _lib.load()
    _need(x, torch.float32, "x")
    x = x.contiguous()
    ip = torch.empty_like(x)
    vuv = torch.empty_like(x)
    _lib.check(L.itts_interpolate_lin_f32(_ptr(x), _lib.offsets_array(offsets), len(offsets) - 1,
                                          _ptr(ip), _ptr(vuv), _stream()),
               "itts_interpolate_lin_f32")
    return ip, vuv


def assemble_cmp(sp, lf0, vuv, bap, offsets, add_deltas=True, out=None):
    """[sp, d, dd | lf0, d, dd | vuv | bap, d, dd] (or the static layout) per frame, float32
    (save_output WorldFeatLabelGen.py:1121-1172 + compute_deltas misc/utils.py:103-105)."""
    L = _lib.load()
    for t, n in ((sp, "sp"), (lf0, "lf0"), (vuv, "vuv"), (bap, "bap")):
        _need(t, torch.float32, n)
    n_sp, n_bap = sp.shape[1], bap.shape[1]
    width = (3 if add_deltas else 1) * (n_sp + 1 + n_bap) + 1
    if out is None:
        out = torch.empty((sp.shape[0], width), dtype=torch.float32, device=sp.device)
    _lib.check(L.itts_assemble_cmp_f32(_ptr(sp), _rows(sp, "sp"), n_sp, _ptr(lf0.contiguous()),
                                       _ptr(vuv.contiguous()), _ptr(bap), _rows(bap, "bap"), n_bap,
                                       _lib.offsets_array(offsets), len(offsets) - 1,
                                       1 if add_deltas else 0, _ptr(out), _rows(out, "out"),
                                       _stream()), "itts_assemble_cmp_f32")
    return out


def feature_stats(x, col0, width, want_cov, sums=None, second=None):
    """sum x [width] and sum x x^T [width, width] (want_cov) or sum x^2 [width] over the rows of
    x[:, col0:col0+width] in fp64; adds to `sums` / `second` when given."""
    L = _lib.load()
    _need(x, torch.float32, "x")
    accumulate = sums is not None
    if sums is None:
        sums = torch.empty(width, dtype=torch.float64, device=x.device)
        second = torch.empty((width, width) if want_cov else (width,), dtype=torch.float64,
                             device=x.device)
    ws = _workspace(L.itts_feature_stats_workspace_bytes(width, 1 if want_cov else 0), x.device)
    _lib.check(L.itts_feature_stats(_ptr(x), _rows(x, "x"), x.shape[0], col0, width,
                                    1 if want_cov else 0, 1 if accumulate else 0, _ptr(sums),
                                    _ptr(second), _ptr(ws), _stream()), "itts_feature_stats")
    return sums, second


# ------------------------------------------------------------------------------ dense layers
# Each product below is written once, for the plain entry point and for its _dropout form: `drop` is None, or the rule
# as _drop_args(p, seed, salt, row_offset) gives it, which goes in front of the stream.
def _linear_fwd(x, w, b, act, out, drop):
    L = _lib.load()
    _need(x, torch.float32, "x")
    _need(w, torch.float32, "w")
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K or not w.is_contiguous():
        raise ValueError("w must be contiguous [N, K]")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    args = (_ptr(x), _rows(x, "x"), _ptr(w), _ptr(b), _ptr(out), _rows(out, "out"), M, N, K, act, _stream())
    if drop is None:
        _lib.check(L.itts_linear_fwd(*args), "itts_linear_fwd")
    else:
        _lib.check(L.itts_linear_fwd_dropout(*args[:-1], *drop, args[-1]), "itts_linear_fwd_dropout")
    return out


def linear_fwd(x, w, b, act=ACT_NONE, out=None):
    return _linear_fwd(x, w, b, act, out, None)


class SparseRows(object):
    """Row lists of a sparse [M, K] matrix (itts_sparse_rows_build): per row the (k, value) pairs of its non-zeros
    in ascending k, in one device block that the caller owns (it must live as long as the lists are used, so it
    is never the shared workspace).  A block is reused for any shape it is large enough for."""

    def __init__(self, M, K, device, block=None):
        out = (ctypes.c_int64 * 4)()
        _lib.check(_lib.load().itts_sparse_rows_layout(M, K, out), "itts_sparse_rows_layout")
        self.M, self.K = int(M), int(K)
        self._counts_off, self._entries_off, self.pitch, self.nbytes = (int(v) for v in out)
        if block is None or block.numel() < self.nbytes:
            block = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        self.block = block

    def counts(self):
        """int32 [M]: non-zeros per row"""
        return self.block[self._counts_off:self._counts_off + 4 * self.M].view(torch.int32)

    def entries(self):
        """int32 [M, pitch, 2]: (k, bits of the float32 value); row m holds counts()[m] of them, then neutral (K, +0.0)
        entries up to the next multiple of 8, then nothing defined"""
        n = 8 * self.M * self.pitch
        return self.block[self._entries_off:self._entries_off + n].view(torch.int32).view(self.M, self.pitch, 2)

    def record(self):
        """(total non-zeros, largest count of a row) of a build with want_record=True; reads the device (one
        synchronisation)"""
        total, most = self.block[:16].view(torch.int64).tolist()
        return total, most

    def density(self):
        return self.record()[0] / float(max(self.M * self.K, 1))


def sparse_rows_build(x, K=None, lists=None, want_record=True):
    """Row lists of the first K (default: all) columns of x [M, >= K] fp32; `lists`: a SparseRows whose block is
    reused when it is large enough."""
    _need(x, torch.float32, "x")
    ldx = _rows(x, "x")
    M = x.shape[0]
    K = x.shape[1] if K is None else int(K)
    if K > x.shape[1]:
        raise ValueError("K exceeds the width of x")
    rows = SparseRows(M, K, x.device, lists.block if lists is not None else None)
    _lib.check(_lib.load().itts_sparse_rows_build(_ptr(x), ldx, M, K, _ptr(rows.block), 1 if want_record else 0,
                                                  _stream()), "itts_sparse_rows_build")
    return rows


def _linear_fwd_sparse(rows, x, w, b, act, out, drop):
    L = _lib.load()
    _need(x, torch.float32, "x")
    _need(w, torch.float32, "w")
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K or not w.is_contiguous():
        raise ValueError("w must be contiguous [N, K]")
    if rows.M != M or rows.K != K:
        raise ValueError("the row lists were built for another shape")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    args = (_ptr(rows.block), _ptr(x), _rows(x, "x"), _ptr(w), _ptr(b), _ptr(out), _rows(out, "out"), M, N, K, act,
            _stream())
    if drop is None:
        _lib.check(L.itts_linear_fwd_sparse(*args), "itts_linear_fwd_sparse")
    else:
        _lib.check(L.itts_linear_fwd_sparse_dropout(*args[:-1], *drop, args[-1]), "itts_linear_fwd_sparse_dropout")
    return out


def linear_fwd_sparse(rows, x, w, b, act=ACT_NONE, out=None):
    """ops.linear_fwd(x, w, b, act) through the row lists `rows` built from x (one fmaf chain per output over the
    row's non-zeros in ascending k); x itself is read only where the shape sends the call to the dense product
    (K > 512)."""
    return _linear_fwd_sparse(rows, x, w, b, act, out, None)


SparsePathCounts = collections.namedtuple("SparsePathCounts", "builds fwd_sparse fwd_dense")


def sparse_path_counts():
    """How the sparse-input entry points of this process went so far (itts_sparse_path_counts; no device call): list
    builds, linear_fwd_sparse calls that ran the sparse kernel, and those that ran the dense product (K > 512)."""
    out = (ctypes.c_int64 * 3)()
    _lib.check(_lib.load().itts_sparse_path_counts(out), "itts_sparse_path_counts")
    return SparsePathCounts(*[int(v) for v in out])


def linear_fwd_mse(x, w, b, target, row_valid, n_valid, loss_weight=1.0, grad=None):
    """Output layer + masked MSE ('mean_per_frame') of a training step in one launch:
    (loss [1], d loss / d output [M, N]); the layer's output itself is not materialised."""
    L = _lib.load()
    _need(x, torch.float32, "x")
    _need(w, torch.float32, "w")
    _need(target, torch.float32, "target")
    _need(row_valid, torch.uint8, "row_valid")
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K or not w.is_contiguous():
        raise ValueError("w must be contiguous [N, K]")
    loss = torch.empty((1,), dtype=torch.float32, device=x.device)
    if grad is None:
        grad = torch.zeros((M, (N + 3) // 4 * 4), dtype=torch.float32, device=x.device)[:, :N]
    ws = _workspace(max(L.itts_linear_fwd_mse_workspace_bytes(M, N), 8), x.device)
    _lib.check(L.itts_linear_fwd_mse(_ptr(x), _rows(x, "x"), _ptr(w), _ptr(b), _ptr(target),
                                     _rows(target, "target"), _ptr(row_valid), float(n_valid),
                                     float(loss_weight), M, N, K, _ptr(loss), _ptr(grad),
                                     _rows(grad, "grad"), _ptr(ws), _stream()),
               "itts_linear_fwd_mse")
    return loss, grad


def _full_rows(t):
    """The [M, pitch] tensor a column-slice view t = buf[:, :N] was cut from (None when t is not one)."""
    if t.dim() != 2 or t.shape[0] == 0 or t.stride(1) != 1 or t.stride(0) <= t.shape[1]:
        return None
    M, P = t.shape[0], t.stride(0)
    if t.storage_offset() + M * P > t.untyped_storage().nbytes() // t.element_size():
        return None
    return torch.as_strided(t, (M, P), (P, 1))


def act_bwd(dy, y, act, out=None):
    """dz = dy * act'(y).  Rows with a padded pitch (views buf[:, :N] of [M, pitch] buffers whose pad columns
    are zero, as LinearActFunction makes them for N % 4 != 0) keep their pitch: the kernel runs over the
    whole buffers (0 * act'(0) = 0 in the pad columns) and the result is the same kind of view, so the GEMMs
    behind it still see 16-byte rows."""
    L = _lib.load()
    if out is None and dy.shape == y.shape:
        fdy, fy = _full_rows(dy), _full_rows(y)
        if fdy is not None and fy is not None and fdy.shape == fy.shape:
            full = torch.empty_like(fdy)
            _lib.check(L.itts_act_bwd(_ptr(fdy), _ptr(fy), _ptr(full), fdy.numel(), act, _stream()),
                       "itts_act_bwd")
            return full[:, :dy.shape[1]]
    dy = dy.contiguous()
    y = y.contiguous()
    if out is None:
        out = torch.empty_like(dy)
    _lib.check(L.itts_act_bwd(_ptr(dy), _ptr(y), _ptr(out), dy.numel(), act, _stream()),
               "itts_act_bwd")
    return out


def rows_gather(src, idx, width=None, fill_row=None, out=None, out_width=None):
    """out[r, :width] = src[idx[r], :width] (the fill row, or zeros, where idx[r] is outside
    [0, len(src))); columns width .. out_width - 1 are zeroed.  src: float32 [R, >= width] with unit
    column stride (any row pitch: column slices of a wider tensor are fine), idx: int64 [n_out]."""
    L = _lib.load()
    assert src.dtype == torch.float32 and src.dim() == 2 and (src.shape[1] <= 1 or src.stride(1) == 1)
    assert idx.dtype == torch.int64 and idx.is_contiguous()
    width = src.shape[1] if width is None else int(width)
    out_width = width if out_width is None else int(out_width)
    n_out = idx.numel()
    if out is None:
        out = torch.empty((n_out, out_width), dtype=torch.float32, device=src.device)
    assert out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == n_out and \
        (out.shape[1] <= 1 or out.stride(1) == 1) and out.shape[1] >= out_width
    ld_src = src.stride(0) if src.shape[0] > 1 else max(src.shape[1], 1)
    ld_dst = out.stride(0) if n_out > 1 else max(out.shape[1], 1)
    fill = fill_row.contiguous() if fill_row is not None else None
    _lib.check(L.itts_rows_gather_f32(_ptr(src), ld_src, src.shape[0], _ptr(idx), n_out, width,
                                      _ptr(fill) if fill is not None else None, _ptr(out), ld_dst, out_width,
                                      _stream()), "itts_rows_gather_f32")
    return out


def _batch_rows_2d(t, name):
    """[B, T, D] / [T, B, D] padded batch (contiguous positions) -> row pitch"""
    if t.dim() != 3 or (t.shape[2] > 1 and t.stride(2) != 1):
        raise ValueError("{} must be a 3-D padded batch with contiguous rows".format(name))
    ld = max(t.stride(1), t.shape[2], 1)
    if t.shape[0] > 1 and t.shape[1] > 0 and t.stride(0) != ld * t.shape[1]:
        raise ValueError("{}: the positions of the padded batch must be evenly spaced".format(name))
    return ld


def batch_pad_gather(rows, starts, lens, n_utts, t_max, batch_first, fill_row=None, want_mask=False, width=None,
                     rep_pos=-1, rep_row=None):
    """The padded batch of utterances whose rows lie back to back in `rows` (float32 [R, >= width]; utterance b:
    rows starts[b] .. starts[b] + lens[b] - 1; starts / lens int64 [n_utts] on the device): position (b, t) takes
    row starts[b] + t for t < lens[b], else the fill row (zeros when None) -- the padding position with flat index
    `rep_pos` takes `rep_row` instead.  Returns (padded [B, T, width] or
    [T, B, width], mask [B, T, 1] / [T, B, 1] or None) -- prepare_batch's pad_sequence + sequence_mask
    (ModularModelHandlerPyTorch.py:388-491) in one launch."""
    L = _lib.load()
    _need(rows, torch.float32, "rows")
    assert rows.dim() == 2 and (rows.shape[1] <= 1 or rows.stride(1) == 1)
    assert starts.dtype == torch.int64 and lens.dtype == torch.int64 and starts.is_cuda and lens.is_cuda
    assert starts.numel() >= n_utts and lens.numel() >= n_utts and starts.is_contiguous() and lens.is_contiguous()
    width = rows.shape[1] if width is None else int(width)
    shape = (n_utts, int(t_max), width) if batch_first else (int(t_max), n_utts, width)
    out = torch.empty(shape, dtype=torch.float32, device=rows.device)
    mask = torch.empty(shape[:2] + (1,), dtype=torch.float32, device=rows.device) if want_mask else None
    fill = fill_row.contiguous() if fill_row is not None else None
    rep = rep_row.contiguous() if rep_row is not None and rep_pos >= 0 else None
    ld_src = rows.stride(0) if rows.shape[0] > 1 else max(rows.shape[1], 1)
    _lib.check(L.itts_batch_pad_gather_f32(_ptr(rows), ld_src, rows.shape[0], _ptr(starts), _ptr(lens), n_utts,
                                           int(t_max), width, 1 if batch_first else 0,
                                           _ptr(fill) if fill is not None else None,
                                           int(rep_pos) if rep is not None else -1, _ptr(rep), _ptr(out), max(width, 1),
                                           _ptr(mask) if mask is not None else None, _stream()),
               "itts_batch_pad_gather_f32")
    return out, mask


def batch_pack_rows(padded, starts, lens, batch_first, n_rows, out_width=None, out=None, rep_pos=-1, rep_dst_row=-1):
    """rows[starts[b] + t, :] = padded position (b, t) for t < lens[b] (the adjoint of batch_pad_gather); columns
    width .. out_width - 1 of the written rows are zeroed.  `n_rows` rows are allocated (rows no valid position maps
    to are left unwritten: the caller owns them).  rep_pos >= 0: that padding position is copied to row rep_dst_row."""
    L = _lib.load()
    _need(padded, torch.float32, "padded")
    ld = _batch_rows_2d(padded, "padded")
    n_utts, t_max = (padded.shape[0], padded.shape[1]) if batch_first else (padded.shape[1], padded.shape[0])
    width = padded.shape[2]
    out_width = width if out_width is None else int(out_width)
    if out is None:
        out = torch.empty((int(n_rows), out_width), dtype=torch.float32, device=padded.device)
    assert out.dim() == 2 and out.shape[0] >= n_rows and out.shape[1] >= out_width and \
        (out.shape[1] <= 1 or out.stride(1) == 1)
    ld_dst = out.stride(0) if out.shape[0] > 1 else max(out.shape[1], 1)
    _lib.check(L.itts_batch_pack_rows_f32(_ptr(padded), ld, _ptr(starts), _ptr(lens), n_utts, t_max, width,
                                          1 if batch_first else 0, _ptr(out), ld_dst, out_width, int(rep_pos),
                                          int(rep_dst_row), _stream()),
               "itts_batch_pack_rows_f32")
    return out


def batch_concat_rows(rows, table, n_out, t_max, width=None, out_width=None):
    """out[dst_starts[b] + t] = rows[src_starts[b] + t] for t < lens[b]; table: int64 [3, B] on the device (src starts,
    dst starts, lens); n_out rows of out_width floats (columns beyond `width` zero).  FrameShard.gather's batches."""
    L = _lib.load()
    _need(rows, torch.float32, "rows")
    assert rows.dim() == 2 and (rows.shape[1] <= 1 or rows.stride(1) == 1)
    assert table.dtype == torch.int64 and table.is_cuda and table.dim() == 2 and table.shape[0] == 3 and \
        table.is_contiguous()
    width = rows.shape[1] if width is None else int(width)
    out_width = width if out_width is None else int(out_width)
    out = torch.empty((int(n_out), out_width), dtype=torch.float32, device=rows.device)
    ld_src = rows.stride(0) if rows.shape[0] > 1 else max(rows.shape[1], 1)
    _lib.check(L.itts_batch_concat_rows_f32(_ptr(rows), ld_src, rows.shape[0], _ptr(table[0]), _ptr(table[1]),
                                            _ptr(table[2]), table.shape[1], int(t_max), width, _ptr(out),
                                            max(out_width, 1), out_width, _stream()), "itts_batch_concat_rows_f32")
    return out


def batch_pad_colsum(padded, lens, batch_first, out=None):
    """Per column, the sum of a padded batch over its padding positions (t >= lens[b]), in a fixed order; into `out`
    (contiguous, at least as wide: the further columns are zeroed) when given."""
    L = _lib.load()
    _need(padded, torch.float32, "padded")
    ld = _batch_rows_2d(padded, "padded")
    n_utts, t_max = (padded.shape[0], padded.shape[1]) if batch_first else (padded.shape[1], padded.shape[0])
    width = padded.shape[2]
    if out is None:
        out = torch.empty(width, dtype=torch.float32, device=padded.device)
    assert out.dim() == 1 and out.is_contiguous() and out.numel() >= width
    ws = torch.empty(max(int(L.itts_batch_pad_colsum_workspace_bytes(n_utts * t_max, width)), 4), dtype=torch.uint8,
                     device=padded.device)
    _lib.check(L.itts_batch_pad_colsum_f32(_ptr(padded), ld, _ptr(lens), n_utts, t_max, width,
                                           1 if batch_first else 0, _ptr(out), out.numel(), _ptr(ws), _stream()),
               "itts_batch_pad_colsum_f32")
    return out


def _linear_bwd_input(dz, w, yprev, act_prev, out, drop):
    L = _lib.load()
    _need(dz, torch.float32, "dz")
    M, N = dz.shape
    K = w.shape[1]
    if out is None:
        out = torch.empty((M, K), dtype=torch.float32, device=dz.device)
    args = (_ptr(dz), _rows(dz, "dz"), _ptr(w), _ptr(out), _rows(out, "out"), _ptr(yprev),
            _rows(yprev, "yprev") if yprev is not None else 0, int(act_prev if act_prev is not None else ACT_NONE),
            M, N, K, _stream())
    if drop is None:
        _lib.check(L.itts_linear_bwd_input(*args), "itts_linear_bwd_input")
    else:
        _lib.check(L.itts_linear_bwd_input_dropout(*args[:-1], *drop, args[-1]), "itts_linear_bwd_input_dropout")
    return out


def linear_bwd_input(dz, w, yprev=None, act_prev=ACT_NONE, out=None):
    return _linear_bwd_input(dz, w, yprev, act_prev, out, None)


_ws_cache = {}
class _DeferState(threading.local):
    """Per host thread, like the library's own deferral switch (thread_local on the C side): calls made
    from another thread -- the autograd worker -- are neither deferred nor counted here."""
    on = False
    next = 0


_defer = _DeferState()


def _workspace(nbytes, device):
    """Scratch of the current (device, stream): two streams never share a workspace.  Inside
    `deferred_reductions()` every call gets a workspace of its own (the partial results it leaves
    there are read by the one reduction launch at the end)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    if _defer.on:
        key = key + (_defer.next,)
        _defer.next += 1
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


class deferred_reductions:
    """with ops.deferred_reductions(): the loss and gradient entry points called inside leave their
    partial sums / split-K slabs in place, and ONE launch reduces them all when the block ends
    (itts_defer_reductions / itts_reduce_deferred; results bit-identical to the separate launches).
    Nothing inside the block may read a loss or a weight / bias gradient produced inside it.
    Blocks do not nest (the inner block's workspaces would be the outer block's still-pending slabs)."""

    def __enter__(self):
        if _defer.on:
            raise RuntimeError("deferred_reductions() blocks do not nest")
        _lib.check(_lib.load().itts_defer_reductions(1), "itts_defer_reductions")
        _defer.on, _defer.next = True, 0
        return self

    def __exit__(self, exc_type, exc, tb):
        _defer.on = False
        _lib.check(_lib.load().itts_reduce_deferred(_stream()), "itts_reduce_deferred")
        return False


def linear_bwd_weight(dz, x, dw=None, db=None, accumulate=False, want_bias=True):
    L = _lib.load()
    _need(dz, torch.float32, "dz")
    _need(x, torch.float32, "x")
    M, N = dz.shape
    K = x.shape[1]
    if dw is None:
        dw = torch.empty((N, K), dtype=torch.float32, device=dz.device)
    if db is None and want_bias:
        db = torch.empty((N,), dtype=torch.float32, device=dz.device)
    ws = _workspace(L.itts_linear_bwd_weight_workspace_bytes(M, N, K), dz.device)
    _lib.check(L.itts_linear_bwd_weight(_ptr(dz), _rows(dz, "dz"), _ptr(x), _rows(x, "x"),
                                        _ptr(dw), _ptr(db), M, N, K, _ptr(ws),
                                        1 if accumulate else 0, _stream()),
               "itts_linear_bwd_weight")
    return dw, db


SPARSE_COLS_MAX_K = 512
SPARSE_COLS_HEAVY = 31          # strip columns for x; the 32nd is the ones of the bias
SPARSE_COLS_OWNERS = 64
SPARSE_COLS_SLOTS = 8
# share of non-zeros above which a column goes to the strip
SPARSE_COLS_HEAVY_DENSITY = 0.25


class SparseColsPlan(object):
    """Which columns of a sparse [M, K] input (K <= 512) the sparse weight gradient treats as heavy (a dense strip
    and MFMAs) and which quarter wave owns each light one (lists).  Made from the non-zero counts per column of one
    batch; it only moves time: every column is served whatever a later batch looks like.
      heavy: the columns with more than heavy_density * rows non-zeros, at most 31, the fullest first
      light: all others, fullest first, each to the owner (of 64, at most 8 columns each) with the least so far"""

    def __init__(self, col_counts, rows, device, heavy_density=SPARSE_COLS_HEAVY_DENSITY):
        counts = [int(c) for c in col_counts]
        K = len(counts)
        if not 0 < K <= SPARSE_COLS_MAX_K:
            raise ValueError("a column plan holds 1 .. {} columns, got {}".format(SPARSE_COLS_MAX_K, K))
        order = sorted(range(K), key=lambda k: (-counts[k], k))
        self.heavy = [k for k in order if counts[k] > heavy_density * rows][:SPARSE_COLS_HEAVY]
        taken = set(self.heavy)
        self.owners = [[] for _ in range(SPARSE_COLS_OWNERS)]
        load = [0] * SPARSE_COLS_OWNERS
        for k in order:
            if k in taken:
                continue
            o = min((o for o in range(SPARSE_COLS_OWNERS) if len(self.owners[o]) < SPARSE_COLS_SLOTS),
                    key=lambda o: (load[o], len(self.owners[o]), o))
            self.owners[o].append(k)
            load[o] += counts[k]
        self.K = K
        self.density = sum(counts) / float(max(rows * K, 1))   # of the batch the plan was made from
        table = [-1] * int(_lib.load().itts_sparse_cols_plan_ints())
        inverse = SPARSE_COLS_HEAVY + 1 + SPARSE_COLS_OWNERS * SPARSE_COLS_SLOTS
        for h, k in enumerate(self.heavy):
            table[h] = k
            table[inverse + k] = 0x1000 + h
        for o, cols in enumerate(self.owners):
            for s, k in enumerate(cols):
                table[SPARSE_COLS_HEAVY + 1 + o * SPARSE_COLS_SLOTS + s] = k
                table[inverse + k] = o * SPARSE_COLS_SLOTS + s
        self.table = torch.tensor(table, dtype=torch.int32, device=device)


def sparse_cols_plan(x, K=None, heavy_density=SPARSE_COLS_HEAVY_DENSITY):
    """SparseColsPlan from the columns of x [M, >= K] itself (reads the device: one synchronisation)"""
    K = x.shape[1] if K is None else int(K)
    counts = (x[:, :K] != 0).sum(dim=0).tolist()
    return SparseColsPlan(counts, x.shape[0], x.device, heavy_density)


class SparseCols(object):
    """Column data of a sparse [M, K] matrix for the sparse weight gradient (itts_sparse_cols_build): per tile of 256
    rows the light columns' (row, value) lists and the strip of the heavy columns, in one device block that the
    caller owns.  A block is reused for any shape it is large enough for."""

    def __init__(self, M, K, device, block=None):
        out = (ctypes.c_int64 * 3)()
        _lib.check(_lib.load().itts_sparse_cols_layout(M, K, out), "itts_sparse_cols_layout")
        self.M, self.K = int(M), int(K)
        self._strip_off, self._streams_off, self.nbytes = (int(v) for v in out)
        if block is None or block.numel() < self.nbytes:
            block = torch.empty(max(self.nbytes, 16), dtype=torch.uint8, device=device)
        self.block = block

    def strip(self):
        """float32 [tiles * 256, 32]: the heavy columns' values, column 31 ones, rows behind M zeros"""
        return self.block[self._strip_off:self._streams_off].view(torch.float32).view(-1, 32)


def sparse_cols_build(x, plan, K=None, cols=None, lists=None):
    """Column data of the first K (default: all) columns of x [M, >= K] fp32 under `plan`; `cols`: a SparseCols whose
    block is reused when it is large enough.  `lists`: the SparseRows of the same x (over at least K columns): the
    block is then built from them (itts_sparse_cols_build_from_rows) and x is not read."""
    _need(x, torch.float32, "x")
    ldx = _rows(x, "x")
    M = x.shape[0]
    K = x.shape[1] if K is None else int(K)
    if K > x.shape[1]:
        raise ValueError("K exceeds the width of x")
    if plan.K != K:
        raise ValueError("the plan was made for {} columns, not {}".format(plan.K, K))
    out = SparseCols(M, K, x.device, cols.block if cols is not None else None)
    if lists is not None:
        if lists.M != M or lists.K < K:
            raise ValueError("the row lists were built for another shape")
        _lib.check(_lib.load().itts_sparse_cols_build_from_rows(_ptr(lists.block), M, lists.K, K, _ptr(plan.table),
                                                                _ptr(out.block), _stream()),
                   "itts_sparse_cols_build_from_rows")
        return out
    _lib.check(_lib.load().itts_sparse_cols_build(_ptr(x), ldx, M, K, _ptr(plan.table), _ptr(out.block), _stream()),
               "itts_sparse_cols_build")
    return out


def linear_bwd_weight_sparse(dz, x, cols, plan, dw=None, db=None, accumulate=False, want_bias=True, K=None):
    """ops.linear_bwd_weight(dz, x[:, :K]) through the column data `cols` built from x under `plan`.  dw may be
    [N, lddw] with lddw >= K: its pad columns become zeros.  Without cols / plan (None), or with a shape the kernel
    does not serve, the dense product runs on x (ops.sparse_wgrad_counts says which)."""
    L = _lib.load()
    _need(dz, torch.float32, "dz")
    _need(x, torch.float32, "x")
    M, N = dz.shape
    K = (cols.K if cols is not None else x.shape[1]) if K is None else int(K)
    if cols is not None and (cols.M != M or cols.K != K or plan is None or plan.K != K):
        raise ValueError("the column data were built for another shape or without this plan")
    if dw is None:
        dw = torch.empty((N, K), dtype=torch.float32, device=dz.device)
    if dw.dim() != 2 or dw.shape[0] != N or dw.shape[1] < K or not dw.is_contiguous():
        raise ValueError("dw must be contiguous [N, >= K]")
    if db is None and want_bias:
        db = torch.empty((N,), dtype=torch.float32, device=dz.device)
    lddw = dw.shape[1]
    ws = _workspace(L.itts_linear_bwd_weight_sparse_workspace_bytes(M, N, K, lddw), dz.device)
    _lib.check(L.itts_linear_bwd_weight_sparse(_ptr(dz), _rows(dz, "dz"),
                                               _ptr(cols.block) if cols is not None else None,
                                               _ptr(plan.table) if plan is not None else None, _ptr(x), _rows(x, "x"),
                                               _ptr(dw), lddw, _ptr(db), M, N, K, _ptr(ws), 1 if accumulate else 0,
                                               _stream()), "itts_linear_bwd_weight_sparse")
    return dw, db


SparseWgradCounts = collections.namedtuple("SparseWgradCounts", "col_builds dw_sparse dw_dense")


def sparse_wgrad_counts():
    """How the sparse weight-gradient entry points of this process went so far (itts_sparse_wgrad_counts; no device
    call): column builds, linear_bwd_weight_sparse calls that ran the sparse kernel, and those sent to the dense
    product."""
    out = (ctypes.c_int64 * 3)()
    _lib.check(_lib.load().itts_sparse_wgrad_counts(out), "itts_sparse_wgrad_counts")
    return SparseWgradCounts(*[int(v) for v in out])


# ------------------------------------------------------------------------------ Conv1d groups
# Activations stay in the model's layout: [B, T, C] (batch_first) or [T, B, C], channels last, so that
# row (b, t) of the padded batch is one row of a 2-D [B*T, ld] view; no transpose to torch's [B, C, T].
def conv1d_out_len(T_in, kernel_size, padding, dilation):
    """T_out of a stride-1 Conv1d (rnn_dyn/CNNWrapper.py:get_output_length)"""
    return T_in + 2 * padding - dilation * (kernel_size - 1)


def _conv_rows(t, name):
    """(t, ld): t as a [B, T, C] / [T, B, C] tensor whose row (i, j) sits at (i * shape[1] + j) * ld, copied
    when its strides do not allow that; a 16-byte pitch wider than C is kept only when the storage holds the
    last row's pad floats (the kernels read them, see the pitch rule in include/idiaptts_amd.h)."""
    if t.dim() != 3:
        raise ValueError("{} must be 3-D [B, T, C] (batch_first) or [T, B, C]".format(name))
    C = t.shape[2]
    ld = t.stride(1) if t.shape[1] > 1 else (t.stride(0) if t.shape[0] > 1 else C)
    ok = (t.stride(2) == 1 or C == 1) and ld >= C and (t.shape[0] == 1 or t.stride(0) == t.shape[1] * ld)
    if ok and ld != C and ld % 4 == 0:
        ok = t.storage_offset() + t.shape[0] * t.shape[1] * ld <= t.untyped_storage().nbytes() // 4
    if ok:
        return t, ld
    return t.clone(memory_format=torch.contiguous_format), C


def _conv_dims(x, batch_first):
    return (x.shape[0], x.shape[1]) if batch_first else (x.shape[1], x.shape[0])


def _conv_geometry(w, padding, dilation, T_in):
    if w.dim() != 3 or not w.is_contiguous():
        raise ValueError("w must be contiguous [Cout, Cin, Kw]")
    Cout, Cin, Kw = w.shape
    padding, dilation = int(padding), int(dilation)
    if padding < 0 or dilation < 1:
        raise ValueError("padding must be >= 0 and dilation >= 1, got {} / {}".format(padding, dilation))
    T_out = conv1d_out_len(T_in, Kw, padding, dilation)
    if T_out <= 0:
        raise ValueError("Conv1d output length T_in + 2 padding - dilation (kernel_size - 1) = {} + 2 * {} - {} * {} "
                         "= {} is not positive".format(T_in, padding, dilation, Kw - 1, T_out))
    return Cout, Cin, Kw, padding, dilation, T_out


def _conv_out(like, batch_first, B, T, C):
    shape = (B, T, C) if batch_first else (T, B, C)
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _conv_out_rows(out, shape, name="out"):
    """The row pitch of a caller's output: a contiguous `shape` tensor or a column slice of a wider one (only its own
    columns are written)."""
    C = shape[2]
    if tuple(out.shape) == tuple(shape) and out.dtype == torch.float32:
        ld = out.stride(1) if shape[1] > 1 else (out.stride(0) if shape[0] > 1 else C)
        if (out.stride(2) == 1 or C == 1) and ld >= C and (shape[0] == 1 or out.stride(0) == shape[1] * ld):
            return ld
    raise ValueError("{} must be a float32 {} tensor with contiguous rows of one pitch".format(name, tuple(shape)))


CONV_FWD, CONV_BWD_INPUT, CONV_BWD_WEIGHT = 0, 1, 2


def conv1d_plan(product, B, T_in, Cin, Cout, kernel_size, padding, dilation, vec=True):
    """(tile_cols, slabs, kchunk) of conv1d_fwd (product CONV_FWD), conv1d_bwd_input (CONV_BWD_INPUT) or
    conv1d_bwd_weight (CONV_BWD_WEIGHT) for such a call: the workgroup tile's 64 or 128 output columns, the number of
    slabs the reduction is split into and the reduction elements per slab (itts_conv1d_plan, the function the kernels'
    launches read; no device work).  vec: whether the operands allow 16-byte loads (it selects the kernel
    instantiation; no tile or split depends on it today).  ValueError for a geometry the products reject."""
    tile, slabs, kchunk = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    rc = _lib.load().itts_conv1d_plan(int(product), int(B), int(T_in), int(Cin), int(Cout), int(kernel_size),
                                      int(padding), int(dilation), 1 if vec else 0, ctypes.byref(tile),
                                      ctypes.byref(slabs), ctypes.byref(kchunk))
    if rc != 0:
        raise ValueError("no Conv1d plan for product {} B {} T_in {} Cin {} Cout {} kernel {} padding {} dilation {}"
                         .format(product, B, T_in, Cin, Cout, kernel_size, padding, dilation))
    return tile.value, slabs.value, kchunk.value


def conv1d_fwd(x, w, b, padding, dilation, batch_first, act=ACT_NONE, out=None):
    """y = act(conv1d(x, w, b, padding, dilation)) over the time axis: x [B, T_in, Cin] (batch_first) or
    [T_in, B, Cin], w [Cout, Cin, Kw] (torch's layout), b [Cout] or None -> y [B, T_out, Cout] / [T_out, B, Cout]."""
    L = _lib.load()
    _need(x, torch.float32, "x")
    _need(w, torch.float32, "w")
    B, T_in = _conv_dims(x, batch_first)
    Cout, Cin, Kw, padding, dilation, T_out = _conv_geometry(w, padding, dilation, T_in)
    if x.shape[2] != Cin:
        raise ValueError("x has {} channels, w expects {}".format(x.shape[2], Cin))
    if b is not None:
        _need(b, torch.float32, "b")
        if b.shape != (Cout,) or not b.is_contiguous():
            raise ValueError("b must be contiguous [Cout]")
    x, ldx = _conv_rows(x, "x")
    shape = (B, T_out, Cout) if batch_first else (T_out, B, Cout)
    if out is None:
        out = _conv_out(x, batch_first, B, T_out, Cout)
    ldy = _conv_out_rows(out, shape)
    _lib.check(L.itts_conv1d_fwd(_ptr(x), ldx, _ptr(w), _ptr(b), _ptr(out), ldy, B, T_in, Cin, Cout, Kw, padding,
                                 dilation, 1 if batch_first else 0, act, _stream()), "itts_conv1d_fwd")
    return out


def conv1d_bwd_input(dz, w, T_in, padding, dilation, batch_first, yprev=None, act_prev=ACT_NONE, out=None):
    """dx [B, T_in, Cin] (layout of dz) from dz [B, T_out, Cout]; with yprev (the previous layer's output, shaped
    as dx) dx *= act_prev'(yprev)."""
    L = _lib.load()
    _need(dz, torch.float32, "dz")
    _need(w, torch.float32, "w")
    B, T_dz = _conv_dims(dz, batch_first)
    Cout, Cin, Kw, padding, dilation, T_out = _conv_geometry(w, padding, dilation, int(T_in))
    if T_dz != T_out or dz.shape[2] != Cout:
        raise ValueError("dz must have {} steps and {} channels, got {}".format(T_out, Cout, tuple(dz.shape)))
    shape = (B, T_in, Cin) if batch_first else (T_in, B, Cin)
    dz, lddz = _conv_rows(dz, "dz")
    ldyp = 0
    if yprev is not None:
        _need(yprev, torch.float32, "yprev")
        if tuple(yprev.shape) != shape:
            raise ValueError("yprev must be {}".format(shape))
        yprev, ldyp = _conv_rows(yprev, "yprev")
    if out is None:
        out = _conv_out(dz, batch_first, B, T_in, Cin)
    lddx = _conv_out_rows(out, shape)
    _lib.check(L.itts_conv1d_bwd_input(_ptr(dz), lddz, _ptr(w), _ptr(out), lddx, _ptr(yprev), ldyp, act_prev, B,
                                       int(T_in), Cin, Cout, Kw, padding, dilation, 1 if batch_first else 0,
                                       _stream()), "itts_conv1d_bwd_input")
    return out


def conv1d_bwd_weight(dz, x, kernel_size, padding, dilation, batch_first, dw=None, db=None, accumulate=False,
                      want_bias=True):
    """(dw [Cout, Cin, Kw], db [Cout] or None) of conv1d_fwd from dz [B, T_out, Cout] and its input x; deterministic
    (a fixed split of the B * T_out rows through a workspace); accumulate adds to dw / db."""
    L = _lib.load()
    _need(dz, torch.float32, "dz")
    _need(x, torch.float32, "x")
    B, T_in = _conv_dims(x, batch_first)
    Cin, Cout, Kw = x.shape[2], dz.shape[2], int(kernel_size)
    T_out = conv1d_out_len(T_in, Kw, int(padding), int(dilation))
    if Kw < 1 or int(padding) < 0 or int(dilation) < 1 or T_out <= 0:
        raise ValueError("Conv1d output length {} (T_in {}, kernel {}, padding {}, dilation {}) is not positive"
                         .format(T_out, T_in, Kw, padding, dilation))
    if _conv_dims(dz, batch_first) != (B, T_out):
        raise ValueError("dz must have batch {} and {} steps, got {}".format(B, T_out, tuple(dz.shape)))
    x, ldx = _conv_rows(x, "x")
    dz, lddz = _conv_rows(dz, "dz")
    if dw is None:
        dw = (torch.zeros if accumulate else torch.empty)((Cout, Cin, Kw), dtype=torch.float32, device=dz.device)
    if db is None and want_bias:
        db = (torch.zeros if accumulate else torch.empty)((Cout,), dtype=torch.float32, device=dz.device)
    if tuple(dw.shape) != (Cout, Cin, Kw) or not dw.is_contiguous():
        raise ValueError("dw must be contiguous [{}, {}, {}]".format(Cout, Cin, Kw))
    if db is not None and (tuple(db.shape) != (Cout,) or not db.is_contiguous()):
        raise ValueError("db must be contiguous [{}]".format(Cout))
    ws = _workspace(L.itts_conv1d_bwd_weight_workspace_bytes(B, T_in, Cin, Cout, Kw, int(padding), int(dilation)),
                    dz.device)
    _lib.check(L.itts_conv1d_bwd_weight(_ptr(dz), lddz, _ptr(x), ldx, _ptr(dw), _ptr(db), B, T_in, Cin, Cout, Kw,
                                        int(padding), int(dilation), 1 if batch_first else 0, _ptr(ws),
                                        1 if accumulate else 0, _stream()), "itts_conv1d_bwd_weight")
    return dw, db


def _linear_bwd(dz, x, w, dw, db, dx, yprev, act_prev, accumulate, drop):
    L = _lib.load()
    _need(dz, torch.float32, "dz")
    _need(x, torch.float32, "x")
    _need(w, torch.float32, "w")
    M, N = dz.shape
    K = x.shape[1]
    if w.shape != (N, K) or not w.is_contiguous() or not dw.is_contiguous() or dw.shape != (N, K):
        raise ValueError("w and dw must be contiguous [N, K]")
    ws = _workspace(L.itts_linear_bwd_weight_workspace_bytes(M, N, K), dz.device)
    args = (_ptr(dz), _rows(dz, "dz"), _ptr(x), _rows(x, "x"), _ptr(w), _ptr(dw), _ptr(db), _ptr(dx), _rows(dx, "dx"),
            _ptr(yprev), _rows(yprev, "yprev") if yprev is not None else 0,
            int(act_prev if act_prev is not None else ACT_NONE), M, N, K, _ptr(ws), 1 if accumulate else 0,
            _stream())
    if drop is None:
        _lib.check(L.itts_linear_bwd(*args), "itts_linear_bwd")
    else:
        _lib.check(L.itts_linear_bwd_dropout(*args[:-1], *drop, args[-1]), "itts_linear_bwd_dropout")
    return dw, db, dx


def linear_bwd(dz, x, w, dw, db, dx, yprev=None, act_prev=ACT_NONE, accumulate=False):
    """dw [N, K] (+ db [N]) and dx [M, K] of a linear layer from dz [M, N], its input x [M, K] and its
    weight w [N, K] in one call (one launch when the buffers allow 16-byte rows); dx is multiplied by
    the derivative of the previous layer's activation when yprev (that layer's output) is given."""
    return _linear_bwd(dz, x, w, dw, db, dx, yprev, act_prev, accumulate, None)


# ------------------------------------------------------------------------------ dropout (csrc/dropout.h)
# The mask of element (row, col) is a function of (seed, salt, row + row_offset, col): the backward recomputes it,
# none is stored.  p in [0, 1); seed a 64-bit integer, salt a 32-bit one (the layer).
def _drop_args(p, seed, salt, row_offset):
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout p must be in [0, 1), got {}".format(p))
    return (p, ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ctypes.c_uint32(int(salt) & 0xFFFFFFFF),
            ctypes.c_int64(int(row_offset)))


def _like_rows(t):
    """[M, N] view of fresh rows whose pitch is N rounded up to four floats, pad columns zero (the GEMMs behind it
    keep their 16-byte rows)"""
    M, N = t.shape
    Np = (N + 3) // 4 * 4
    full = torch.empty((M, Np), dtype=torch.float32, device=t.device)
    if Np != N:
        full[:, N:] = 0
    return full[:, :N]


def dropout_apply(x, p, seed, salt, row_offset=0, out=None):
    """out = x * m * (1 / (1 - p)) on [M, N] rows (any pitch), the forward and the backward of a dropout alike;
    out may be x (in place)."""
    L = _lib.load()
    _need(x, torch.float32, "x")
    if out is None:
        out = _like_rows(x)
    _need(out, torch.float32, "out")
    if out.shape != x.shape:
        raise ValueError("out must have the shape of x")
    M, N = x.shape
    if N == 0:
        return out
    _lib.check(L.itts_dropout_apply(_ptr(x), _rows(x, "x"), _ptr(out), _rows(out, "out"), M, N, 0,
                                    *_drop_args(p, seed, salt, row_offset), _stream()), "itts_dropout_apply")
    return out


def dropout_mask(M, N, p, seed, salt, row_offset=0, device="cuda"):
    """bool [M, N]: True where the rule keeps the element"""
    L = _lib.load()
    out = torch.empty((int(M), int(N)), dtype=torch.uint8, device=device)
    if M and N:
        _lib.check(L.itts_dropout_apply(None, 0, _ptr(out), int(N), int(M), int(N), 1,
                                        *_drop_args(p, seed, salt, row_offset), _stream()), "itts_dropout_apply")
    return out.bool()


def dropout_act_bwd(dy, d, act, p, seed, salt, row_offset=0, out=None):
    """dz = dy * m * scale * act'(y) from the dropped output d = y * m * scale of a layer (act_bwd for a layer with
    dropout); out may be dy"""
    L = _lib.load()
    _need(dy, torch.float32, "dy")
    _need(d, torch.float32, "d")
    if dy.shape != d.shape:
        raise ValueError("dy and d must have one shape")
    if out is None:
        out = _like_rows(dy)
    M, N = dy.shape
    if N == 0:
        return out
    _lib.check(L.itts_dropout_act_bwd(_ptr(dy), _rows(dy, "dy"), _ptr(d), _rows(d, "d"), _ptr(out), _rows(out, "out"),
                                      M, N, int(act if act is not None else ACT_NONE),
                                      *_drop_args(p, seed, salt, row_offset), _stream()), "itts_dropout_act_bwd")
    return out


def linear_fwd_dropout(x, w, b, act=ACT_NONE, p=0.0, seed=0, salt=0, row_offset=0, out=None):
    """linear_fwd with dropout on the output, applied in the product's epilogue"""
    return _linear_fwd(x, w, b, act, out, _drop_args(p, seed, salt, row_offset))


def linear_fwd_sparse_dropout(rows, x, w, b, act=ACT_NONE, p=0.0, seed=0, salt=0, row_offset=0, out=None):
    """linear_fwd_sparse with dropout on the output"""
    return _linear_fwd_sparse(rows, x, w, b, act, out, _drop_args(p, seed, salt, row_offset))


def linear_bwd_input_dropout(dz, w, yprev, act_prev=ACT_NONE, p=0.0, seed=0, salt=0, row_offset=0, out=None):
    """linear_bwd_input where yprev, the previous layer's output, carries the dropout (p, seed, salt, row_offset)"""
    return _linear_bwd_input(dz, w, yprev, act_prev, out, _drop_args(p, seed, salt, row_offset))


def linear_bwd_dropout(dz, x, w, dw, db, dx, yprev, act_prev=ACT_NONE, p=0.0, seed=0, salt=0, row_offset=0,
                       accumulate=False):
    """linear_bwd where yprev, the previous layer's output, carries the dropout (p, seed, salt, row_offset)"""
    return _linear_bwd(dz, x, w, dw, db, dx, yprev, act_prev, accumulate, _drop_args(p, seed, salt, row_offset))


def masked_mse(pred, target, row_valid, n_valid, loss_weight=1.0, want_grad=True, grad=None):
    """NamedLoss(MSELoss, 'mean_per_frame') (loss/NamedLoss.py:70-117) on [M, D] rows."""
    L = _lib.load()
    _need(pred, torch.float32, "pred")
    _need(target, torch.float32, "target")
    _need(row_valid, torch.uint8, "row_valid")
    M, D = pred.shape
    loss = torch.empty((1,), dtype=torch.float32, device=pred.device)
    if want_grad and grad is None:
        grad = torch.empty((M, D), dtype=torch.float32, device=pred.device)
    ws = _workspace(max(L.itts_masked_mse_workspace_bytes(M, D), 8), pred.device)
    _lib.check(L.itts_masked_mse(_ptr(pred), _rows(pred, "pred"), _ptr(target),
                                 _rows(target, "target"), _ptr(row_valid), M, D, float(n_valid),
                                 float(loss_weight), _ptr(loss),
                                 _ptr(grad) if want_grad else None,
                                 _rows(grad, "grad") if want_grad else 0, _ptr(ws), _stream()),
               "itts_masked_mse")
    return loss, (grad if want_grad else None)


LAYER_NORM_MAX_WIDTH = 4096      # LN_MAX_D of csrc/layernorm.hip


def layer_norm_fwd(x, gamma, beta, eps=1e-5, act=ACT_NONE, out=None):
    """torch.nn.LayerNorm over the last extent of [N, D] rows (+ the activation `act`): (y, mean [N], rstd [N]);
    gamma / beta [D] or None (rnn_dyn/FFWrapper.py: a LayerNorm group)."""
    L = _lib.load()
    _need(x, torch.float32, "x")
    ldx = _rows(x, "x")
    N, D = x.shape
    for name, t in (("gamma", gamma), ("beta", beta)):
        if t is not None:
            _need(t, torch.float32, name)
            if t.shape != (D,) or not t.is_contiguous():
                raise ValueError("{} must be a contiguous [{}] vector".format(name, D))
    if out is None:
        out = torch.empty((N, D), dtype=torch.float32, device=x.device)
    stats = torch.empty((2, N), dtype=torch.float32, device=x.device)
    _lib.check(L.itts_layernorm_fwd(_ptr(x), ldx, _ptr(gamma), _ptr(beta), _ptr(out), _rows(out, "out"),
                                    _ptr(stats[0]), _ptr(stats[1]), N, D, float(eps), int(act), _stream()),
               "itts_layernorm_fwd")
    return out, stats[0], stats[1]


def layer_norm_bwd(dy, x, mean, rstd, gamma, y=None, act=ACT_NONE, want_gamma=True, want_beta=True, dx=None):
    """(dx, dgamma or None, dbeta or None) of layer_norm_fwd; `y` (the forward's output) is needed under an
    activation only.  The column sums go through per-workgroup slabs reduced in a fixed order."""
    L = _lib.load()
    _need(dy, torch.float32, "dy")
    _need(x, torch.float32, "x")
    N, D = x.shape
    if dy.shape != x.shape:
        raise ValueError("dy must have the shape of x")
    if act != ACT_NONE and y is None:
        raise ValueError("layer_norm_bwd under an activation needs the forward's output y")
    if dx is None:
        dx = torch.empty((N, D), dtype=torch.float32, device=x.device)
    dgamma = torch.empty((D,), dtype=torch.float32, device=x.device) if want_gamma else None
    dbeta = torch.empty((D,), dtype=torch.float32, device=x.device) if want_beta else None
    ws = None
    if want_gamma or want_beta:
        ws = _workspace(max(L.itts_layernorm_workspace_bytes(N, D), 8), x.device)
    _lib.check(L.itts_layernorm_bwd(_ptr(dy), _rows(dy, "dy"), _ptr(x), _rows(x, "x"),
                                    _ptr(y) if act != ACT_NONE else None,
                                    _rows(y, "y") if act != ACT_NONE else 0, _ptr(mean), _ptr(rstd), _ptr(gamma),
                                    _ptr(dx), _rows(dx, "dx"), _ptr(dgamma), _ptr(dbeta), N, D, int(act), _ptr(ws),
                                    _stream()), "itts_layernorm_bwd")
    return dx, dgamma, dbeta


# the envelope of csrc/attention.hip (AT_*)
ATTENTION_MIN_HEAD_DIM, ATTENTION_MAX_HEAD_DIM, ATTENTION_HEAD_DIM_STEP = 4, 128, 4
ATTENTION_MAX_WIDTH, ATTENTION_MAX_TIME, ATTENTION_MAX_BATCH_HEADS = 1024, 32768, 65535


def attention_check_envelope(d_model, nhead, T=None, B=None):
    """NotImplementedError naming the value that the attention kernels do not take (d_model = nhead * dh)"""
    dh = d_model // nhead
    if (d_model != nhead * dh or dh % ATTENTION_HEAD_DIM_STEP
            or not ATTENTION_MIN_HEAD_DIM <= dh <= ATTENTION_MAX_HEAD_DIM):
        raise NotImplementedError("attention with head width d_model / nhead = {} / {}: the kernel takes multiples "
                                  "of {} in {} .. {}".format(d_model, nhead, ATTENTION_HEAD_DIM_STEP,
                                                             ATTENTION_MIN_HEAD_DIM, ATTENTION_MAX_HEAD_DIM))
    if d_model > ATTENTION_MAX_WIDTH:
        raise NotImplementedError("attention over d_model = {}: the kernel takes at most {}"
                                  .format(d_model, ATTENTION_MAX_WIDTH))
    if T is not None and not 1 <= T <= ATTENTION_MAX_TIME:
        raise NotImplementedError("attention over T = {} positions: the kernel takes 1 .. {}"
                                  .format(T, ATTENTION_MAX_TIME))
    if B is not None and B * nhead > ATTENTION_MAX_BATCH_HEADS:
        raise NotImplementedError("attention over B * nhead = {} * {}: the kernel takes at most {}"
                                  .format(B, nhead, ATTENTION_MAX_BATCH_HEADS))


def _attention_operands(qkv, nhead, klen, batch_first):
    _need(qkv, torch.float32, "qkv")
    if qkv.dim() != 3 or not qkv.is_contiguous() or qkv.shape[2] % 3:
        raise ValueError("qkv must be a contiguous [B, T, 3 D] / [T, B, 3 D] tensor")
    B, T = (qkv.shape[0], qkv.shape[1]) if batch_first else (qkv.shape[1], qkv.shape[0])
    D = qkv.shape[2] // 3
    attention_check_envelope(D, nhead, T if B else None, B)
    if klen is not None:
        _need(klen, torch.int32, "klen")
        if klen.shape != (B,) or not klen.is_contiguous():
            raise ValueError("klen must be a contiguous [{}] vector".format(B))
    strides = (T, 1) if batch_first else (1, B)
    return B, T, D, strides


def attention_forward(qkv, nhead, klen=None, batch_first=True, p=0.0, seed=0, salt=0):
    """softmax(q k^T / sqrt(dh)) v per utterance and head (torch.nn.MultiheadAttention between its projections):
    qkv [B, T, 3 D] (batch_first) or [T, B, 3 D] as the in-projection writes it, klen [B] int32 keys per utterance
    (None: T); every query t < T attends keys 0 .. klen[b] - 1.  p > 0: dropout on the probabilities, mask from
    (seed, salt, (b * nhead + h) * T + t, key).  Returns (o in qkv's layout with D columns, lse [B, nhead, T])."""
    L = _lib.load()
    B, T, D, (sb, st) = _attention_operands(qkv, nhead, klen, batch_first)
    o = torch.empty(qkv.shape[:2] + (D,), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, nhead, T), dtype=torch.float32, device=qkv.device)
    if B * T:
        pp, seed, salt, _ = _drop_args(p, seed, salt, 0)
        _lib.check(L.itts_attention_fwd(_ptr(qkv), _ptr(o), _ptr(klen), _ptr(lse), B, T, nhead, D // nhead, sb, st,
                                        pp, seed, salt, _stream()), "itts_attention_fwd")
    return o, lse


def attention_backward(do, qkv, o, lse, nhead, klen=None, batch_first=True, p=0.0, seed=0, salt=0):
    """dqkv (qkv's shape: dq | dk | dv) of attention_forward from do, the forward's operands and outputs and the
    same dropout rule; nothing but qkv, o and lse is stored between the two, and repeated calls give the same bits."""
    L = _lib.load()
    B, T, D, (sb, st) = _attention_operands(qkv, nhead, klen, batch_first)
    for name, t in (("do", do), ("o", o)):
        _need(t, torch.float32, name)
        if t.shape != qkv.shape[:2] + (D,) or not t.is_contiguous():
            raise ValueError("{} must be contiguous with the shape of the forward's output".format(name))
    _need(lse, torch.float32, "lse")
    if lse.shape != (B, nhead, T) or not lse.is_contiguous():
        raise ValueError("lse must be the forward's [B, nhead, T] log-sum-exp")
    dqkv = torch.empty_like(qkv)
    if B * T:
        pp, seed, salt, _ = _drop_args(p, seed, salt, 0)
        _lib.check(L.itts_attention_bwd(_ptr(do), _ptr(qkv), _ptr(o), _ptr(klen), _ptr(lse), _ptr(dqkv), B, T, nhead,
                                        D // nhead, sb, st, pp, seed, salt, _stream()), "itts_attention_bwd")
    return dqkv


ALLPASS_MAX_SIZE = 64            # kAllpassMaxN of csrc/allpass.h


def _allpass_operands(x, alpha, mean, std_dev, N):
    _need(x, torch.float32, "x")
    _need(alpha, torch.float32, "alpha")
    M, D = x.shape
    if alpha.shape != (M,) or not alpha.is_contiguous():
        raise ValueError("alpha must be a contiguous [{}] vector, one factor per row".format(M))
    for name, t in (("mean", mean), ("std_dev", std_dev)):
        if t is not None:
            _need(t, torch.float32, name)
            if t.shape != (D,) or not t.is_contiguous():
                raise ValueError("{} must be a contiguous [{}] vector".format(name, D))
    return M, D


def allpass_warp_fwd(x, alpha, N, mean=None, std_dev=None, out=None):
    """All-pass warping of [M, D] rows, D = nb * N, by one factor per row (layers/AllPassWarp.py forward between
    layers/AllPassWarpLayer.py's _denormalise / _normalise): returns y [M, D]; x is not modified."""
    L = _lib.load()
    M, D = _allpass_operands(x, alpha, mean, std_dev, N)
    if out is None:
        out = torch.empty((M, D), dtype=torch.float32, device=x.device)
    _need(out, torch.float32, "out")
    _lib.check(L.itts_allpass_warp_fwd(_ptr(x), _rows(x, "x"), _ptr(alpha), _ptr(mean), _ptr(std_dev), _ptr(out),
                                       _rows(out, "out"), M, D, int(N), _stream()), "itts_allpass_warp_fwd")
    return out


def allpass_warp_bwd(dy, x, alpha, N, mean=None, std_dev=None):
    """(dx [M, D], dalpha [M]) of allpass_warp_fwd for dy = dL/dy; the warp is recomputed from alpha."""
    L = _lib.load()
    M, D = _allpass_operands(x, alpha, mean, std_dev, N)
    _need(dy, torch.float32, "dy")
    if dy.shape != x.shape:
        raise ValueError("dy must have the shape of x")
    dx = torch.empty((M, D), dtype=torch.float32, device=x.device)
    dalpha = torch.empty((M,), dtype=torch.float32, device=x.device)
    _lib.check(L.itts_allpass_warp_bwd(_ptr(dy), _rows(dy, "dy"), _ptr(x), _rows(x, "x"), _ptr(alpha), _ptr(mean),
                                       _ptr(std_dev), _ptr(dx), _rows(dx, "dx"), _ptr(dalpha), M, D, int(N),
                                       _stream()), "itts_allpass_warp_bwd")
    return dx, dalpha


POOL_LAST, POOL_MEAN = 0, 1      # ITTS_POOL_* in include/idiaptts_amd.h


def time_pool_plan(n_utts, t_max, width):
    """(segments, split, workspace bytes) of a MEAN pooling call of that shape (itts_time_pool_plan; no device work):
    `split` when every 128-row segment of time gets a workgroup and a second launch adds the segment sums."""
    L = _lib.load()
    seg, split, nbytes = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    if L.itts_time_pool_plan(int(n_utts), int(t_max), int(width), ctypes.byref(seg), ctypes.byref(split),
                             ctypes.byref(nbytes)) != 0:
        raise ValueError("no pooling plan for n_utts={}, t_max={}, width={}".format(n_utts, t_max, width))
    return seg.value, bool(split.value), nbytes.value


def pool_pitch(t):
    """The position pitch of a padded batch [B, T, D] / [T, B, D] whose positions are evenly spaced rows of unit
    stride, else None.  (The stride of an extent of 1 says nothing: `contiguous()` leaves any value there.)"""
    if t.dim() != 3 or (t.shape[2] > 1 and t.stride(2) != 1):
        return None
    n0, n1, width = t.shape
    if n1 > 1:
        ld = t.stride(1)
        if n0 > 1 and t.stride(0) != ld * n1:
            return None
    else:
        ld = t.stride(0) if n0 > 1 else width
    return ld if ld >= max(width, 1) else None


def _pool_pitch(t, name):
    ld = pool_pitch(t)
    if ld is None:
        raise ValueError("{} must be a 3-D padded batch of evenly spaced rows with unit stride".format(name))
    return ld


def _pool_lens(lens, n_utts, t_max, mode, device):
    """int64 lengths on the device; a host tensor (or list) is checked for 1 <= len <= t_max first"""
    if lens is None:
        if mode == POOL_MEAN:
            raise ValueError("mean pooling divides by the lengths: lens is None")
        return None
    if torch.is_tensor(lens) and lens.is_cuda and lens.dtype == torch.int64 and lens.dim() == 1 \
            and lens.is_contiguous() and lens.numel() == n_utts:
        return lens                      # (what the autograd node hands over: nothing to convert on the step's path)
    if not torch.is_tensor(lens) or not lens.is_cuda:
        lens = torch.as_tensor(lens, dtype=torch.int64).reshape(-1)
        if lens.numel() and (int(lens.min()) < 1 or int(lens.max()) > t_max):
            raise ValueError("sequence lengths must lie in 1 .. t_max = {}, got {} .. {}"
                             .format(t_max, int(lens.min()), int(lens.max())))
        lens = lens.to(device)
    lens = lens.reshape(-1).to(torch.int64).contiguous()
    if lens.numel() != n_utts:
        raise ValueError("{} lengths for {} utterances".format(lens.numel(), n_utts))
    return lens


def time_pool_fwd(x, lens, batch_first, mode, out=None):
    """[B, T, D] (batch_first) or [T, B, D] -> [B, D]: row len_b - 1 (POOL_LAST; row T - 1 when lens is None) or the
    sum over ALL T positions divided by len_b (POOL_MEAN) -- rnn_dyn/Pooling.py."""
    L = _lib.load()
    _need(x, torch.float32, "x")
    ld = _pool_pitch(x, "x")
    n_utts, t_max = (x.shape[0], x.shape[1]) if batch_first else (x.shape[1], x.shape[0])
    width = x.shape[2]
    lens = _pool_lens(lens, n_utts, t_max, mode, x.device)
    if out is None:
        out = torch.empty((n_utts, width), dtype=torch.float32, device=x.device)
    _need(out, torch.float32, "out")
    ws = None
    if mode == POOL_MEAN and n_utts > 0 and t_max > 0 and width > 0:
        nbytes = time_pool_plan(n_utts, t_max, width)[2]
        if nbytes:                       # (the segment sums of a time-split call, read back by its second launch)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    _lib.check(L.itts_time_pool_fwd(_ptr(x), ld, _ptr(lens), n_utts, t_max, width, 1 if batch_first else 0, int(mode),
                                    _ptr(out), _rows(out, "out"), _ptr(ws), _stream()), "itts_time_pool_fwd")
    return out


def time_pool_bwd(dy, lens, t_max, batch_first, mode, out=None):
    """dx [B, T, D] / [T, B, D] of time_pool_fwd for dy [B, D]; every position is written."""
    L = _lib.load()
    _need(dy, torch.float32, "dy")
    n_utts, width = dy.shape
    lens = _pool_lens(lens, n_utts, t_max, mode, dy.device)
    if out is None:
        shape = (n_utts, int(t_max), width) if batch_first else (int(t_max), n_utts, width)
        out = torch.empty(shape, dtype=torch.float32, device=dy.device)
    _need(out, torch.float32, "out")
    _lib.check(L.itts_time_pool_bwd(_ptr(dy), _rows(dy, "dy"), _ptr(lens), n_utts, int(t_max), width,
                                    1 if batch_first else 0, int(mode), _ptr(out), _pool_pitch(out, "out"),
                                    _stream()), "itts_time_pool_bwd")
    return out


def vae_reparam_fwd(h, eps, out=None):
    """z = eps * exp(0.5 * log_var) + mu for h [M, 2L] = mu | log_var and eps [M, L] (rnn_dyn/VAE.py:19-27)."""
    L = _lib.load()
    _need(h, torch.float32, "h")
    _need(eps, torch.float32, "eps")
    M, two_l = h.shape
    if two_l % 2 or eps.shape != (M, two_l // 2):
        raise ValueError("h must be [M, 2L] and eps [M, L], got {} and {}".format(tuple(h.shape), tuple(eps.shape)))
    lat = two_l // 2
    if out is None:
        out = torch.empty((M, lat), dtype=torch.float32, device=h.device)
    _need(out, torch.float32, "out")
    _lib.check(L.itts_vae_reparam_fwd(_ptr(h), _rows(h, "h"), _ptr(eps), _rows(eps, "eps"), _ptr(out),
                                      _rows(out, "out"), M, lat, _stream()), "itts_vae_reparam_fwd")
    return out


def vae_reparam_bwd(dz, dmu, dlv, h, eps, out=None):
    """dh [M, 2L] from the gradients into z, mu and log_var (each [M, L] or None) in one pass."""
    L = _lib.load()
    _need(h, torch.float32, "h")
    M, two_l = h.shape
    lat = two_l // 2
    for name, t in (("dz", dz), ("dmu", dmu), ("dlv", dlv), ("eps", eps)):
        if t is not None:
            _need(t, torch.float32, name)
            if t.shape != (M, lat):
                raise ValueError("{} must be [{}, {}], got {}".format(name, M, lat, tuple(t.shape)))
    if out is None:
        out = torch.empty((M, two_l), dtype=torch.float32, device=h.device)
    _need(out, torch.float32, "out")

    def ld(t, name):
        return _rows(t, name) if t is not None else 0
    _lib.check(L.itts_vae_reparam_bwd(_ptr(dz), ld(dz, "dz"), _ptr(dmu), ld(dmu, "dmu"), _ptr(dlv), ld(dlv, "dlv"),
                                      _ptr(h), _rows(h, "h"), _ptr(eps), ld(eps, "eps"), _ptr(out), _rows(out, "out"),
                                      M, lat, _stream()), "itts_vae_reparam_bwd")
    return out


def vae_kld(mu, log_var, row_weight, want_grad=True, want_elem=False, dmu=None, dlv=None):
    """sum_r w[r] * 0.5 * sum_c (exp(lv) + mu^2 - 1 - lv) on [M, L] rows (loss/VAEKLDLoss.py:56-58):
    (loss [1], dmu or None, dlv or None, per-row values [M] or None).  mu and log_var may be the two halves of one
    [M, 2L] tensor; rows of weight 0 may hold anything."""
    L = _lib.load()
    _need(mu, torch.float32, "mu")
    _need(log_var, torch.float32, "log_var")
    _need(row_weight, torch.float32, "row_weight")
    M, lat = mu.shape
    if log_var.shape != mu.shape or row_weight.numel() != M:
        raise ValueError("mu {} / log_var {} / row_weight {} do not match".format(
            tuple(mu.shape), tuple(log_var.shape), tuple(row_weight.shape)))
    loss = torch.empty((1,), dtype=torch.float32, device=mu.device)
    if want_grad:
        dmu = torch.empty((M, lat), dtype=torch.float32, device=mu.device) if dmu is None else dmu
        dlv = torch.empty((M, lat), dtype=torch.float32, device=mu.device) if dlv is None else dlv
    else:
        dmu = dlv = None
    elem = torch.empty((M,), dtype=torch.float32, device=mu.device) if want_elem else None
    ws = torch.empty(max(L.itts_vae_kld_workspace_bytes(M, lat), 8), dtype=torch.uint8, device=mu.device)
    _lib.check(L.itts_vae_kld(_ptr(mu), _rows(mu, "mu"), _ptr(log_var), _rows(log_var, "log_var"),
                              _ptr(row_weight.reshape(-1).contiguous()), M, lat, _ptr(loss),
                              _ptr(dmu), _rows(dmu, "dmu") if dmu is not None else 0,
                              _ptr(dlv), _rows(dlv, "dlv") if dlv is not None else 0, _ptr(elem), _ptr(ws), _stream()),
               "itts_vae_kld")
    return loss, dmu, dlv, elem


XENT_ROWS, XENT_STRIDED = 0, 1      # ITTS_XENT_* in include/idiaptts_amd.h
XENT_LAYOUTS = {"rows": XENT_ROWS, "strided": XENT_STRIDED, XENT_ROWS: XENT_ROWS, XENT_STRIDED: XENT_STRIDED}
XENT_MAX_CLASSES = 4096
CONF_MAX_CLASSES = 1024


def xent_plan(N, C, layout="rows"):
    """(lanes a row, steps of 4 * lanes columns) of a softmax cross-entropy call (itts_xent_plan; no device work):
    class-contiguous rows ("rows") share 1, 2, 4 .. 64 lanes, the smallest power of two with 4 * lanes >= C, and
    take 2 .. 16 steps from C = 257 on; the class-strided layout ("strided") reports (4, ceil(C / 4)): the waves
    that share a frame and the classes each of them takes (kept in registers up to 64, read again above)."""
    L = _lib.load()
    if layout not in XENT_LAYOUTS:
        raise ValueError("unknown layout {!r}".format(layout))
    lanes, steps = ctypes.c_int(0), ctypes.c_int(0)
    if L.itts_xent_plan(int(N), int(C), XENT_LAYOUTS[layout], ctypes.byref(lanes), ctypes.byref(steps)) != 0:
        raise ValueError("no cross-entropy plan for N={}, C={}".format(N, C))
    return lanes.value, steps.value


def _xent_common(class_weight, row_weight, C, n_rows):
    _need(row_weight, torch.float32, "row_weight")
    if row_weight.numel() != n_rows:
        raise ValueError("row_weight has {} entries for {} rows".format(row_weight.numel(), n_rows))
    if class_weight is not None:
        _need(class_weight, torch.float32, "class_weight")
        if class_weight.numel() != C:
            raise ValueError("class_weight has {} entries for {} classes".format(class_weight.numel(), C))
        class_weight = class_weight.reshape(-1).contiguous()
    return class_weight, row_weight.reshape(-1).contiguous()


def softmax_xent(x, target, row_weight, class_weight=None, ignore_index=-100, want_grad=True, want_elem=False,
                 grad=None):
    """Row-weighted softmax cross-entropy of class-contiguous logits x [N, C] (contiguous rows, any pitch) with
    int64 targets [N] (itts_softmax_xent): (loss [1] = sum_r w[r] l_r, grad [N, C] or None, w[r] l_r [N] or None)."""
    L = _lib.load()
    _need(x, torch.float32, "x")
    _need(target, torch.int64, "target")
    N, C = x.shape
    if target.numel() != N:
        raise ValueError("target has {} entries for {} rows".format(target.numel(), N))
    class_weight, row_weight = _xent_common(class_weight, row_weight, C, N)
    loss = torch.empty((1,), dtype=torch.float32, device=x.device)
    if want_grad and grad is None:
        grad = torch.empty((N, C), dtype=torch.float32, device=x.device)
    if not want_grad:
        grad = None
    if grad is not None:
        _need(grad, torch.float32, "grad")
        if grad.shape != x.shape:
            raise ValueError("grad must have the shape of x")
    elem = torch.empty((N,), dtype=torch.float32, device=x.device) if want_elem else None
    ws = torch.empty(max(L.itts_softmax_xent_workspace_bytes(N, C), 8), dtype=torch.uint8, device=x.device)
    _lib.check(L.itts_softmax_xent(_ptr(x), _rows(x, "x"), _ptr(target.reshape(-1).contiguous()), _ptr(class_weight),
                                   _ptr(row_weight), N, C, int(ignore_index), _ptr(loss), _ptr(elem), _ptr(grad),
                                   _rows(grad, "grad") if grad is not None else 0, _ptr(ws), _stream()),
               "itts_softmax_xent")
    return loss, grad, elem


def softmax_xent_strided(x, onehot, row_weight, class_weight=None, ignore_index=-100, shift=None, want_grad=True,
                         want_elem=False):
    """The same loss on class-strided logits x [B, C, T] (contiguous) with a one-hot target of the same shape
    (itts_softmax_xent_strided; loss/OneHotCrossEntropyLoss.py): frame t of the input is scored against the arg-max
    of onehot[:, :, t + shift]; row_weight and the per-frame values are [B, T - shift], grad is [B, C, T]."""
    L = _lib.load()
    _need(x, torch.float32, "x")
    _need(onehot, torch.float32, "onehot")
    if x.dim() != 3 or onehot.shape != x.shape:
        raise ValueError("x and onehot must both be [B, C, T], got {} and {}".format(tuple(x.shape),
                                                                                   tuple(onehot.shape)))
    x, onehot = x.contiguous(), onehot.contiguous()
    B, C, T = x.shape
    shift = int(shift or 0)
    if B > 0 and not 0 <= shift < max(T, 1):
        raise ValueError("shift = {} is outside 0 .. T - 1 = {}".format(shift, T - 1))
    Tn = T - shift
    class_weight, row_weight = _xent_common(class_weight, row_weight, C, B * Tn)
    loss = torch.empty((1,), dtype=torch.float32, device=x.device)
    grad = torch.empty((B, C, T), dtype=torch.float32, device=x.device) if want_grad else None
    elem = torch.empty((B, Tn), dtype=torch.float32, device=x.device) if want_elem else None
    ws = torch.empty(max(L.itts_softmax_xent_strided_workspace_bytes(B, T), 8), dtype=torch.uint8, device=x.device)
    _lib.check(L.itts_softmax_xent_strided(_ptr(x), _ptr(onehot), _ptr(class_weight), _ptr(row_weight), B, C, T,
                                           shift, int(ignore_index), _ptr(loss), _ptr(elem), _ptr(grad), _ptr(ws),
                                           _stream()), "itts_softmax_xent_strided")
    return loss, grad, elem


def class_counts(x, target=None, want_pred=True, correct=None, conf=None):
    """Arg-max over the classes of x [N, C] with torch.argmax's order (itts_class_counts): (pred [N] int64 or None,
    correct [1] int64, conf [C, C] int64).  `correct` and `conf` (rows = true class) are ADDED to when given, fresh
    zeros otherwise; without `target` only the predictions are made and both come back as None."""
    L = _lib.load()
    _need(x, torch.float32, "x")
    N, C = x.shape
    pred = torch.empty((N,), dtype=torch.int64, device=x.device) if want_pred else None
    if target is None:
        correct = conf = None
    else:
        _need(target, torch.int64, "target")
        if target.numel() != N:
            raise ValueError("target has {} entries for {} rows".format(target.numel(), N))
        target = target.reshape(-1).contiguous()
        if C > CONF_MAX_CLASSES and conf is None:
            raise ValueError("a confusion matrix of C = {} classes exceeds the {} it takes".format(
                C, CONF_MAX_CLASSES))
        if correct is None:
            correct = torch.zeros((1,), dtype=torch.int64, device=x.device)
        if conf is None:
            conf = torch.zeros((C, C), dtype=torch.int64, device=x.device)
        for name, t, shape in (("correct", correct, (1,)), ("conf", conf, (C, C))):
            _need(t, torch.int64, name)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("{} must be a contiguous int64 {}".format(name, shape))
    _lib.check(L.itts_class_counts(_ptr(x), _rows(x, "x"), _ptr(target), N, C, _ptr(pred), _ptr(correct), _ptr(conf),
                                   _stream()), "itts_class_counts")
    return pred, correct, conf


def weighted_loss(pred, target, row_weight, kind, want_grad=True, want_elem=False):
    """sum_r w[r] sum_c e(pred - target) on [M, D] rows, e squared (kind 0) / absolute (kind 1)
    error: (loss [1], grad or None, elementwise values or None)."""
    L = _lib.load()
    _need(pred, torch.float32, "pred")
    _need(target, torch.float32, "target")
    _need(row_weight, torch.float32, "row_weight")
    M, D = pred.shape
    loss = torch.empty((1,), dtype=torch.float32, device=pred.device)
    grad = torch.empty((M, D), dtype=torch.float32, device=pred.device) if want_grad else None
    elem = torch.empty((M, D), dtype=torch.float32, device=pred.device) if want_elem else None
    ws = torch.empty(max(L.itts_masked_mse_workspace_bytes(M, D), 8), dtype=torch.uint8,
                     device=pred.device)
    _lib.check(L.itts_weighted_loss(_ptr(pred), _rows(pred, "pred"), _ptr(target),
                                    _rows(target, "target"), _ptr(row_weight.contiguous()), M, D,
                                    int(kind), _ptr(loss), _ptr(grad), D if want_grad else 0,
                                    _ptr(elem), D if want_elem else 0, _ptr(ws), _stream()),
               "itts_weighted_loss")
    return loss, grad, elem


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
              weight_decay=0.0, grad_scale=1.0):
    L = _lib.load()
    for t, n in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"),
                 (exp_avg_sq, "exp_avg_sq")):
        _need(t, torch.float32, n)
        if not t.is_contiguous():
            raise ValueError(n + " must be contiguous")
    _lib.check(L.itts_adam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq),
                                param.numel(), lr, betas[0], betas[1], eps, weight_decay,
                                int(step), grad_scale, _stream()), "itts_adam_step")


def grad_norm_accum(x, accum, norm_kind=2, accumulate=False):
    """accum[0] (+)= sum x^2 (norm_kind 2) or max(accum[0], max |x|) (norm_kind 0 = infinity norm)
    of a flat f32 buffer; the input of the clipping inside adam_step_fused."""
    L = _lib.load()
    _need(x, torch.float32, "x")
    _need(accum, torch.float32, "accum")
    if not x.is_contiguous():
        raise ValueError("x must be contiguous")
    _lib.check(L.itts_grad_norm_accum(_ptr(x), x.numel(), int(norm_kind), _ptr(accum),
                                      int(bool(accumulate)), _ptr(_workspace(4096, x.device)),
                                      _stream()), "itts_grad_norm_accum")
    return accum


def adam_step_fused(param, grad, exp_avg, exp_avg_sq, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                    weight_decay=0.0, grad_scale=1.0, norm_accum=None, norm_kind=2,
                    clip_max_norm=0.0, clip_value=0.0, ema_shadow=None, ema_decay=0.0):
    """Gradient clipping (by norm from `norm_accum`, by value), Adam and the parameter EMA in one
    pass over flat f32 buffers."""
    L = _lib.load()
    for t, n in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"),
                 (exp_avg_sq, "exp_avg_sq")) + \
            (((ema_shadow, "ema_shadow"),) if ema_shadow is not None else ()):
        _need(t, torch.float32, n)
        if not t.is_contiguous() or t.numel() != param.numel():
            raise ValueError(n + " must be contiguous and as long as param")
    _lib.check(L.itts_adam_step_fused(
        _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), lr, betas[0],
        betas[1], eps, weight_decay, int(step), grad_scale,
        _ptr(norm_accum) if norm_accum is not None else None, int(norm_kind),
        float(clip_max_norm), float(clip_value or 0.0),
        _ptr(ema_shadow) if ema_shadow is not None else None, float(ema_decay), _stream()),
        "itts_adam_step_fused")


def sgd_step(param, grad, momentum_buf=None, first_step=False, lr=1e-3, momentum=0.0,
             dampening=0.0, weight_decay=0.0, nesterov=False, grad_scale=1.0):
    L = _lib.load()
    for t, n in ((param, "param"), (grad, "grad")) + \
            (((momentum_buf, "momentum_buf"),) if momentum_buf is not None else ()):
        _need(t, torch.float32, n)
        if not t.is_contiguous():
            raise ValueError(n + " must be contiguous")
    _lib.check(L.itts_sgd_step(_ptr(param), _ptr(grad),
                               _ptr(momentum_buf) if momentum_buf is not None else None,
                               param.numel(), lr, momentum, dampening, weight_decay,
                               int(bool(nesterov)), int(bool(first_step)), grad_scale,
                               _stream()), "itts_sgd_step")


def ema_update(shadow, param, decay):
    L = _lib.load()
    for t, n in ((shadow, "shadow"), (param, "param")):
        _need(t, torch.float32, n)
        if not t.is_contiguous():
            raise ValueError(n + " must be contiguous")
    _lib.check(L.itts_ema_update(_ptr(shadow), _ptr(param), shadow.numel(), float(decay),
                                 _stream()), "itts_ema_update")


GemmPathCounts = collections.namedtuple("GemmPathCounts", "ring staged")


def gemm_path_counts():
    """Which kernel the dense-layer products of this process ran on so far (itts_gemm_path_counts; no device call):
    `ring` and `staged` are 4-tuples indexed by the epilogue kind (0 store, 1 bias + activation, 2 activation
    derivative, 3 masked MSE)."""
    out = (ctypes.c_int64 * 8)()
    _lib.check(_lib.load().itts_gemm_path_counts(out), "itts_gemm_path_counts")
    v = [int(x) for x in out]
    return GemmPathCounts(tuple(v[:4]), tuple(v[4:]))


GEMM_KERNELS = {1: "staged", 2: "ring", 3: "ring_pair"}
GEMM_EPILOGUES = {0: "store", 1: "bias_act", 2: "dact", 3: "mse"}
GemmLaunch = collections.namedtuple("GemmLaunch", "kernel a_row b_row epi tn stages wm vec_a vec_b wide grouped splitk "
                                                  "family tiles grid dropout")
SlabReduction = collections.namedtuple("SlabReduction", "vec merged deferred slabs")
GEMM_PLAN_MAX = 8                # kPlanMax of csrc/nn.hip


def gemm_last_plan():
    """What the last dense call of this host thread launched (linear_fwd, linear_fwd_mse, linear_bwd_input,
    linear_bwd_weight, linear_bwd; itts_gemm_last_plan, no device call): a list, in launch order, of
    GemmLaunch(kernel "staged" / "ring" / "ring_pair", a_row, b_row, epi "store" / "bias_act" / "dact" / "mse", tn and
    stages (staged; 0 otherwise), wm (ring; 0 otherwise), vec_a, vec_b, wide (the wide-store epilogue), grouped (tile
    order), splitk, family (0 base, 1 extended activations), tiles, grid, dropout (the epilogue applied it)) -- a pair
    launch gives two, the weight and
    the input product -- and SlabReduction(vec: float4 or scalar columns, merged with the bias, deferred, slabs)."""
    L = _lib.load()
    out = (ctypes.c_int32 * (16 * GEMM_PLAN_MAX))()
    n = L.itts_gemm_last_plan(out, GEMM_PLAN_MAX)
    if n > GEMM_PLAN_MAX:
        raise _lib.IttsError("the record holds {} launches, the call made {}".format(GEMM_PLAN_MAX, n))
    plan = []
    for i in range(n):
        v = [int(x) for x in out[16 * i:16 * i + 16]]
        if v[0] == 4:
            plan.append(SlabReduction(bool(v[1]), bool(v[2]), bool(v[3]), v[4]))
        else:
            plan.append(GemmLaunch(GEMM_KERNELS[v[0]], bool(v[1]), bool(v[2]), GEMM_EPILOGUES[v[3]], v[4], v[5], v[6],
                                   bool(v[7]), bool(v[8]), bool(v[9]), bool(v[10]), v[11], v[12], v[13], v[14], bool(v[15])))
    return plan


RnnPathCounts = collections.namedtuple("RnnPathCounts", "fwd_ran fwd_declined fwd_gave_up bwd_ran bwd_declined bwd_gave_up")


def rnn_path_counts():
    """Which way the LSTM / GRU layer calls of this process went so far (itts_rnn_path_counts; no device call): per
    recurrence, `ran` = the persistent kernel did the layer, `declined` = it was not launched and the per-step
    kernels did it, `gave_up` = a persistent launch failed or gave up waiting and the per-step kernels redid it."""
    out = (ctypes.c_int64 * 6)()
    _lib.check(_lib.load().itts_rnn_path_counts(out), "itts_rnn_path_counts")
    return RnnPathCounts(*[int(v) for v in out])


RnnLayerCounts = collections.namedtuple("RnnLayerCounts", "fwd bwd")


def rnn_layer_counts():
    """Forward and backward vanilla RNN layer calls of this process so far (itts_rnn_layer_counts; no device call).
    rnn_path_counts() does not count them: they have no persistent kernel to run on or be declined by."""
    out = (ctypes.c_int64 * 2)()
    _lib.check(_lib.load().itts_rnn_layer_counts(out), "itts_rnn_layer_counts")
    return RnnLayerCounts(int(out[0]), int(out[1]))



# ------------------------------------------------------------------------- WORLD frame kernels
def _c_int_ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def cheaptrick_mcep(x, x_off, f0, f_off, fs, frame_period=5.0, fft_size=None, q1=-0.15,
                    want_sp=True, order=None, alpha=None, eps=1e-8, miniter=2, maxiter=30,
                    threshold=1e-3, mc_dtype=torch.float32, want_iters=False):
    """CheapTrick (+ fused SPTK mcep when `order` is given) for utterances stored back to back.
    x f64 [Ntot], f0 f64 [Ttot]; x_off / f_off python lists (U+1). Returns (sp or None,
    mcep or None, iters or None)."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    _need(f0, torch.float64, "f0")
    fft_size = fft_size or L.itts_cheaptrick_fft_size(fs, 71.0)
    T = int(f_off[-1])
    K = fft_size // 2 + 1
    sp = torch.empty((T, K), dtype=torch.float64, device=x.device) if want_sp else None
    mc32 = mc64 = iters = None
    if order is not None:
        if mc_dtype == torch.float32:
            mc32 = torch.empty((T, order + 1), dtype=torch.float32, device=x.device)
        else:
            mc64 = torch.empty((T, order + 1), dtype=torch.float64, device=x.device)
        if want_iters:
            iters = torch.empty((T,), dtype=torch.int32, device=x.device)
    _lib.check(L.itts_cheaptrick_mcep(_ptr(x), _lib.offsets_array(x_off), _ptr(f0),
                                      _lib.offsets_array(f_off), len(x_off) - 1, fs,
                                      float(frame_period), fft_size, q1, _ptr(sp),
                                      order if order is not None else 0,
                                      float(alpha) if alpha is not None else 0.0, eps, miniter,
                                      maxiter, threshold, _ptr(mc32), (order or 0) + 1, _ptr(mc64),
                                      _ptr(iters), _stream()), "itts_cheaptrick_mcep")
    return sp, (mc32 if mc32 is not None else mc64), iters


def mcep(amp_sp, order, alpha, eps=1e-8, miniter=2, maxiter=30, threshold=1e-3,
         dtype=torch.float32, want_iters=False):
    """pysptk.mcep(amp_sp, order, alpha, eps, etype=1, itype=3) on [T, K] f64 (GPU)."""
    L = _lib.load()
    _need(amp_sp, torch.float64, "amp_sp")
    amp_sp = amp_sp.contiguous()
    T, K = amp_sp.shape
    out = torch.empty((T, order + 1), dtype=dtype, device=amp_sp.device)
    iters = torch.empty((T,), dtype=torch.int32, device=amp_sp.device) if want_iters else None
    f32 = out if dtype == torch.float32 else None
    f64 = out if dtype == torch.float64 else None
    _lib.check(L.itts_mcep(_ptr(amp_sp), T, K, order, float(alpha), eps, miniter, maxiter,
                           threshold, _ptr(f32), order + 1, _ptr(f64), _ptr(iters), _stream()),
               "itts_mcep")
    return (out, iters) if want_iters else out


def mgc2sp(mc, alpha, fftlen, want_logamp=False, want_pow=False):
    """exp(float32(pysptk.mgc2sp(mc, alpha, 0, fftlen).real)) -> [T, fftlen/2+1] f32
    (or the f64 log amplitude when want_logamp, or the f64 power spectrum when want_pow)."""
    L = _lib.load()
    _need(mc, torch.float64, "mc")
    mc = mc.contiguous()
    T, m1 = mc.shape
    K = fftlen // 2 + 1
    out32 = None if (want_logamp or want_pow) else torch.empty((T, K), dtype=torch.float32,
                                                               device=mc.device)
    out64 = torch.empty((T, K), dtype=torch.float64, device=mc.device) if want_logamp else None
    outpw = torch.empty((T, K), dtype=torch.float64, device=mc.device) if want_pow else None
    _lib.check(L.itts_mgc2sp(_ptr(mc), T, m1 - 1, float(alpha), fftlen, _ptr(out32), _ptr(out64),
                             _ptr(outpw), _stream()), "itts_mgc2sp")
    return out64 if want_logamp else (outpw if want_pow else out32)


def mgcep(sp, order, alpha, gamma, eps=1e-8, miniter=2, maxiter=30, threshold=1e-3,
          dtype=torch.float32, want_iters=False, input_is_power=False):
    """pysptk.mgcep(amp_sp, order, alpha, gamma, eps, min_det=0, etype=1, itype=3) on [T, K] f64
    amplitude spectra (or power spectra with input_is_power)."""
    L = _lib.load()
    _need(sp, torch.float64, "sp")
    sp = sp.contiguous()
    T, K = sp.shape
    out = torch.empty((T, order + 1), dtype=dtype, device=sp.device)
    iters = torch.empty((T,), dtype=torch.int32, device=sp.device) if want_iters else None
    f32 = out if dtype == torch.float32 else None
    f64 = out if dtype == torch.float64 else None
    _lib.check(L.itts_mgcep(_ptr(sp), 1 if input_is_power else 0, T, K, order, float(alpha),
                            float(gamma), eps, miniter, maxiter, threshold, _ptr(f32), order + 1,
                            _ptr(f64), _ptr(iters), _stream()), "itts_mgcep")
    return (out, iters) if want_iters else out


def mgc2sp_gamma(mgc, alpha, gamma, fftlen, want_logamp=False, want_pow=False):
    """exp(float32(pysptk.mgc2sp(mgc, alpha, gamma, fftlen).real)) -> [T, fftlen/2+1] f32 (or the f64
    log amplitude / f64 power spectrum)."""
    L = _lib.load()
    _need(mgc, torch.float64, "mgc")
    mgc = mgc.contiguous()
    T, m1 = mgc.shape
    K = fftlen // 2 + 1
    out32 = None if (want_logamp or want_pow) else torch.empty((T, K), dtype=torch.float32,
                                                               device=mgc.device)
    out64 = torch.empty((T, K), dtype=torch.float64, device=mgc.device) if want_logamp else None
    outpw = torch.empty((T, K), dtype=torch.float64, device=mgc.device) if want_pow else None
    _lib.check(L.itts_mgc2sp_gamma(_ptr(mgc), T, m1 - 1, float(alpha), float(gamma), fftlen,
                                   _ptr(out32), _ptr(out64), _ptr(outpw), _stream()),
               "itts_mgc2sp_gamma")
    return out64 if want_logamp else (outpw if want_pow else out32)


def code_aperiodicity(ap, fs, dtype=torch.float64):
    L = _lib.load()
    _need(ap, torch.float64, "ap")
    ap = ap.contiguous()
    T, K = ap.shape
    nap = L.itts_num_aperiodicities(fs)
    out = torch.empty((T, nap), dtype=dtype, device=ap.device)
    _lib.check(L.itts_code_aperiodicity(_ptr(ap), T, (K - 1) * 2, fs,
                                        _ptr(out) if dtype == torch.float64 else None,
                                        _ptr(out) if dtype == torch.float32 else None, _stream()),
               "itts_code_aperiodicity")
    return out


def decode_aperiodicity(bap, fs, fft_size, voiced_f0=None):
    """pyworld.decode_aperiodicity: bap [T, nap] f64 -> ap [T, fft_size / 2 + 1] f64.  With `voiced_f0` (f0 [T] f64)
    only the rows the synthesis of that contour can read -- voiced frames and their neighbours -- are decoded, the
    others are uninitialised memory: for world_synthesize and nothing else."""
    L = _lib.load()
    _need(bap, torch.float64, "bap")
    bap = bap.contiguous()
    T = bap.shape[0]
    out = torch.empty((T, fft_size // 2 + 1), dtype=torch.float64, device=bap.device)
    if voiced_f0 is not None:
        _need(voiced_f0, torch.float64, "voiced_f0")
        if voiced_f0.numel() != T:
            raise ValueError("voiced_f0 and bap differ in frames")
        _lib.check(L.itts_decode_aperiodicity_voiced(_ptr(bap), _ptr(voiced_f0.contiguous()), T, fs, fft_size,
                                                     _ptr(out), _stream()), "itts_decode_aperiodicity_voiced")
        return out
    _lib.check(L.itts_decode_aperiodicity(_ptr(bap), T, fs, fft_size, _ptr(out), _stream()),
               "itts_decode_aperiodicity")
    return out


def dio(x, x_off, f_off, fs, frame_period=5.0, f0_floor=71.0, f0_ceil=800.0,
        channels_in_octave=2.0, allowed_range=0.1):
    """pyworld.dio for utterances stored back to back -> f0 [Ttot] f64."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    f0 = torch.empty((int(f_off[-1]),), dtype=torch.float64, device=x.device)
    _lib.check(L.itts_dio(_ptr(x), _lib.offsets_array(x_off), _lib.offsets_array(f_off),
                          len(x_off) - 1, fs, float(frame_period), f0_floor, f0_ceil,
                          channels_in_octave, allowed_range, _ptr(f0), _stream()), "itts_dio")
    return f0


def harvest_num_frames(n_samples, fs, frame_period=5.0):
    return int(_lib.load().itts_harvest_num_frames(int(n_samples), int(fs), float(frame_period)))


def harvest(x, x_off, f_off, fs, frame_period=5.0, f0_floor=71.0, f0_ceil=800.0, stages=False):
    """pyworld.harvest for utterances stored back to back: f0 [Ttot] f64 (frame counts from
    harvest_num_frames).  stages=True (one utterance): also a dict with the raw band candidates,
    the refined candidates / scores and the 1 ms contour before smoothing."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    f0 = torch.empty((int(f_off[-1]),), dtype=torch.float64, device=x.device)
    dbg = {}
    ptrs = [None, None, None, None]
    if stages:
        import math
        assert len(x_off) == 2, "stages are returned for a single utterance"
        nch = 1 + int(math.log(f0_ceil * 1.1 / (f0_floor * 0.9)) / math.log(2.0) * 40.0)
        maxc = int(nch / 10.0 + 0.5) * 7
        T1 = harvest_num_frames(int(x_off[1]) - int(x_off[0]), fs, 1.0)
        dbg = dict(raw=torch.zeros((nch, T1), dtype=torch.float64, device=x.device),
                   cand=torch.zeros((T1, maxc), dtype=torch.float64, device=x.device),
                   score=torch.zeros((T1, maxc), dtype=torch.float64, device=x.device),
                   best=torch.zeros((T1,), dtype=torch.float64, device=x.device))
        ptrs = [_ptr(dbg[k]) for k in ("raw", "cand", "score", "best")]
    _lib.check(L.itts_harvest(_ptr(x), _lib.offsets_array(x_off), _lib.offsets_array(f_off),
                              len(x_off) - 1, fs, float(frame_period), float(f0_floor),
                              float(f0_ceil), _ptr(f0), ptrs[0], ptrs[1], ptrs[2], ptrs[3],
                              _stream()), "itts_harvest")
    return (f0, dbg) if stages else f0


def wav2world(x, x_off, f_off, fs, frame_period=5.0, fft_size=None, want_sp=True, want_ap=True):
    """pyworld.wav2world for utterances stored back to back: (f0 [Ttot], sp [Ttot, K] or None,
    ap [Ttot, K] or None), all f64 (WorldFeatLabelGen.py:792-793)."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    fft_size = fft_size or L.itts_cheaptrick_fft_size(fs, 71.0)
    T, K = int(f_off[-1]), fft_size // 2 + 1
    f0 = torch.empty((T,), dtype=torch.float64, device=x.device)
    sp = torch.empty((T, K), dtype=torch.float64, device=x.device) if want_sp else None
    ap = torch.empty((T, K), dtype=torch.float64, device=x.device) if want_ap else None
    _lib.check(L.itts_wav2world(_ptr(x), _lib.offsets_array(x_off), _lib.offsets_array(f_off),
                                len(x_off) - 1, fs, float(frame_period), fft_size, _ptr(f0),
                                _ptr(sp), _ptr(ap), _stream()), "itts_wav2world")
    return f0, sp, ap


def stonemask(x, x_off, f0, f_off, fs, frame_period=5.0):
    L = _lib.load()
    _need(x, torch.float64, "x")
    _need(f0, torch.float64, "f0")
    out = torch.empty_like(f0)
    _lib.check(L.itts_stonemask(_ptr(x), _lib.offsets_array(x_off), _ptr(f0),
                                _lib.offsets_array(f_off), len(x_off) - 1, fs,
                                float(frame_period), _ptr(out), _stream()), "itts_stonemask")
    return out


def d4c(x, x_off, f0, f_off, fs, frame_period=5.0, fft_size=None, threshold=0.85, want_ap=True,
        want_bap=None):
    """pyworld.d4c (+ optional fused code_aperiodicity). want_bap: None | torch.float64 | float32.
    Returns (ap or None, bap or None)."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    _need(f0, torch.float64, "f0")
    fft_size = fft_size or L.itts_cheaptrick_fft_size(fs, 71.0)
    T = int(f_off[-1])
    nap = L.itts_num_aperiodicities(fs)
    ap = torch.empty((T, fft_size // 2 + 1), dtype=torch.float64, device=x.device) if want_ap \
        else None
    bap = torch.empty((T, nap), dtype=want_bap, device=x.device) if want_bap is not None else None
    _lib.check(L.itts_d4c(_ptr(x), _lib.offsets_array(x_off), _ptr(f0), _lib.offsets_array(f_off),
                          len(x_off) - 1, fs, float(frame_period), fft_size, threshold, _ptr(ap),
                          _ptr(bap) if want_bap == torch.float64 else None,
                          _ptr(bap) if want_bap == torch.float32 else None, nap, _stream()),
               "itts_d4c")
    return ap, bap


def synth_offsets(f_off, fs, frame_period=5.0):
    """Sample offsets of the synthesised utterances for the frame offsets f_off (pyworld.synthesize's output lengths)."""
    L = _lib.load()
    y_off = [0]
    for u in range(len(f_off) - 1):
        y_off.append(y_off[-1] + L.itts_world_synth_length(int(f_off[u + 1] - f_off[u]), fs,
                                                           float(frame_period)))
    return y_off


def world_synthesize(f0, sp, ap, f_off, fs, frame_period=5.0, preemphasis=0.0,
                     dtype=torch.float32, spectra_ready=None, y_off=None, ap_ready=None):
    """pyworld.synthesize + float32 cast + de-pre-emphasis for utterances stored back to back.
    Returns (y [Ytot], y_off list).  spectra_ready: a torch.cuda.Event recorded behind the producer of sp (and of ap,
    unless ap_ready is given: an event of its own behind the producer of ap) when they run on another stream: the part
    of the synthesis in front of the pulse kernels needs f0 only, the unvoiced pulses the envelope only."""
    L = _lib.load()
    for t, n in ((f0, "f0"), (sp, "sp"), (ap, "ap")):
        _need(t, torch.float64, n)
    sp = sp.contiguous()
    ap = ap.contiguous()
    K = sp.shape[1]
    fft_size = (K - 1) * 2
    if y_off is None:
        y_off = synth_offsets(f_off, fs, frame_period)
    y = torch.empty((y_off[-1],), dtype=dtype, device=f0.device)
    args = (_ptr(f0), _ptr(sp), _ptr(ap), _lib.offsets_array(f_off),
            _lib.offsets_array(y_off), len(f_off) - 1, fs,
            float(frame_period), fft_size, float(preemphasis),
            _ptr(y) if dtype == torch.float32 else None,
            _ptr(y) if dtype == torch.float64 else None, _stream())
    if spectra_ready is None:
        _lib.check(L.itts_world_synthesize(*args), "itts_world_synthesize")
    else:
        ap_ev = ap_ready if ap_ready is not None else spectra_ready
        _lib.check(L.itts_world_synthesize_after(*args, ctypes.c_void_p(spectra_ready.cuda_event),
                                                 ctypes.c_void_p(ap_ev.cuda_event)),
                   "itts_world_synthesize_after")
        cur = torch.cuda.current_stream(f0.device)
        sp.record_stream(cur)
        ap.record_stream(cur)
    return y, y_off


# ------------------------------------------------------------------------- corpus audio preparation
FIR_MAX_TAPS = 2047              # FIR_MAX_TAPS of csrc/audio_prep.hip
RESAMPLE_MAX_RATE = 1024         # RS_MAX_RATE
RMS_PAD = {"constant": 0, "reflect": 1}     # ITTS_PAD_*


def fir_filtfilt(x, offsets, taps, out=None):
    """scipy.signal.filtfilt(taps, [1], x_s) (padtype "odd", padlen 3 * len(taps)) of every float64 signal
    x[offsets[s]:offsets[s + 1]]; taps: float64 [numtaps] on the device, numtaps odd.  Returns y like x."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    _need(taps, torch.float64, "taps")
    x, taps = x.contiguous(), taps.contiguous()
    n_sig, numtaps = len(offsets) - 1, int(taps.numel())
    if out is None:
        out = torch.empty_like(x)
    _need(out, torch.float64, "out")
    # (torch's allocator, not the cached _workspace: a corpus batch's first pass is as large as the batch)
    ws = torch.empty((max(int(L.itts_fir_filtfilt_workspace_bytes(int(offsets[-1]), n_sig, numtaps)), 8),),
                     dtype=torch.uint8, device=x.device)
    _lib.check(L.itts_fir_filtfilt_batch(_ptr(x), _lib.offsets_array(offsets), n_sig, _ptr(taps), numtaps, _ptr(out),
                                         _ptr(ws), _stream()), "itts_fir_filtfilt_batch")
    return out


def resample_out_offsets(offsets, up, down):
    """Offsets of the resampled signals: ceil(n * up / down) samples each."""
    out = [0]
    for s in range(len(offsets) - 1):
        out.append(out[-1] + -((int(offsets[s + 1]) - int(offsets[s])) * up // -down))
    return out


def resample_poly(x, offsets, up, down, taps):
    """scipy.signal.resample_poly(x_s, up, down) of every float64 signal with the filter `taps` (float64 [2 * half + 1]
    on the device, already times up).  Returns (y, out_offsets)."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    _need(taps, torch.float64, "taps")
    x, taps = x.contiguous(), taps.contiguous()
    out_off = resample_out_offsets(offsets, up, down)
    y = torch.empty((out_off[-1],), dtype=torch.float64, device=x.device)
    _lib.check(L.itts_resample_poly_batch(_ptr(x), _lib.offsets_array(offsets), _lib.offsets_array(out_off),
                                          len(offsets) - 1, int(up), int(down), _ptr(taps), int(taps.numel()),
                                          _ptr(y), _stream()), "itts_resample_poly_batch")
    return y, out_off


def loudness_normalise(x, offsets, ref_rms=0.1, out=None):
    """(x_s - mean) * sqrt(n * ref_rms^2 / sum((x_s - mean)^2)) of every float64 signal."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    x = x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    _need(out, torch.float64, "out")
    _lib.check(L.itts_loudness_normalise_batch(_ptr(x), _lib.offsets_array(offsets), len(offsets) - 1, float(ref_rms),
                                               _ptr(out), _stream()), "itts_loudness_normalise_batch")
    return out


def frame_rms_offsets(offsets, frame_length, hop):
    """Frame offsets of librosa.feature.rms(center=True): 1 + n // hop frames per signal for an even frame_length."""
    out = [0]
    for s in range(len(offsets) - 1):
        padded = int(offsets[s + 1]) - int(offsets[s]) + 2 * (frame_length // 2)
        out.append(out[-1] + (1 + (padded - frame_length) // hop if padded >= frame_length else 0))
    return out


def frame_rms(x, offsets, frame_length, hop, pad_mode="constant"):
    """librosa.feature.rms(y=x_s, frame_length, hop_length=hop, center=True, pad_mode) of every float64 signal.
    Returns (rms [frames of all signals], frame offsets)."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    x = x.contiguous()
    if pad_mode not in RMS_PAD:
        raise ValueError("unknown pad_mode {!r} (constant, reflect)".format(pad_mode))
    f_off = frame_rms_offsets(offsets, int(frame_length), max(int(hop), 1))
    rms = torch.empty((f_off[-1],), dtype=torch.float64, device=x.device)
    _lib.check(L.itts_frame_rms_batch(_ptr(x), _lib.offsets_array(offsets), _lib.offsets_array(f_off),
                                      len(offsets) - 1, int(frame_length), int(hop), RMS_PAD[pad_mode], _ptr(rms),
                                      _stream()), "itts_frame_rms_batch")
    return rms, f_off


# ----------------------------------------------------------------------------- raw-waveform targets
MOL_MAX_MIXTURES = 64            # MOL_MAX_K of csrc/mol.hip
MULAW_MAX_MU = 65535


def mol_loss(x, y, row_weight, num_classes=256, log_scale_min=-7.0, shift=None, hinge=True, want_grad=True,
             want_elem=False):
    """Discretized mixture-of-logistics loss of x [B, 3K, T] (logits, means, log-scales; contiguous float32) against
    the targets y [B, 1, T] in [-1, 1] (itts_mol_loss; loss/DiscretizedMixturelogisticLoss.py): frame t of the input
    is scored against y[t + shift]; row_weight and the per-frame values are [B, T - shift], grad is [B, 3K, T].
    Returns (loss [1] = sum w l, grad or None, w l or None)."""
    L = _lib.load()
    _need(x, torch.float32, "x")
    _need(y, torch.float32, "y")
    if x.dim() != 3:
        raise ValueError("x must be [B, 3K, T], got {}".format(tuple(x.shape)))
    B, C, T = x.shape
    if C % 3 != 0:
        raise ValueError("C = {} channels is no multiple of 3 (logits, means, log-scales)".format(C))
    if y.numel() != B * T:
        raise ValueError("y must be [B, 1, T] = [{}, 1, {}], got {}".format(B, T, tuple(y.shape)))
    x, y = x.contiguous(), y.reshape(B, T).contiguous()
    shift = int(shift or 0)
    if B > 0 and not 0 <= shift < max(T, 1):
        raise ValueError("shift = {} is outside 0 .. T - 1 = {}".format(shift, T - 1))
    Tn = T - shift
    _need(row_weight, torch.float32, "row_weight")
    if row_weight.numel() != B * Tn:
        raise ValueError("row_weight has {} entries for {} rows".format(row_weight.numel(), B * Tn))
    row_weight = row_weight.reshape(-1).contiguous()
    loss = torch.empty((1,), dtype=torch.float32, device=x.device)
    grad = torch.empty((B, C, T), dtype=torch.float32, device=x.device) if want_grad else None
    elem = torch.empty((B, Tn), dtype=torch.float32, device=x.device) if want_elem else None
    ws = torch.empty(max(L.itts_mol_loss_workspace_bytes(B, T), 8), dtype=torch.uint8, device=x.device)
    _lib.check(L.itts_mol_loss(_ptr(x), _ptr(y), _ptr(row_weight), B, C // 3, T, shift, int(num_classes),
                               float(log_scale_min), int(bool(hinge)), _ptr(loss), _ptr(elem), _ptr(grad), _ptr(ws),
                               _stream()), "itts_mol_loss")
    return loss, grad, elem


def _signal_offsets(offsets, total, name):
    offsets = [int(o) for o in offsets]
    if len(offsets) < 1 or offsets[0] != 0 or offsets[-1] != total:
        raise ValueError("offsets must run from 0 to the {} values of {}, got {} .. {}".format(
            total, name, offsets[0] if offsets else None, offsets[-1] if offsets else None))
    return offsets


def mulaw_encode(x, offsets, mu=255):
    """RawWaveformLabelGen.mu_law_companding of every float64 signal x[offsets[s]:offsets[s + 1]]: int64 indices in
    [0, mu], truncated toward zero (itts_mulaw_encode_f64)."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    x = x.reshape(-1).contiguous()
    offsets = _signal_offsets(offsets, x.numel(), "x")
    out = torch.empty(x.shape, dtype=torch.int64, device=x.device)
    _lib.check(L.itts_mulaw_encode_f64(_ptr(x), _lib.offsets_array(offsets), len(offsets) - 1, int(mu), _ptr(out),
                                       _stream()), "itts_mulaw_encode_f64")
    return out


def mulaw_decode(index, offsets, mu=255):
    """RawWaveformLabelGen.mu_law_companding_reversed of int64 indices: float64 (itts_mulaw_decode)."""
    L = _lib.load()
    _need(index, torch.int64, "index")
    index = index.reshape(-1).contiguous()
    offsets = _signal_offsets(offsets, index.numel(), "index")
    out = torch.empty(index.shape, dtype=torch.float64, device=index.device)
    _lib.check(L.itts_mulaw_decode(_ptr(index), _lib.offsets_array(offsets), len(offsets) - 1, int(mu), _ptr(out),
                                   _stream()), "itts_mulaw_decode")
    return out


def mulaw_onehot(x, begins, lengths, mu=255, out=None):
    """The [n, mu + 1] float32 one-hot targets of every float64 signal x[begins[s]:begins[s] + lengths[s]], back to
    back, from one launch (itts_mulaw_onehot).  Returns (onehot [sum(lengths), mu + 1], row offsets)."""
    L = _lib.load()
    _need(x, torch.float64, "x")
    x = x.reshape(-1).contiguous()
    begins, lengths = [int(b) for b in begins], [int(n) for n in lengths]
    if len(begins) != len(lengths):
        raise ValueError("{} begins for {} lengths".format(len(begins), len(lengths)))
    out_off = [0]
    for s, (b, n) in enumerate(zip(begins, lengths)):
        if b < 0 or n < 0 or b + n > x.numel():
            raise ValueError("signal {} = x[{}:{}] lies outside the {} samples of x".format(s, b, b + n, x.numel()))
        out_off.append(out_off[-1] + n)
    if not 1 <= int(mu) <= MULAW_MAX_MU:
        raise ValueError("mu = {} is outside 1 .. {}".format(mu, MULAW_MAX_MU))
    if out is None:
        out = torch.empty((out_off[-1], int(mu) + 1), dtype=torch.float32, device=x.device)
    _need(out, torch.float32, "out")
    if tuple(out.shape) != (out_off[-1], int(mu) + 1) or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 [{}, {}]".format(out_off[-1], int(mu) + 1))
    if begins:
        _lib.check(L.itts_mulaw_onehot(_ptr(x), _lib.offsets_array(begins), _lib.offsets_array(out_off), len(begins),
                                       int(mu), _ptr(out), _stream()), "itts_mulaw_onehot")
    return out, out_off


def sample_linearly(x, offsets, m, dtype=torch.float32):
    """misc.utils.sample_linearly of every signal x[offsets[s]:offsets[s + 1]] (rows of D float32 / float64 values):
    [T, D] becomes [m T, D] at linspace(0, T - 1, m T), interpolated in float64 and stored as `dtype`
    (itts_sample_linearly).  Returns (y [m * rows, D], output offsets)."""
    L = _lib.load()
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError("x must be float32 or float64, got {}".format(x.dtype))
    if dtype not in (torch.float32, torch.float64):
        raise TypeError("dtype must be float32 or float64, got {}".format(dtype))
    _need(x, x.dtype, "x")
    if x.dim() != 2:
        raise ValueError("x must be [rows, D], got {}".format(tuple(x.shape)))
    x = x.contiguous()
    offsets = _signal_offsets(offsets, x.shape[0], "x")
    m = int(m)
    y = torch.empty((x.shape[0] * m, x.shape[1]), dtype=dtype, device=x.device)
    _lib.check(L.itts_sample_linearly(_ptr(x), int(x.dtype == torch.float64), _lib.offsets_array(offsets),
                                      len(offsets) - 1, x.shape[1], m, _ptr(y), int(dtype == torch.float64),
                                      _stream()), "itts_sample_linearly")
    return y, [o * m for o in offsets]


VOCODER_WINDOW_FIELDS = 5


def vocoder_windows(x, feat, windows, W, m, mu=255, target=None, cond=None):
    """A training batch of the vocoder from the resident corpus, one launch (itts_vocoder_windows): `x` float64 [n]
    samples and `feat` float32 [rows, cin] conditioning frames, the utterances back to back (`feat` None: no
    conditioning); `windows` host int64 [B, 5] = (first sample in x, len, first frame row of the utterance, its T
    frames, place a of the first sample in the utterance).  Returns (target [B, mu + 1, W] one-hot, or [B, 1, W]
    samples with mu None / 0; cond [B, cin, W] or None): columns past a window's len are zeros, every element is
    written.  `target` / `cond`: contiguous float32 buffers of those shapes to write into."""
    import numpy as np
    L = _lib.load()
    mu = 0 if mu is None else int(mu)
    W, m = int(W), int(m)
    win = np.ascontiguousarray(np.asarray(windows, dtype=np.int64).reshape(-1, VOCODER_WINDOW_FIELDS))
    B = win.shape[0]
    _need(x, torch.float64, "x")
    x = x.reshape(-1).contiguous()
    cin = 0
    if feat is not None:
        _need(feat, torch.float32, "feat")
        if feat.dim() != 2:
            raise ValueError("feat must be [rows, cin], got {}".format(tuple(feat.shape)))
        feat = feat.contiguous()
        cin = feat.shape[1]
    outs = []
    for buf, name, shape in ((target, "target", (B, mu + 1, max(W, 0))), (cond, "cond", (B, cin, max(W, 0)))):
        if name == "cond" and cin == 0:
            outs.append(None)
            continue
        if buf is None:
            buf = torch.empty(shape, dtype=torch.float32, device=x.device)
        _need(buf, torch.float32, name)
        if tuple(buf.shape) != shape or not buf.is_contiguous():
            raise ValueError("{} must be a contiguous float32 {}".format(name, list(shape)))
        outs.append(buf)
    target, cond = outs
    _lib.check(L.itts_vocoder_windows(_ptr(x), x.numel(), _ptr(feat) if cin else None,
                                      feat.shape[0] if cin else 0, cin, m, mu,
                                      (ctypes.c_int64 * win.size).from_buffer(win) if win.size else None, B, W,
                                      _ptr(target), _ptr(cond), _stream()), "itts_vocoder_windows")
    return target, cond


# ---------------------------------------------------------------------------------------- WaveNet
def _gate_rows(t, name, width=None):
    _need(t, torch.float32, name)
    if t.dim() != 2:
        raise ValueError("{} must be 2-D [N, {}]".format(name, "G" if width is None else width))
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def glu_gate(x, c=None, out=None):
    """z [N, G / 2] = tanh(a + ca) * sigmoid(b + cb) of x [N, G] = a | b and the optional c [N, G] = ca | cb
    (itts_glu_gate_fwd): the gate of a WaveNet residual layer.  Rows of any pitch; float4 loads where the pitches
    allow."""
    L = _lib.load()
    x, ldx = _gate_rows(x, "x")
    N, G = x.shape
    if G < 2 or G % 2:
        raise ValueError("G = {} is not a positive even number".format(G))
    ldc = 0
    if c is not None:
        c, ldc = _gate_rows(c, "c")
        if tuple(c.shape) != (N, G):
            raise ValueError("c must be [N, G] = [{}, {}], got {}".format(N, G, tuple(c.shape)))
    if out is None:
        out = torch.empty((N, G // 2), dtype=torch.float32, device=x.device)
    _need(out, torch.float32, "out")
    if tuple(out.shape) != (N, G // 2) or (G > 2 and out.stride(1) != 1):
        raise ValueError("out must be float32 [{}, {}] with contiguous rows".format(N, G // 2))
    ldz = out.stride(0) if N > 1 else max(out.stride(0), G // 2)
    _lib.check(L.itts_glu_gate_fwd(_ptr(x), ldx, _ptr(c), ldc, _ptr(out), ldz, N, G, _stream()), "itts_glu_gate_fwd")
    return out


def glu_gate_bwd(dz, x, c=None):
    """dx [N, G] of glu_gate from dz [N, G / 2], recomputed from x and c (itts_glu_gate_bwd); it is the gradient of c
    as well."""
    L = _lib.load()
    x, ldx = _gate_rows(x, "x")
    N, G = x.shape
    dz, lddz = _gate_rows(dz, "dz")
    if tuple(dz.shape) != (N, G // 2):
        raise ValueError("dz must be [N, G / 2] = [{}, {}], got {}".format(N, G // 2, tuple(dz.shape)))
    ldc = 0
    if c is not None:
        c, ldc = _gate_rows(c, "c")
        if tuple(c.shape) != (N, G):
            raise ValueError("c must be [N, G] = [{}, {}], got {}".format(N, G, tuple(c.shape)))
    dx = torch.empty((N, G), dtype=torch.float32, device=x.device)
    _lib.check(L.itts_glu_gate_bwd(_ptr(dz), lddz, _ptr(x), ldx, _ptr(c), ldc, _ptr(dx), G, N, G, _stream()),
               "itts_glu_gate_bwd")
    return dx


# the envelope of itts_wavenet_generate (csrc/wavenet.hip)
WAVENET_TILE_ROWS = 16
WAVENET_MAX_WIDTH, WAVENET_MAX_CIN, WAVENET_MAX_CLASSES, WAVENET_MAX_MIXTURES = 512, 128, 256, 64
WAVENET_MAX_LAYERS, WAVENET_MAX_DILATION = 64, 512


def wavenet_check_envelope(layers, dilations, kernel_size, residual_channels, gate_channels, skip_out_channels,
                           cin_channels, out_channels, scalar_input):
    """NotImplementedError naming the first argument outside what the generation kernel covers"""
    def refuse(name, value, what):
        raise NotImplementedError("WaveNet {}={}: the generation kernel covers {}".format(name, value, what))
    if kernel_size not in (2, 3):
        refuse("kernel_size", kernel_size, "2 and 3")
    if not 1 <= layers <= WAVENET_MAX_LAYERS:
        refuse("layers", layers, "1 .. {}".format(WAVENET_MAX_LAYERS))
    if max(dilations) > WAVENET_MAX_DILATION:
        refuse("layers / stacks", "{} (dilation {})".format(layers, max(dilations)),
               "dilations up to {}".format(WAVENET_MAX_DILATION))
    for name, value in (("residual_channels", residual_channels), ("skip_out_channels", skip_out_channels)):
        if value < 16 or value % 16 or value > WAVENET_MAX_WIDTH:
            refuse(name, value, "multiples of 16 up to {}".format(WAVENET_MAX_WIDTH))
    if gate_channels < 32 or gate_channels % 32 or gate_channels > WAVENET_MAX_WIDTH:
        refuse("gate_channels", gate_channels, "multiples of 32 up to {}".format(WAVENET_MAX_WIDTH))
    if not 0 <= cin_channels <= WAVENET_MAX_CIN:
        refuse("cin_channels", cin_channels, "0 .. {}".format(WAVENET_MAX_CIN))
    if scalar_input:
        if out_channels < 3 or out_channels % 3 or out_channels // 3 > WAVENET_MAX_MIXTURES:
            refuse("out_channels", out_channels, "3 K with K up to {} for scalar input".format(WAVENET_MAX_MIXTURES))
    elif not 2 <= out_channels <= WAVENET_MAX_CLASSES:
        refuse("out_channels", out_channels, "2 .. {} classes".format(WAVENET_MAX_CLASSES))


def _c_ints(values):
    values = [int(v) for v in values]
    return (ctypes.c_int * len(values))(*values)


def wavenet_state_floats(B, dilations, kernel_size, residual_channels):
    """floats of the ring-buffer scratch of wavenet_generate for B rows (itts_wavenet_state_floats)"""
    n = _lib.load().itts_wavenet_state_floats(int(B), len(dilations), int(kernel_size), int(residual_channels),
                                              _c_ints(dilations))
    if n < 0:
        _lib.check(-1, "itts_wavenet_state_floats")
    return n


def wavenet_pack(w, rows=None, cols=None):
    """The MFMA weight image of an operand w [K, N] (zero filled to `rows` x `cols`, multiples of 16):
    image[kb][tile][lane][j] = w[16 kb + 4 (lane >> 4) + j][16 tile + (lane & 15)], flat.  Data movement only."""
    K, N = w.shape
    rows = (K + 15) // 16 * 16 if rows is None else rows
    cols = (N + 15) // 16 * 16 if cols is None else cols
    full = torch.zeros((rows, cols), dtype=torch.float32, device=w.device)
    full[:K, :N] = w
    # [kb, kg, j, tile, col] -> [kb, tile, kg, col, j]
    return full.view(rows // 16, 4, 4, cols // 16, 16).permute(0, 3, 1, 4, 2).contiguous().reshape(-1)


WaveNetWeights = collections.namedtuple(
    "WaveNetWeights", "wf bf w1 b1 w2 b2 wh1 bh1 wh2 bh2 dilations kernel_size residual_channels gate_channels "
    "skip_out_channels cin_channels out_channels scalar_input log_scale_min")


def wavenet_generate(weights, c, lengths, uniforms, initial_class=-1, return_logits=False, state=None):
    """Sample-by-sample generation of a batch in one launch (itts_wavenet_generate).  weights: a WaveNetWeights of
    packed effective weights (nn.WaveNet.generation_weights()); c [B, Tc, cin] float32 conditioning at the sample rate
    (None with cin 0); lengths: B ints; uniforms [B, T] (classes) or [B, T, 2] (scalar input), float32 in (0, 1), T >=
    max(lengths).  Returns int32 classes [B, T] or float32 samples [B, T], zeros past each row's length, and with
    return_logits the network outputs [B, T, out_channels] as well."""
    L = _lib.load()
    wt = weights
    lengths = [int(n) for n in lengths]
    B = len(lengths)
    _need(uniforms, torch.float32, "uniforms")
    want = 3 if wt.scalar_input else 2
    if uniforms.dim() != want or uniforms.shape[0] != B or (wt.scalar_input and uniforms.shape[2] != 2):
        raise ValueError("uniforms must be [B, T{}] with B = {}, got {}".format(", 2" if wt.scalar_input else "", B,
                                                                                tuple(uniforms.shape)))
    uniforms = uniforms.contiguous()
    T = uniforms.shape[1]
    if lengths and (min(lengths) < 0 or max(lengths) > T):
        raise ValueError("lengths must lie in 0 .. T = {}, got {} .. {}".format(T, min(lengths), max(lengths)))
    Tc = 0
    if wt.cin_channels > 0:
        if c is None:
            raise ValueError("cin_channels = {} needs conditioning c".format(wt.cin_channels))
        _need(c, torch.float32, "c")
        if c.dim() != 3 or c.shape[0] != B or c.shape[2] != wt.cin_channels:
            raise ValueError("c must be [B, Tc, cin] = [{}, Tc, {}], got {}".format(B, wt.cin_channels,
                                                                                    tuple(c.shape)))
        c = c.contiguous()
        Tc = c.shape[1]
        if lengths and Tc < max(lengths):
            raise ValueError("c has {} steps, the longest row {}".format(Tc, max(lengths)))
    else:
        c = None
    dev = uniforms.device
    need = wavenet_state_floats(B, wt.dilations, wt.kernel_size, wt.residual_channels)
    if state is None:
        state = torch.empty((max(need, 4),), dtype=torch.float32, device=dev)
    _need(state, torch.float32, "state")
    if state.numel() < need or not state.is_contiguous():
        raise ValueError("state must be a contiguous float32 tensor of {} elements, got {}".format(need,
                                                                                                   state.numel()))
    out = torch.zeros((B, T), dtype=torch.float32 if wt.scalar_input else torch.int32, device=dev)
    logits = torch.zeros((B, T, wt.out_channels), dtype=torch.float32, device=dev) if return_logits else None
    _lib.check(L.itts_wavenet_generate(
        _ptr(wt.wf), _ptr(wt.bf), _ptr(wt.w1), _ptr(wt.b1), _ptr(wt.w2), _ptr(wt.b2), _ptr(wt.wh1), _ptr(wt.bh1),
        _ptr(wt.wh2), _ptr(wt.bh2), _c_ints(wt.dilations), len(wt.dilations), int(wt.kernel_size),
        int(wt.residual_channels), int(wt.gate_channels), int(wt.skip_out_channels), int(wt.cin_channels),
        int(wt.out_channels), int(bool(wt.scalar_input)), float(wt.log_scale_min), _ptr(c), Tc, _ptr(uniforms),
        _c_ints(lengths), B, T, int(initial_class), _ptr(state), state.numel(), _ptr(out), _ptr(logits), _stream()),
        "itts_wavenet_generate")
    return (out, logits) if return_logits else out


FIXED_ATTENTION_MAX_P, FIXED_ATTENTION_MAX_C, FIXED_ATTENTION_MAX_N = 2048, 4096, 64     # csrc/fixed_attention.hip


def fixed_attention_plan(B, T, P, C, n, partial_last=False):
    """What a fixed-attention call of that shape launches (itts_fixed_attention_plan; no device work): a dict with
    K (chunks), fwd_grid, fwd_lds_bytes, bwd_grid (x, y) and vec_p / vec_c -- whether dense tensors on 16-byte bases
    take 16-byte accesses on the phoneme side (A, Abar) and on the channel side (enc, ctx, d_enc).  ValueError
    outside the envelope (P <= 2048, C <= 4096, n <= 64) or for T % n != 0 without partial_last."""
    L = _lib.load()
    K = ctypes.c_int64(0)
    v = [ctypes.c_int(0) for _ in range(6)]
    if L.itts_fixed_attention_plan(int(B), int(T), int(P), int(C), int(n), 1 if partial_last else 0, ctypes.byref(K),
                                   *[ctypes.byref(i) for i in v]) != 0:
        raise ValueError("no fixed-attention plan for B={}, T={}, P={}, C={}, n_frames_per_step={}, partial_last={}"
                         .format(B, T, P, C, n, bool(partial_last)))
    return {"K": K.value, "fwd_grid": v[0].value, "fwd_lds_bytes": v[1].value, "bwd_grid": (v[2].value, v[3].value),
            "vec_p": bool(v[4].value), "vec_c": bool(v[5].value)}


def _fa_steps(t, name):
    """(row pitch, utterance step) in floats of a [B, R, W] tensor with unit stride on W"""
    if t.dim() != 3 or (t.shape[2] > 1 and t.stride(2) != 1):
        raise ValueError("{} must be 3-D with unit stride on the last extent".format(name))
    B, R, W = t.shape
    ld = t.stride(1) if R > 1 else W
    utt = t.stride(0) if B > 1 else max(R, 1) * ld
    if ld < W or (B > 1 and utt < R * ld):
        raise ValueError("{}: rows or utterances overlap (strides {})".format(name, tuple(t.stride())))
    return ld, utt


def fixed_attention(A, enc, n_frames_per_step=1, partial_last=False, abar=None, ctx=None):
    """A [B, T, P] (the attention matrix of the durations), enc [B, P, C] -> (ctx [B, K, C], Abar [B, K, P]): the chunk
    means of A over n_frames_per_step frames and their product with enc, walking each row's non-zeros
    (FixedAttention.forward_batched of the reference).  K = T / n; with `partial_last` K = ceil(T / n) and the last
    chunk is the mean over the rows it has."""
    L = _lib.load()
    _need(A, torch.float32, "A")
    _need(enc, torch.float32, "enc")
    if A.requires_grad:
        raise ValueError("fixed_attention: A.requires_grad is set, but the attention matrix is a ground-truth input "
                         "and has no gradient")
    ldA, uttA = _fa_steps(A, "A")
    ldE, uttE = _fa_steps(enc, "enc")
    B, T, P = A.shape
    n = int(n_frames_per_step)
    if enc.shape[0] != B or enc.shape[1] != P:
        raise ValueError("enc must be [B, P, C] = [{}, {}, C], got {}".format(B, P, tuple(enc.shape)))
    C = enc.shape[2]
    if not 1 <= n <= FIXED_ATTENTION_MAX_N:
        raise ValueError("n_frames_per_step = {} is outside 1 .. {}".format(n, FIXED_ATTENTION_MAX_N))
    if not partial_last and T % n != 0:
        raise ValueError("T = {} is not a multiple of n_frames_per_step = {} and partial_last is not set".format(T, n))
    K = -(-T // n) if partial_last else T // n
    if abar is None:
        abar = torch.empty((B, K, P), dtype=torch.float32, device=A.device)
    if ctx is None:
        ctx = torch.empty((B, K, C), dtype=torch.float32, device=A.device)
    _need(abar, torch.float32, "abar")
    _need(ctx, torch.float32, "ctx")
    if tuple(abar.shape) != (B, K, P) or tuple(ctx.shape) != (B, K, C):
        raise ValueError("abar / ctx must be [{0}, {1}, {2}] / [{0}, {1}, {3}]".format(B, K, P, C))
    ldM, uttM = _fa_steps(abar, "abar")
    ldX, uttX = _fa_steps(ctx, "ctx")
    _lib.check(L.itts_fixed_attention_fwd(_ptr(A), ldA, uttA, _ptr(enc), ldE, uttE, B, T, P, C, n,
                                          1 if partial_last else 0, _ptr(abar), ldM, uttM, _ptr(ctx), ldX, uttX,
                                          _stream()), "itts_fixed_attention_fwd")
    return ctx, abar


def fixed_attention_bwd(abar, dctx, out=None):
    """d_enc [B, P, C] of fixed_attention for Abar [B, K, P] and dctx [B, K, C]; every position is written."""
    L = _lib.load()
    _need(abar, torch.float32, "abar")
    _need(dctx, torch.float32, "dctx")
    B, K, P = abar.shape
    if dctx.dim() != 3 or dctx.shape[0] != B or dctx.shape[1] != K:
        raise ValueError("dctx must be [B, K, C] = [{}, {}, C], got {}".format(B, K, tuple(dctx.shape)))
    C = dctx.shape[2]
    if out is None:
        out = torch.empty((B, P, C), dtype=torch.float32, device=abar.device)
    _need(out, torch.float32, "out")
    if tuple(out.shape) != (B, P, C):
        raise ValueError("out must be [{}, {}, {}]".format(B, P, C))
    ldM, uttM = _fa_steps(abar, "abar")
    ldX, uttX = _fa_steps(dctx, "dctx")
    ldE, uttE = _fa_steps(out, "out")
    _lib.check(L.itts_fixed_attention_bwd(_ptr(abar), ldM, uttM, _ptr(dctx), ldX, uttX, B, K, P, C, _ptr(out), ldE,
                                          uttE, _stream()), "itts_fixed_attention_bwd")
    return out


CELL_LSTM, CELL_GRU, CELL_RNN = 0, 1, 2      # ITTS_CELL_* in include/idiaptts_amd.h


def rnn_cell_step(kind, gi, gh, h, c=None, b_hh=None, act=ACT_TANH):
    """One time step of an LSTM / GRU / RNN layer direction on per-row states (itts_rnn_cell_step): gi [B, G*H] =
    x W_ih^T + b_ih (LSTM, RNN: + b_hh), gh [B, G*H] = h W_hh^T, h / c [B, H] -> (h', c') (c' None unless LSTM)."""
    L = _lib.load()
    for t, name in ((gi, "gi"), (gh, "gh"), (h, "h")):
        _need(t, torch.float32, name)
    B, H = h.shape
    G = {CELL_LSTM: 4, CELL_GRU: 3, CELL_RNN: 1}[kind]
    if tuple(gi.shape) != (B, G * H) or tuple(gh.shape) != (B, G * H):
        raise ValueError("gi / gh must be [{}, {}], got {} / {}".format(B, G * H, tuple(gi.shape), tuple(gh.shape)))
    h_out = torch.empty((B, H), dtype=torch.float32, device=h.device)
    c_out = None
    if kind == CELL_LSTM:
        _need(c, torch.float32, "c")
        if tuple(c.shape) != (B, H):
            raise ValueError("c must be [{}, {}]".format(B, H))
        c_out = torch.empty((B, H), dtype=torch.float32, device=h.device)
    if kind == CELL_GRU:
        _need(b_hh, torch.float32, "b_hh")
        b_hh = b_hh.contiguous()
        if b_hh.numel() != 3 * H:
            raise ValueError("b_hh must hold 3 H = {} values".format(3 * H))
    else:
        b_hh = None
    _lib.check(L.itts_rnn_cell_step(int(kind), int(act), _ptr(gi), _rows(gi, "gi"), _ptr(gh), _rows(gh, "gh"),
                                    _ptr(b_hh), _ptr(h), _rows(h, "h"), _ptr(c), _rows(c, "c") if c is not None else 0,
                                    B, H, _ptr(h_out), H, _ptr(c_out), H, _stream()), "itts_rnn_cell_step")
    return h_out, c_out


# ------------------------------------------------------------------------------- dynamic time warping
DTW_MAX_T, DTW_MAX_D = 4096, 128                # csrc/dtw.hip
# bytes of decisions (one per cell of the padded grids) a single itts_dtw_align call may hold; dtw_align splits the
# batch into groups under it (256 pairs of 1 600 x 1 600 frames are 0.66 GB: one group)
DTW_WORKSPACE_CAP = 1 << 30


def _dtw_check_sizes(T1, T2, D):
    for name, v in (("T1", T1), ("T2", T2)):
        if not 1 <= int(v) <= DTW_MAX_T:
            raise ValueError("dtw: {} = {} is outside 1 .. {}".format(name, int(v), DTW_MAX_T))
    if not 1 <= int(D) <= DTW_MAX_D:
        raise ValueError("dtw: D = {} is outside 1 .. {}".format(int(D), DTW_MAX_D))


def dtw_plan(T1, T2, D):
    """What a DTW of a [T1, D] against a [T2, D] sequence uses (itts_dtw_plan; no device work): the forward kernel's
    tile edges `col_block` and `rows_per_pass`, and `cell_bytes_x8`, 8 x the bytes of decisions stored per cell."""
    _dtw_check_sizes(T1, T2, D)
    W, R, c8 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if _lib.load().itts_dtw_plan(int(T1), int(T2), int(D), ctypes.byref(W), ctypes.byref(R), ctypes.byref(c8)) != 0:
        raise ValueError("dtw_plan: ({}, {}, {}) is outside the envelope".format(T1, T2, D))
    return {"col_block": W.value, "rows_per_pass": R.value, "cell_bytes_x8": c8.value}


def dtw_step_probe(mode, steps):
    """Queues `steps` empty steps of a dependency chain in one workgroup (itts_dtw_step_probe; mode "barrier": 256
    threads, one workgroup barrier a step; "shift": one wave, one lane shift a step) and returns the 256 doubles it
    leaves; the caller times it (scripts/bench_dtw.py)."""
    out = torch.empty(256, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().itts_dtw_step_probe({"barrier": 0, "shift": 1}[mode], int(steps), _ptr(out), _stream()),
               "itts_dtw_step_probe")
    return out


def _dtw_side(t, lens, name):
    """(tensors or padded tensor, lengths, D) of one side of dtw_align, sizes checked (ValueError) on the host."""
    if isinstance(t, (list, tuple)):
        if len(t) < 1:
            raise ValueError("dtw_align: {} holds B = 0 sequences".format(name))
        for u in t:
            if u.dim() != 2:
                raise ValueError("dtw_align: every sequence of {} must be [T, D], got {}".format(name, tuple(u.shape)))
        D = int(t[0].shape[1])
        for b, u in enumerate(t):
            if int(u.shape[1]) != D:
                raise ValueError("dtw_align: {}[{}] has D = {}, {}[0] has D = {}".format(name, b, int(u.shape[1]), name, D))
        given = [int(u.shape[0]) for u in t]
        if lens is not None and [int(v) for v in lens] != given:
            raise ValueError("dtw_align: {}_lens = {} do not match the sequences' lengths {}".format(
                name, [int(v) for v in lens], given))
        return list(t), given, D
    if t.dim() != 3:
        raise ValueError("dtw_align: {} must be [B, T, D] or a list of [T, D], got {}".format(name, tuple(t.shape)))
    if lens is None:
        raise ValueError("dtw_align: {}_lens is needed with a padded {}".format(name, name))
    lens = [int(v) for v in (lens.tolist() if hasattr(lens, "tolist") else lens)]
    if int(t.shape[0]) < 1 or len(lens) != int(t.shape[0]):
        raise ValueError("dtw_align: {} holds B = {} sequences, {}_lens {}".format(name, int(t.shape[0]), name, len(lens)))
    for b, v in enumerate(lens):
        if v > int(t.shape[1]):
            raise ValueError("dtw_align: {}_lens[{}] = {} is longer than the buffer's {} frames".format(
                name, b, v, int(t.shape[1])))
    return t, lens, int(t.shape[2])


def _dtw_groups(t1, t2, cap):
    """Consecutive pairs whose padded decision grids fit `cap` bytes together (a pair on its own always goes)."""
    groups, g0, m1, m2 = [], 0, 0, 0
    for b in range(len(t1)):
        n1, n2 = max(m1, t1[b]), max(m2, t2[b])
        if b > g0 and (b - g0 + 1) * n1 * n2 > cap:
            groups.append((g0, b))
            g0, n1, n2 = b, t1[b], t2[b]
        m1, m2 = n1, n2
    groups.append((g0, len(t1)))
    return groups


def dtw_align(x, x_lens, y, y_lens, band=None, return_path=True):
    """Dynamic time warping of B pairs (itts_dtw_align): x / y padded [B, T, D] tensors with their lengths, or lists of
    [T, D] tensors (lengths None); float32 or float64 (anything else, or a mixed pair, is widened to float64).  Local
    distance: the Euclidean norm; steps (1,1), (1,0), (0,1), ties in that order; all arithmetic float64.  band = r
    admits |j - round(i (T2-1)/(T1-1))| <= r only (None: no band).
    -> cost float64 [B], length int32 [B], path int32 [B, Lmax, 2] (rows behind length[b] are -1; None without
    return_path).  A pair whose band does not connect its corners has cost inf and length 0.  The batch is cut into
    groups of at most DTW_WORKSPACE_CAP bytes of decisions; a pair's result does not depend on the grouping."""
    x, t1, D = _dtw_side(x, x_lens, "x")
    y, t2, Dy = _dtw_side(y, y_lens, "y")
    if D != Dy:
        raise ValueError("dtw_align: x has D = {}, y has D = {}".format(D, Dy))
    if len(t1) != len(t2):
        raise ValueError("dtw_align: x holds B = {} sequences, y {}".format(len(t1), len(t2)))
    for b in range(len(t1)):
        _dtw_check_sizes(t1[b], t2[b], D)
    if band is not None and int(band) < 0:
        raise ValueError("dtw_align: band = {} is negative (None: no band)".format(band))
    band = -1 if band is None else min(int(band), 2 * DTW_MAX_T)
    B = len(t1)
    first = x[0] if isinstance(x, list) else x
    firsty = y[0] if isinstance(y, list) else y
    dtype = first.dtype if first.dtype == firsty.dtype and first.dtype in (torch.float32, torch.float64) \
        else torch.float64

    def padded(t, name):
        if isinstance(t, list):
            for u in t:
                if not u.is_cuda:
                    raise _lib.IttsError("{} must live on the GPU (no CPU fallback)".format(name))
            t = torch.nn.utils.rnn.pad_sequence([u.to(dtype) for u in t], batch_first=True)
        elif not t.is_cuda:
            raise _lib.IttsError("{} must live on the GPU (no CPU fallback)".format(name))
        t = t.to(dtype)
        return t if t.stride(2) == 1 else t.contiguous()

    x, y = padded(x, "x"), padded(y, "y")
    L = _lib.load()
    dev = x.device
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    length = torch.empty(B, dtype=torch.int32, device=dev)
    paths = []
    for g0, g1 in _dtw_groups(t1, t2, DTW_WORKSPACE_CAP):
        n, m1, m2 = g1 - g0, max(t1[g0:g1]), max(t2[g0:g1])
        nbytes = L.itts_dtw_workspace_bytes(n, m1, m2)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rows = m1 + m2 - 1
        path = torch.empty((n, rows, 2), dtype=torch.int32, device=dev) if return_path else None
        h1 = (ctypes.c_int32 * n)(*t1[g0:g1])
        h2 = (ctypes.c_int32 * n)(*t2[g0:g1])
        xg, yg = x[g0:g1], y[g0:g1]
        _lib.check(L.itts_dtw_align(_ptr(xg), x.stride(1), x.stride(0), _ptr(yg), y.stride(1), y.stride(0),
                                    1 if dtype == torch.float64 else 0, h1, h2, n, m1, m2, D, band, _ptr(cost[g0:g1]),
                                    _ptr(length[g0:g1]), _ptr(path), rows, _ptr(work), nbytes, _stream()),
                   "itts_dtw_align")
        paths.append(path)
    if not return_path:
        return cost, length, None
    lmax = max(int(length.max().item()), 1)
    out = torch.full((B, lmax, 2), -1, dtype=torch.int32, device=dev)
    for (g0, g1), path in zip(_dtw_groups(t1, t2, DTW_WORKSPACE_CAP), paths):
        keep = min(lmax, path.shape[1])
        out[g0:g1, :keep] = path[:, :keep]
    return cost, length, out
