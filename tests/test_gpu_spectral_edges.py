"""The four spectral kernels at their edges (tests/spectral_cases.py; tests/test_spectral_cases.py proves on the CPU
which branch every case reaches): stft_wave_kernel and mel_project_kernel of csrc/stft.hip, griffinlim_kernel and
mel_inverse_kernel, against the float64 restatements stft_spec, griffinlim_spec and mel_inverse_spec with the bounds
tests/test_gpu_stft.py, test_gpu_griffinlim.py and test_gpu_mel_inverse.py hold these kernels to.  No frame, bin,
band or draw is exempt, and no case relaxes a bound (RELAXED is empty).

Every case prints its measured error ("[spectral_edges] ..."; err/bound is the largest elementwise error in units of
its bound).  Worst figures measured on an MI355X (110 tests, 11 s):
  STFT amp_sp        3.5e-7 of the bound   (1024, one sample, reflect)
  STFT amp_sp_f64    1.8e-6 of the bound   (1024, hop 1, 40 samples)
  STFT mfbanks       2.6e-6 of the bound   (1024, three samples, reflect); mel_project: the reference's bits
  STFT log_amp_sp    1.5e-5 dB of 1e-4     (sweep draw 12)
  Griffin-Lim f64    1.6e-11 of 1e-9       (1024, hop 64, T = 2)
  Griffin-Lim f32    3.2e-8 of 1e-6        (one live frame, 1024)
  mel inversion f64  8.5e-13 of 1e-9       (48 kHz, 256 bands); NNLS gap 1.2e-12 of 1e-9 (129 bands)
  mel inversion f32  5.5e-8 of 2e-6        (16 kHz, one band)
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import griffinlim_spec as gl
import mel_inverse_spec as mi
import spectral_cases as sc
import stft_spec as spec
from idiaptts_amd import lib, ops, world
from test_gpu_mel_inverse import TOL_F32, TOL_F64, _gaps
from test_gpu_stft import _close

pytestmark = pytest.mark.gpu

DB_TOL = 1e-4               # log_amp_sp, absolute dB
GL_TOL_F64 = 1e-9           # Griffin-Lim, relative to the largest sample
GL_TOL_F32 = 1e-6           # float32 state at one iteration
NNLS_GAP = 1e-9
NAN_FRAME = 64
# case name -> relaxed bound; a case may only enter with four times the error of the float64 restatement re-run
# with float32 or reversed sums on the same input, recorded beside it.  None was needed.
RELAXED = {}


def _say(*parts):
    print("[spectral_edges]", *parts)


def _bound(case, default):
    return RELAXED.get(case, default)


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    scale = np.abs(ref).max()
    return np.abs(got - ref).max() / scale if scale > 0 else np.abs(got).max()


# ================================================================================================ STFT
@functools.lru_cache(maxsize=None)
def _basis64(fs, n_fft, n_mels):
    return spec.mel_basis(fs, n_fft, n_mels).astype(np.float64)


def _expected(amp, kind, fs, n_fft, n_mels):
    """what the reference's librosa calls give for the float64 amplitude rows `amp` of the restatement"""
    if kind == "amp_sp":
        return amp.astype(np.float32)
    if kind == "amp_sp_f64":
        return amp
    if kind == "log_amp_sp":
        return 20 * np.log10(np.maximum(np.float32(1e-5), amp.astype(np.float32)))
    return (_basis64(fs, n_fft, n_mels) @ amp.T).T.astype(np.float32)


def _check(case, kind, got, amp, fs, n_fft, n_mels=80):
    ref = _expected(amp, kind, fs, n_fft, n_mels)
    assert got.dtype == (np.float64 if kind == "amp_sp_f64" else np.float32), (case, kind)
    assert got.shape == ref.shape, (case, kind, got.shape, ref.shape)
    assert np.isfinite(got).all(), (case, kind)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    if kind == "log_amp_sp":
        _say(case, kind, "max dB error", err.max())
        assert err.max() <= _bound(case, DB_TOL), (case, kind, err.max())
        return
    bound = 1e-6 * np.abs(ref).astype(np.float64) + 1e-10 * np.abs(ref).max()
    ratio = np.where(err > 0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny), 0.0)
    _say(case, kind, "err/bound", ratio.max())
    try:
        _close(got, ref, _bound(case, 1e-6))
    except AssertionError as e:
        raise AssertionError("{} {}: {}".format(case, kind, e))


def _amp_rows(raws, first, rows, n_fft, hop, win_length=None, center=True, pad_mode="reflect"):
    """the restatement's rows first[u] .. first[u] + rows[u] of every utterance, stacked"""
    parts = [spec.amp_sp(r, n_fft, hop, win_length, center, pad_mode)[a:a + k] if k else np.zeros((0, n_fft // 2 + 1))
             for r, a, k in zip(raws, first, rows)]
    assert all(len(p) == k for p, k in zip(parts, rows))
    return np.concatenate(parts)


def _features(raws, kind, n_fft, hop, first=None, rows=None, n_mels=80, win_length=None, center=True,
              pad_mode="reflect", out=None):
    first = [0] * len(raws) if first is None else first
    rows = [sc.stft_frames(len(r), n_fft, hop, center) for r in raws] if rows is None else rows
    x = torch.from_numpy(np.concatenate(raws)).cuda()
    got = world.stft_features(x, world.offsets([len(r) for r in raws]), world.offsets(rows), first, sc.FS_OF[n_fft],
                              kind, n_fft, hop, n_mels=n_mels, win_length=win_length, center=center,
                              pad_mode=pad_mode, out=out)
    return got


def _all_kinds(case, raws, n_fft, hop, first=None, rows=None, n_mels=80, **kw):
    first = [0] * len(raws) if first is None else first
    rows = [sc.stft_frames(len(r), n_fft, hop, kw.get("center", True)) for r in raws] if rows is None else rows
    amp = _amp_rows(raws, first, rows, n_fft, hop, kw.get("win_length"), kw.get("center", True),
                    kw.get("pad_mode", "reflect"))
    out = {}
    for kind in sc.KINDS:
        got = _features(raws, kind, n_fft, hop, first, rows, n_mels, **kw).cpu().numpy()
        _check(case, kind, got, amp, sc.FS_OF[n_fft], n_fft, n_mels)
        out[kind] = got
    return out


@pytest.mark.parametrize("n_fft,hop", sc.STFT_POINTS)
def test_stft_lengths(gpu, n_fft, hop):
    for n in sc.STFT_LENGTHS[n_fft]:
        raw = sc.signal(n, n)
        for center, pad_mode in sc.stft_modes(n_fft, n):
            case = "length n_fft={} n={} center={} pad={}".format(n_fft, n, center, pad_mode)
            got = _all_kinds(case, [raw], n_fft, hop, center=center, pad_mode=pad_mode)
            assert len(got["amp_sp"]) == (1 + n // hop if center else 1 + (n - n_fft) // hop)


@pytest.mark.parametrize("n_fft,hop", sc.STFT_POINTS)
def test_stft_window_lengths(gpu, n_fft, hop):
    raws = [sc.signal(3 * n_fft + 5, 7), sc.signal(n_fft // 3, 9)]
    for win_length in sc.WIN_LENGTHS[n_fft]:
        _all_kinds("win_length n_fft={} win={}".format(n_fft, win_length), raws, n_fft, hop, win_length=win_length)
    _all_kinds("win_length n_fft={} win={} center=False".format(n_fft, sc.WIN_LENGTHS[n_fft][0]), raws[:1], n_fft,
               hop, win_length=sc.WIN_LENGTHS[n_fft][0], center=False)


@pytest.mark.parametrize("hop,n", sc.HOP_CASES)
def test_stft_hops(gpu, hop, n):
    raw = sc.signal(n, hop)
    for center, pad_mode in sc.stft_modes(1024, n):
        _all_kinds("hop={} n={} center={} pad={}".format(hop, n, center, pad_mode), [raw], 1024, hop, center=center,
                   pad_mode=pad_mode)


@pytest.mark.parametrize("n_fft,hop,center", [(1024, 80, True), (2048, 240, True), (2048, 240, False)])
def test_stft_first_frames_of_a_ragged_batch(gpu, n_fft, hop, center):
    raws, first, keep = sc.first_batch(n_fft, hop, center)
    case = "first n_fft={} center={}".format(n_fft, center)
    cut = _all_kinds(case, raws, n_fft, hop, first, keep, center=center)
    # and the rows are the bits of the untrimmed run
    full_rows = [sc.stft_frames(len(r), n_fft, hop, center) for r in raws]
    f_off, c_off = world.offsets(full_rows), world.offsets(keep)
    for kind in sc.KINDS:
        full = _features(raws, kind, n_fft, hop, center=center).cpu().numpy()
        for u in range(len(raws)):
            a = f_off[u] + first[u]
            assert np.array_equal(cut[kind][c_off[u]:c_off[u + 1]], full[a:a + keep[u]]), (kind, u)


def test_stft_many_utterances_search_equals_ballot(gpu):
    x, lengths, rows = sc.many_utterances()
    x_off = world.offsets(lengths)
    raws = [x[a:b] for a, b in zip(x_off[:-1], x_off[1:])]
    got = _all_kinds("1030 utterances", raws, 1024, 80, rows=rows)
    n_x, n_rows = x_off[sc.N_PREFIX], sum(rows[:sc.N_PREFIX])
    assert 0 < n_rows < sum(rows)
    for kind in sc.KINDS:
        prefix = _features(raws[:sc.N_PREFIX], kind, 1024, 80, rows=rows[:sc.N_PREFIX]).cpu().numpy()
        assert len(np.concatenate(raws[:sc.N_PREFIX])) == n_x
        assert prefix.tobytes() == got[kind][:n_rows].tobytes(), kind


@pytest.mark.parametrize("fs,n_fft", sorted(sc.MEL_BANDS))
def test_mel_band_counts(gpu, fs, n_fft):
    hop = dict(sc.STFT_POINTS)[n_fft]
    raw = sc.signal(3 * n_fft, 11)
    amp = spec.amp_sp(raw, n_fft, hop)
    amp_dev = torch.from_numpy(amp).cuda()
    for n_mels in sc.MEL_BANDS[(fs, n_fft)]:
        case = "bands fs={} n_mels={}".format(fs, n_mels)
        empty = ~spec.mel_basis(fs, n_fft, n_mels).any(axis=1)
        assert (empty.sum() > 0) == (n_mels == 513)
        x = torch.from_numpy(raw).cuda()
        fused = world.stft_features(x, [0, len(raw)], [0, len(amp)], [0], fs, "mfbanks", n_fft, hop,
                                    n_mels=n_mels).cpu().numpy()
        projected = world.mel_project(amp_dev, fs, n_fft, n_mels).cpu().numpy()
        for name, got in (("stft_mel", fused), ("mel_project", projected)):
            _check(case + " " + name, "mfbanks", got, amp, fs, n_fft, n_mels)
            assert not got[:, empty].any(), (case, name)
            assert (got[:, ~empty] > 0).all(), (case, name)


@pytest.mark.parametrize("T", sc.MEL_PROJECT_ROWS)
def test_mel_project_row_counts(gpu, T):
    amp = np.random.default_rng(T).random((T, 513)) ** 2
    got = world.mel_project(torch.from_numpy(amp).cuda(), 16000, 1024, 80).cpu().numpy()
    _check("mel_project T={}".format(T), "mfbanks", got, amp, 16000, 1024, 80)


def _framed(rows, width, dtype):
    """a [rows, width] view of pitch width + 3 inside a buffer with NaN frames of 64 elements on both sides"""
    ld = width + 3
    buf = torch.full((2 * NAN_FRAME + rows * ld,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[NAN_FRAME:NAN_FRAME + rows * ld].view(rows, ld)[:, :width]


def _untouched(buf, rows, width):
    ld = width + 3
    inner = buf[NAN_FRAME:NAN_FRAME + rows * ld].view(rows, ld)
    return bool(torch.isnan(buf[:NAN_FRAME]).all() and torch.isnan(buf[NAN_FRAME + rows * ld:]).all()
                and torch.isnan(inner[:, width:]).all() and torch.isfinite(inner[:, :width]).all())


@pytest.mark.parametrize("n_fft,hop", sc.STFT_POINTS)
def test_pitched_outputs_inside_nan_frames(gpu, n_fft, hop):
    raws = [sc.signal(n_fft + 3 * hop, 31), sc.signal(n_fft // 2 - 1, 32), sc.signal(2 * n_fft, 33)]
    rows = sum(sc.stft_frames(len(r), n_fft, hop) for r in raws)
    for kind in sc.KINDS:
        width = 80 if kind == "mfbanks" else n_fft // 2 + 1
        buf, view = _framed(rows, width, torch.float64 if kind == "amp_sp_f64" else torch.float32)
        assert view.stride(0) == width + 3
        _features(raws, kind, n_fft, hop, out=view)
        plain = _features(raws, kind, n_fft, hop)
        torch.cuda.synchronize()
        assert _untouched(buf, rows, width), kind
        assert view.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes(), kind
    # mel_project
    fs = sc.FS_OF[n_fft]
    amp = torch.from_numpy(spec.amp_sp(raws[0], n_fft, hop)).cuda()
    tab, w = (torch.from_numpy(np.array(a)).cuda() for a in world.mel_tables(fs, n_fft, 80))
    buf, view = _framed(len(amp), 80, torch.float32)
    ops.mel_project(amp, tab, w, 80, out=view)
    plain = world.mel_project(amp, fs, n_fft, 80)
    torch.cuda.synchronize()
    assert _untouched(buf, len(amp), 80)
    assert view.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()


@pytest.mark.parametrize("n_fft,hop", sc.STFT_POINTS)
def test_zero_input(gpu, n_fft, hop):
    raws = [sc.signal(n_fft, 41), np.zeros(2 * n_fft + 17), sc.signal(300, 42)]
    rows = [sc.stft_frames(len(r), n_fft, hop) for r in raws]
    a, b = rows[0], rows[0] + rows[1]
    for pad_mode in sc.PAD_MODES:
        got = _all_kinds("zero utterance n_fft={} pad={}".format(n_fft, pad_mode), raws, n_fft, hop, pad_mode=pad_mode)
        assert not got["amp_sp"][a:b].any() and not got["amp_sp_f64"][a:b].any() and not got["mfbanks"][a:b].any()
        assert (got["log_amp_sp"][a:b] == np.float32(-100.0)).all()
        assert got["amp_sp"][:a].any() and got["amp_sp"][b:].any()
    alone = _all_kinds("zero utterance alone n_fft={}".format(n_fft), raws[1:2], n_fft, hop)
    assert not alone["amp_sp"].any() and not alone["mfbanks"].any() and (alone["log_amp_sp"] == -100.0).all()


@pytest.mark.parametrize("i", range(24))
def test_stft_random_sweep(gpu, i):
    d = sc.sweep_draws()[i]
    raws = sc.sweep_signals(d)
    kw = dict(win_length=d["win_length"], center=d["center"], pad_mode=d["pad_mode"])
    try:
        amp = _amp_rows(raws, d["first"], d["rows"], d["n_fft"], d["hop"], **kw)
        got = _features(raws, d["kind"], d["n_fft"], d["hop"], d["first"], d["rows"], d["n_mels"], **kw).cpu().numpy()
        _check("sweep draw {}".format(i), d["kind"], got, amp, sc.FS_OF[d["n_fft"]], d["n_fft"], d["n_mels"])
    except AssertionError as e:
        raise AssertionError("draw {} {}: {}".format(i, d, e))


# ================================================================================================ Griffin-Lim
def test_restated_tile_formula_is_the_library_s(gpu):
    L = lib.load()
    for n_fft, hop, _ in sc.GL_CASES:
        assert L.itts_griffinlim_tile_frames(n_fft, hop) == sc.gl_tile_frames(n_fft, hop), (n_fft, hop)
    for n_fft in (1024, 2048):
        for hop in (1, 2, 3, 5, 7, 33, 80, 110, 240, 300, 511, n_fft // 2):
            assert L.itts_griffinlim_tile_frames(n_fft, hop) == sc.gl_tile_frames(n_fft, hop), (n_fft, hop)


def _gl_batch(spectra, hop, win_length, seed, n_fft, **kw):
    hop_arg = None if hop == (win_length or n_fft) // 4 else hop          # the default hop where it is the case's
    return world.griffinlim_batch(spectra, hop_length=hop_arg, win_length=win_length,
                                  random_state=np.random.RandomState(seed), **kw)


def _gl_params():
    out = []
    for n_fft, hop, win_length in sc.GL_CASES:
        for pad_mode in (sc.PAD_MODES if (n_fft, hop) in sc.GL_BOTH_PADS else sc.PAD_MODES[:1]):
            for dtype in ((np.float64, np.float32) if (n_fft, hop) in sc.GL_BOTH_DTYPES and win_length is None
                          else (np.float64,)):
                out.append((n_fft, hop, win_length, pad_mode, dtype))
    return out


@pytest.mark.parametrize("n_fft,hop,win_length,pad_mode,dtype", _gl_params())
def test_griffinlim_tiles(gpu, n_fft, hop, win_length, pad_mode, dtype):
    F = lib.load().itts_griffinlim_tile_frames(n_fft, hop)
    assert F == sc.gl_tile_frames(n_fft, hop)
    counts = (2, 3, F, F + 1, 2 * F + 1)
    f32 = dtype == np.float32
    n_iter, tol = (1, GL_TOL_F32) if f32 else (sc.GL_ITERS, GL_TOL_F64)
    spectra = sc.gl_spectra(n_fft, counts, seed=hop, dtype=dtype)
    kw = dict(n_iter=n_iter, pad_mode=pad_mode, n_fft=n_fft)
    batch = _gl_batch(spectra, hop, win_length, 3, **kw)
    rs = np.random.RandomState(3)
    single = [world.griffinlim_batch([sp], n_iter=n_iter, hop_length=hop, win_length=win_length, pad_mode=pad_mode,
                                     random_state=rs)[0] for sp in spectra]
    phases = world.griffinlim_init_phases([sp.shape for sp in spectra], "random", np.random.RandomState(3))
    case = "gl n_fft={} hop={} win={} pad={} {}".format(n_fft, hop, win_length, pad_mode, np.dtype(dtype).name)
    for t, sp, a0, y, s in zip(counts, spectra, phases, batch, single):
        assert y.dtype == dtype and len(y) == hop * (t - 1) and np.isfinite(y).all()
        assert np.array_equal(y, s), (case, t)
        ref = gl.griffinlim(sp, a0, n_iter, hop, win_length, pad_mode, c64=f32)
        r = _rel(y, ref)
        _say(case, "T={} tiles={}".format(t, len(sc.gl_tiles(t, F))), "rel", r)
        assert r <= _bound(case, tol), (case, t, r)


@pytest.mark.parametrize("variant", ["n_iter=0", "init=None", "momentum=0"])
def test_griffinlim_arguments(gpu, variant):
    n_fft, hop = 1024, 256
    F = lib.load().itts_griffinlim_tile_frames(n_fft, hop)
    (S,) = sc.gl_spectra(n_fft, (F + 1,), seed=77)
    kw = {"n_iter=0": dict(n_iter=0), "init=None": dict(n_iter=sc.GL_ITERS, init=None),
          "momentum=0": dict(n_iter=sc.GL_ITERS, momentum=0.0)}[variant]
    y = world.griffinlim(S.T, hop_length=hop, random_state=9, **kw)
    a0 = np.ones(S.shape, dtype=np.complex128) if "init" in kw else gl.init_phases(S.shape, 9)
    ref = gl.griffinlim(S, a0, kw["n_iter"], hop, momentum=kw.get("momentum", 0.99))
    r = _rel(y, ref)
    _say("gl", variant, "rel", r)
    assert y.dtype == np.float64 and len(y) == hop * F and r <= _bound("gl " + variant, GL_TOL_F64), r


@pytest.mark.parametrize("n_fft,hop", [(1024, 256), (2048, 1024)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_griffinlim_zero_spectra(gpu, n_fft, hop, dtype):
    F = lib.load().itts_griffinlim_tile_frames(n_fft, hop)
    T, K = 2 * F + 1, n_fft // 2 + 1
    zero = np.zeros((T, K), dtype=dtype)
    one = zero.copy()
    one[F] = sc.gl_spectra(n_fft, (1,), seed=5, dtype=dtype)[0][0]            # the first frame of the second tile
    n_iter = 1 if dtype == np.float32 else sc.GL_ITERS
    y0, y1 = world.griffinlim_batch([zero, one], n_iter=n_iter, hop_length=hop, random_state=np.random.RandomState(1))
    assert y0.dtype == dtype and len(y0) == hop * (T - 1) and not y0.any()
    assert np.isfinite(y1).all() and y1.any()
    phases = world.griffinlim_init_phases([zero.shape, one.shape], "random", np.random.RandomState(1))
    r = _rel(y1, gl.griffinlim(one, phases[1], n_iter, hop, c64=dtype == np.float32))
    _say("gl one live frame n_fft={} {}".format(n_fft, np.dtype(dtype).name), "rel", r)
    assert r <= _bound("gl one live frame", GL_TOL_F32 if dtype == np.float32 else GL_TOL_F64), r


@pytest.mark.parametrize("f64", [True, False])
def test_griffinlim_buffers_inside_nan_frames(gpu, f64):
    """the waveform and the three state buffers framed by NaN on both sides, through the C entry point"""
    L = lib.load()
    n_fft, hop, K = 1024, 512, 513
    F = L.itts_griffinlim_tile_frames(n_fft, hop)
    counts = (2, F + 1, 2 * F + 1)
    real = torch.float64 if f64 else torch.float32
    spectra = sc.gl_spectra(n_fft, counts, seed=12, dtype=np.float64 if f64 else np.float32)
    phases = world.griffinlim_init_phases([sp.shape for sp in spectra], "random", np.random.RandomState(4),
                                          np.complex128 if f64 else np.complex64)
    f_off = world.offsets(counts)
    rows, n_y = f_off[-1], hop * (f_off[-1] - len(counts))
    S = torch.from_numpy(np.concatenate(spectra)).cuda()
    angles = torch.from_numpy(np.ascontiguousarray(np.concatenate(phases))).cuda()
    (win,) = (torch.from_numpy(np.array(world.stft_window(n_fft))).cuda(),)

    def framed(n):
        buf = torch.full((n + 2 * NAN_FRAME,), float("nan"), dtype=real, device="cuda")
        return buf, buf[NAN_FRAME:NAN_FRAME + n]

    def intact(buf, n):
        return bool(torch.isnan(buf[:NAN_FRAME]).all() and torch.isnan(buf[NAN_FRAME + n:]).all()
                    and torch.isfinite(buf[NAN_FRAME:NAN_FRAME + n]).all())

    n_c = 2 * rows * K
    (ba, a), (bb, b), (bt, t), (by, y) = framed(n_c), framed(n_c), framed(n_c), framed(n_y)
    a.copy_(torch.view_as_real(angles).reshape(-1))
    ptr = lambda v: ctypes.c_void_p(v.data_ptr())          # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(L.itts_griffinlim(ptr(S), ptr(a), ptr(b), ptr(t), lib.offsets_array(f_off), len(counts), n_fft, hop, 1,
                                ptr(win), 2, 0.99, int(f64), ptr(y), stream), "itts_griffinlim")
    torch.cuda.synchronize()
    assert intact(ba, n_c) and intact(bb, n_c) and intact(bt, n_c) and intact(by, n_y)
    plain = ops.griffinlim(S, angles.clone(), f_off, n_fft, hop, "reflect", win, 2, 0.99)
    assert torch.equal(plain, y)


# ================================================================================================ mel inversion
def _mi_run(B, fs, n_fft, **kw):
    out, iters = world.mel_inverse(torch.from_numpy(np.ascontiguousarray(B)).cuda(), fs, n_fft, return_iters=True,
                                   **kw)
    return out.cpu().numpy(), iters.cpu().numpy()


def _mi_params():
    return [(fs, n_fft, m, dtype) for (fs, n_fft), bands in sorted(sc.MI_BANDS.items()) for m in bands
            for dtype in (np.float32, np.float64)]


@pytest.mark.parametrize("fs,n_fft,n_mels,dtype", _mi_params())
def test_mel_inverse_band_counts(gpu, fs, n_fft, n_mels, dtype):
    B = sc.mel_bands(fs, n_fft, n_mels).astype(dtype)
    K = n_fft // 2 + 1
    out, iters = _mi_run(B, fs, n_fft)
    assert out.dtype == dtype and out.shape == (len(B), K) and np.isfinite(out).all() and (out >= 0).all()
    assert iters.min() >= mi.CHECK and iters.max() <= mi.CAP and np.all(iters % mi.CHECK == 0)
    A = mi.basis(fs, n_fft, n_mels, dtype)
    X, _ = mi.solve(A, B, iters=iters)
    r = _rel(out, X * K)
    case = "mel_inverse fs={} n_mels={} {}".format(fs, n_mels, np.dtype(dtype).name)
    _say(case, "slot", sc.lane_slot(n_mels), "iters", iters.min(), iters.max(), "rel", r)
    assert r <= _bound(case, TOL_F64 if dtype == np.float64 else TOL_F32), (case, r)
    if dtype == np.float64 and (fs, n_fft) == (16000, 1024) and n_mels in sc.MI_NNLS_BANDS:
        g = _gaps(A, B, out / K)
        _say(case, "NNLS gap", g.max())
        assert g.max() <= NNLS_GAP, (case, g.max())


@pytest.mark.parametrize("F", sc.MI_FRAME_COUNTS)
def test_mel_inverse_frame_counts(gpu, F):
    B = sc.mel_bands(16000, 1024, 65)[10:10 + F].astype(np.float64)
    out, iters = _mi_run(B, 16000, 1024)
    X, _ = mi.solve(mi.basis(16000, 1024, 65, np.float64), B, iters=iters)
    r = _rel(out, X * 513)
    _say("mel_inverse F={}".format(F), "rel", r)
    assert out.shape == (F, 513) and iters.shape == (F,) and r <= TOL_F64, r
    whole, _ = _mi_run(sc.mel_bands(16000, 1024, 65).astype(np.float64), 16000, 1024)
    assert out.tobytes() == whole[10:10 + F].tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mel_inverse_iteration_caps(gpu, dtype):
    B = sc.mel_bands(16000, 1024, 129).astype(dtype)
    A = mi.basis(16000, 1024, 129, dtype)
    tol = TOL_F64 if dtype == np.float64 else TOL_F32
    out, iters = _mi_run(B, 16000, 1024, max_iter=0)           # the start alone
    r = _rel(out, mi.start(A, B) * 513)
    _say("mel_inverse max_iter=0", np.dtype(dtype).name, "rel", r)
    assert not iters.any() and r <= tol, r
    assert world.MEL_INVERSE_CHECK == 16
    out, iters = _mi_run(B, 16000, 1024, max_iter=7)           # a cap below the first stopping test
    X, _ = mi.solve(A, B, iters=np.full(len(B), 7))
    r = _rel(out, X * 513)
    _say("mel_inverse max_iter=7", np.dtype(dtype).name, "rel", r)
    assert (iters == 7).all() and r <= tol, r


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_mels", [65, 256])
def test_mel_inverse_zero_and_negative_bands(gpu, n_mels, dtype):
    B = sc.mel_bands(16000, 1024, n_mels).astype(dtype)
    out, iters = _mi_run(np.zeros_like(B), 16000, 1024)
    assert not out.any() and (iters == world.MEL_INVERSE_CHECK).all()
    live = B.max(axis=1) > 0
    mixed = np.where((np.arange(len(B)) % 2 == 0)[:, None], -B, B)       # negative frames between live ones
    out, iters = _mi_run(mixed, 16000, 1024)
    assert not out[0::2].any(), np.abs(out[0::2]).max()
    assert out[1::2][live[1::2]].any(axis=1).all()
    both, _ = _mi_run(B, 16000, 1024)
    assert out[1::2].tobytes() == both[1::2].tobytes()
    out, _ = _mi_run(-B, 16000, 1024)
    assert not out.any(), np.abs(out).max()


def _mi_entry(mel, n_mels, fs, n_fft, out, iters, table_dtype):
    """itts_mel_inverse itself: mel and out are row views of any pitch and either precision"""
    L = lib.load()
    tabs = world.mel_inverse_tables(fs, n_fft, n_mels, table_dtype)
    bin_j, bin_w, filt, pinv_t = (torch.from_numpy(np.array(a, order="C")).cuda() for a in tabs[:4])
    ptr = lambda v: ctypes.c_void_p(v.data_ptr())          # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(L.itts_mel_inverse(ptr(mel), mel.shape[0], n_mels, mel.stride(0), int(mel.dtype == torch.float64), n_fft,
                                 ptr(bin_j), ptr(bin_w), ptr(filt), ptr(pinv_t), tabs[4], world.MEL_INVERSE_TOL,
                                 world.MEL_INVERSE_CAP, world.MEL_INVERSE_CHECK, ptr(out), out.stride(0),
                                 int(out.dtype == torch.float64), ptr(iters), stream), "itts_mel_inverse")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mel_inverse_pitched_rows_inside_nan_frames(gpu, dtype):
    """ld_mel = n_mels + 3 (through ops.mel_inverse and the entry point), ld_out = K + 5 (the entry point: ops
    allocates its own output), NaN between the rows and in frames of 64 elements around both buffers"""
    n_mels, K, F = 129, 513, 9
    B = sc.mel_bands(16000, 1024, n_mels)[20:20 + F].astype(dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    plain, plain_iters = _mi_run(B, 16000, 1024)
    ld_mel, ld_out = n_mels + 3, K + 5
    mbuf = torch.full((2 * NAN_FRAME + F * ld_mel,), float("nan"), dtype=tdt, device="cuda")
    mel = mbuf[NAN_FRAME:NAN_FRAME + F * ld_mel].view(F, ld_mel)[:, :n_mels]
    mel.copy_(torch.from_numpy(B))
    tabs = world.mel_inverse_tables(16000, 1024, n_mels, dtype)
    dev_tabs = [torch.from_numpy(np.array(a, order="C")).cuda() for a in tabs[:4]]
    via_ops = ops.mel_inverse(mel, 1024, *dev_tabs, tabs[4], world.MEL_INVERSE_TOL, world.MEL_INVERSE_CAP,
                              world.MEL_INVERSE_CHECK, tdt)
    assert via_ops.cpu().numpy().tobytes() == plain.tobytes()
    obuf = torch.full((2 * NAN_FRAME + F * ld_out,), float("nan"), dtype=tdt, device="cuda")
    out = obuf[NAN_FRAME:NAN_FRAME + F * ld_out].view(F, ld_out)[:, :K]
    iters = torch.full((F + 2,), -1, dtype=torch.int32, device="cuda")
    _mi_entry(mel, n_mels, 16000, 1024, out, iters[1:F + 1], dtype)
    inner = obuf[NAN_FRAME:NAN_FRAME + F * ld_out].view(F, ld_out)
    assert torch.isnan(obuf[:NAN_FRAME]).all() and torch.isnan(obuf[NAN_FRAME + F * ld_out:]).all()
    assert torch.isnan(inner[:, K:]).all() and torch.isfinite(inner[:, :K]).all()
    assert out.cpu().numpy().tobytes() == plain.tobytes()
    assert iters.cpu().tolist() == [-1] + plain_iters.tolist() + [-1]
    # the bands were only read
    assert torch.isnan(mbuf[:NAN_FRAME]).all() and torch.isnan(mbuf[NAN_FRAME + F * ld_mel:]).all()
    assert torch.isnan(mbuf[NAN_FRAME:-NAN_FRAME].view(F, ld_mel)[:, n_mels:]).all()
    assert np.array_equal(mel.cpu().numpy(), B)


@pytest.mark.parametrize("in_dtype,out_dtype", [(np.float32, np.float64), (np.float64, np.float32)])
def test_mel_inverse_mixed_precisions(gpu, in_dtype, out_dtype):
    """in_f64 and out_f64 are independent: the iteration is that of the input's basis, only the last rounding differs"""
    n_mels, K = 65, 513
    B = np.ascontiguousarray(sc.mel_bands(16000, 1024, n_mels)[::4], dtype=in_dtype)
    same, iters_same = _mi_run(B, 16000, 1024)
    mel = torch.from_numpy(B).cuda()
    out = torch.full((len(B), K), float("nan"), dtype=torch.float64 if out_dtype == np.float64 else torch.float32,
                     device="cuda")
    iters = torch.zeros(len(B), dtype=torch.int32, device="cuda")
    _mi_entry(mel, n_mels, 16000, 1024, out, iters, in_dtype)
    got = out.cpu().numpy()
    assert got.dtype == out_dtype and np.array_equal(iters.cpu().numpy(), iters_same)
    X, _ = mi.solve(mi.basis(16000, 1024, n_mels, in_dtype), B, iters=iters_same)
    r = _rel(got, X * K)
    _say("mel_inverse {} in, {} out".format(np.dtype(in_dtype).name, np.dtype(out_dtype).name), "rel", r)
    assert r <= (TOL_F64 if out_dtype == np.float64 else TOL_F32), r
    if out_dtype == np.float32:
        assert got.tobytes() == same.astype(np.float32).tobytes()        # the float64 result, rounded once
    else:
        assert got.astype(np.float32).tobytes() == same.tobytes()


# ================================================================================================ bounds
def test_only_named_cases_may_relax_a_bound():
    """no case relaxes a bound today; one that must enters RELAXED by its full name, with its figure recorded"""
    assert RELAXED == {}
    assert _bound("sweep draw 3", 1e-6) == 1e-6 and _bound("gl n_iter=0", GL_TOL_F64) == 1e-9
    assert (DB_TOL, GL_TOL_F64, GL_TOL_F32, NNLS_GAP, TOL_F64, TOL_F32) == (1e-4, 1e-9, 1e-6, 1e-9, 1e-9, 2e-6)
