"""The mel-cepstral kernels -- csrc/mcep_lockstep.hip (itts_mcep), itts_mgc2sp (csrc/world_frame.hip) and
csrc/mgcep.hip (itts_mgcep, itts_mgc2sp_gamma) -- away from the few points the rest of the suite holds them at
(K = 513, orders 19 / 24 / 59 / 79, default stopping rule, fftlen 512 / 1024), over tests/cepstral_cases.py, whose
conditions tests/test_cepstral_cases.py proves from the C oracle alone.

What reaches what (mcep_lockstep picks by m1 = order + 1; A = test_mcep_solve_widths):
  mcls_solve_dpp_kernel<20>  A orders 1, 5 (padded), 19 (full)     <24>  A 20 (padded), 23 (full)
  mcls_solve_dpp_kernel<32>  A 24, 31                               <48>  A 32, 40, 47
  mcls_solve_dpp_kernel<60>  A 48, 59                               <64>  A 60, 61, 63
  mcls_solve_kernel (LDS)    A 64, 79, 127
  mcls_fused3_kernel<4>      A orders <= 31      <8>  A 32 .. 63      unfused launches: A 64, 79, 127 and every
                             order <= 63 once more under ITTS_MCEP_FUSED=0, bit for bit.  The sweep's envelopes lie
                             outside the model class: frames leave the compacted work list round by round
  transform sizes 64 .. 2048 test_mcep_sizes (K 33 .. 1025), test_mgcep_sizes (mgcep_kernel's NQ x 256 threads over
                             f2 + 1 bins, 2 x 64 lanes over 2 m + 1 <= 127 outputs at order 63)
  gemm_f64_lds_kernel        test_long_batches: mcep order 79 and (unfused) order 59 at T = 1100, mgc2sp order 79
  gemm_f64_staged_kernel     test_long_batches: mgc2sp order 64 (m1 = 65: no vector loads) at T = 1100
  host loop                  test_stopping_rules: maxiter 1 (no read-back), the cap reached with frames still on the
                             compacted work list, miniter above maxiter, eps 0 and 1e-3
  mg_gc2gc_rows_kernel       test_mgc2sp_gamma_sizes: T in 1, 2, 3, 5, 37 (the fr >= T exit), fftlen 64 .. 4096
  itts_mgc2sp one-GEMM path  test_mgc2sp_sizes: fftlen 64 / 512 / 2048, orders 0, 18 (scalar loads), 19, 63 (vector)
  itts_mgc2sp fallback       test_mgc2sp_sizes: order 64 from fftlen 512 up, every order at 4096 / 8192 (131 KB of LDS)

Bounds are those of the existing tests: Newton trip counts equal to the oracle's and |mc - ref| < 1e-8
(test_fused_newton_products_on_ragged_frame_counts), mgcep within 1e-8 max(1, |ref|) (test_mgcep_matches_oracle),
decoding within 1e-9 max(1, |ref|) for gamma != 0, 1e-10 for gamma = 0, rtol 2e-6 for float32.  Against the closed
form the bound is the same plus the 1e-12 the CPU file holds the oracle to.  Every figure is printed before it is
asserted (pytest -s).

Measured wall time of this file on an MI355X: 28 s for its 186 tests, most of it the oracle on the host (up to 2 s
for the 37 frames of an mgcep case at K = 1025); no test takes more than 0.3 s of GPU work, and the warping tables
(one alpha per transform size) are built in the first call of a size."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import cepstral_cases as cc

pytestmark = pytest.mark.gpu

GUARD_ROWS = 8
SENTINEL = 7.25


def _say(*parts):
    print("[cepstral]", *parts)


@contextlib.contextmanager
def _fused(mode):
    """tests/test_gpu_world.py's save / restore of ITTS_MCEP_FUSED (read by every itts_mcep call)."""
    old = os.environ.get("ITTS_MCEP_FUSED")
    try:
        if mode is None:
            os.environ.pop("ITTS_MCEP_FUSED", None)
        else:
            os.environ["ITTS_MCEP_FUSED"] = mode
        yield
    finally:
        if old is None:
            os.environ.pop("ITTS_MCEP_FUSED", None)
        else:
            os.environ["ITTS_MCEP_FUSED"] = old


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _analyse(gpu, kind, a, order, alpha, gamma=None, f32_pitch=None, input_is_power=False, eps=1e-8, miniter=2,
             maxiter=30, threshold=1e-3):
    """itts_mcep / itts_mgcep through the C ABI into the head of sentinel-filled buffers: GUARD_ROWS rows of
    coefficients and trip counts behind the output, and the pad columns of an f32 output of pitch f32_pitch, must come
    back untouched.  Returns (coefficients [T, order + 1] f64 numpy, trip counts)."""
    from idiaptts_amd import lib as _lib, ops
    L = _lib.load()
    x = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    T, K = x.shape
    m1 = order + 1
    pitch = f32_pitch or m1
    out = torch.full((T + GUARD_ROWS, pitch), SENTINEL, dtype=torch.float32 if f32_pitch else torch.float64, device=gpu)
    iters = torch.full((T + GUARD_ROWS,), -7, dtype=torch.int32, device=gpu)
    o32, o64 = (out, None) if f32_pitch else (None, out)
    if kind == "mcep":
        assert not input_is_power
        _lib.check(L.itts_mcep(_p(x), T, K, order, float(alpha), eps, miniter, maxiter, threshold, _p(o32), pitch,
                               _p(o64), _p(iters), ops._stream()), "itts_mcep")
    else:
        _lib.check(L.itts_mgcep(_p(x), 1 if input_is_power else 0, T, K, order, float(alpha), float(gamma), eps,
                                miniter, maxiter, threshold, _p(o32), pitch, _p(o64), _p(iters), ops._stream()),
                   "itts_mgcep")
    out, iters = out.cpu().numpy(), iters.cpu().numpy()
    assert (out[T:] == SENTINEL).all() and (iters[T:] == -7).all(), "rows behind the output were written"
    assert (out[:T, m1:] == SENTINEL).all(), "pad columns were written"
    return out[:T, :m1].astype(np.float64), iters[:T]


def _check_analysis(got, it, ref, it_ref, scale_by_ref, tag):
    bound = 1e-8 * (max(1.0, float(np.abs(ref).max())) if scale_by_ref else 1.0)
    diff = float(np.abs(got - ref).max())
    _say(tag, "frames", len(ref), "trip counts", int(it_ref.min()), "..", int(it_ref.max()), "equal",
         bool(np.array_equal(it, it_ref)), "max |c - ref|", diff, "bound", bound)
    assert got.shape == ref.shape, tag
    assert np.array_equal(it, it_ref), tag
    assert diff < bound, tag


def _run_counted(gpu, case, fused=None, frames=None):
    a = cc.amp_of(case)[:frames]
    with _fused(fused):
        return _analyse(gpu, case.kind, a, case.order, case.alpha, case.gamma, **cc.rule_of(case))


def _mcep_case(gpu, case):
    """Assertions of A and B: the oracle's trip counts and values; below order 64 the unfused launches bit for bit."""
    ref, it_ref = cc.oracle_analysis(case.name)
    got, it = _run_counted(gpu, case)
    _check_analysis(got, it, ref, it_ref, False, case.name)
    if case.order <= 63:
        got0, it0 = _run_counted(gpu, case, fused="0")
        assert np.array_equal(it0, it) and np.array_equal(got0, got), case.name + ": fused != unfused"


# ------------------------------------------------------------------------------------------ A, B, C: mcep
@pytest.mark.parametrize("name", [c.name for c in cc.WIDTH_CASES])
def test_mcep_solve_widths(gpu, name):
    _mcep_case(gpu, cc.BY_NAME[name])


@pytest.mark.parametrize("K", sorted(cc.SIZE_ORDERS))
def test_mcep_sizes(gpu, K):
    for case in cc.SIZE_CASES:
        if case.K == K:
            _mcep_case(gpu, case)


def test_long_batches_reach_the_long_k_gemms(gpu):
    """T = 1100 >= 1024 rows and K > 64: launch_gemm_f64 leaves gemm_f64_kernel for gemm_f64_lds_kernel (16-byte
    aligned rows, K % 4 == 0 or slack behind the rows) or gemm_f64_staged_kernel.  mcep without the fused
    kernels (order 79; order 59 under ITTS_MCEP_FUSED=0) sends its init, spectrum and autocorrelation products there;
    ops.mgc2sp's fallback sends its de-warping product: order 79 (m1 = 80) on the LDS kernel, order 64 (m1 = 65, odd
    pitch) on the staged kernel.  The fused order-59 run must give the same bits as the unfused one."""
    for case, fused in zip(cc.LONG_CASES, (None, "0")):
        ref, it_ref = cc.oracle_analysis(case.name)
        got, it = _run_counted(gpu, case, fused=fused)
        _check_analysis(got, it, ref, it_ref, False, case.name)
        if fused == "0":
            got1, it1 = _run_counted(gpu, case)
            assert np.array_equal(it1, it) and np.array_equal(got1, got)
    for order in cc.LONG_DECODE_ORDERS:
        c = cc.tiled(cc.decode_coefficients(order, 0.58, 0.0), cc.T_LONG)
        ref = cc.tiled(cc.oracle_decode(order, 0.58, 0.0, 1024), cc.T_LONG)
        _check_decode(gpu, c, 0.58, 0.0, 1024, ref, "long mgc2sp order %d" % order)


# ------------------------------------------------------------------------------------------ D: stopping rules
@pytest.mark.parametrize("name", [c.name for c in cc.RULE_CASES])
def test_stopping_rules(gpu, name):
    from idiaptts_amd import ops
    case = cc.BY_NAME[name]
    ref, it_ref = cc.oracle_analysis(name)
    x = torch.from_numpy(cc.amp_of(case)).to(gpu)
    rule = cc.rule_of(case)
    if case.kind == "mcep":
        got, it = ops.mcep(x, case.order, case.alpha, dtype=torch.float64, want_iters=True, **rule)
    else:
        got, it = ops.mgcep(x, case.order, case.alpha, case.gamma, dtype=torch.float64, want_iters=True, **rule)
    if dict(case.rule).get("threshold") == 1e-12:
        assert (it_ref == rule["maxiter"]).any() and (it_ref < rule["maxiter"]).any()
    _check_analysis(got.cpu().numpy(), it.cpu().numpy(), ref, it_ref, case.kind == "mgcep", name)


# ------------------------------------------------------------------------------------------ E: degenerate frames
@pytest.mark.parametrize("kind", ["mcep", "mgcep"])
def test_degenerate_frames_inside_a_batch(gpu, kind):
    """An all-zero row (an STFT of silence), a flat 1e-6 row and a flat 1.0 row between envelopes: every row equals
    the oracle ON THAT ROW ALONE, so neither the degenerate rows nor their neighbours see each other.  Values only: the
    trip counts are printed, not asserted (these rows are not in the CPU file's stopping-margin check)."""
    from oracle import capi
    d = cc.DEGENERATE
    a = cc.degenerate_amp()
    gamma = d["gamma"] if kind == "mgcep" else None
    got, it = _analyse(gpu, kind, a, d["order"], d["alpha"], gamma)
    assert np.isfinite(got).all()
    for r in range(len(a)):
        row = a[r:r + 1]
        if kind == "mcep":
            ref, it_ref = capi.mcep(row, d["order"], d["alpha"], return_iters=True)
        else:
            ref, it_ref = capi.mgcep(row, d["order"], d["alpha"], gamma, return_iters=True)
        diff = float(np.abs(got[r] - ref[0]).max())
        bound = 1e-8 * max(1.0, float(np.abs(ref).max()))
        _say("degenerate", kind, "row", r, "flat" if r in cc.DEGENERATE_ROWS else "envelope", "trip counts", int(it[r]),
             int(it_ref[0]), "max |c - ref|", diff, "bound", bound)
        assert diff < bound, (kind, r)


# ------------------------------------------------------------------------------------------ F: output forms
@pytest.mark.parametrize("kind", ["mcep", "mgcep"])
def test_f32_output_with_a_wider_pitch(gpu, kind):
    """An f32 output of pitch order + 1 + 3 in a sentinel-filled buffer: the values are the f64 result rounded once,
    the pad columns and the rows behind stay untouched (_analyse asserts both)."""
    d = cc.DEGENERATE
    a = cc.amp(d["K"], cc.T, seed=2)
    gamma = d["gamma"] if kind == "mgcep" else None
    got64, it64 = _analyse(gpu, kind, a, d["order"], d["alpha"], gamma)
    got32, it32 = _analyse(gpu, kind, a, d["order"], d["alpha"], gamma, f32_pitch=d["order"] + 1 + 3)
    assert np.array_equal(it32, it64)
    assert np.array_equal(got32.astype(np.float32), got64.astype(np.float32))


def test_power_input_with_f64_output(gpu):
    """input_is_power = 1 with an f64 output against the amplitude call fed the amplitudes whose squares were passed:
    the kernel squares an amplitude exactly as the host does, so the periodograms are the same numbers."""
    d = cc.DEGENERATE
    amp = cc.amp(d["K"], cc.T, seed=2)
    for gamma in (d["gamma"], 0.0, -1.0):
        from_amp, it_a = _analyse(gpu, "mgcep", amp, d["order"], d["alpha"], gamma)
        from_pow, it_p = _analyse(gpu, "mgcep", amp * amp, d["order"], d["alpha"], gamma, input_is_power=True)
        rel = float((np.abs(from_pow - from_amp) / np.maximum(1e-300, np.abs(from_amp))).max())
        _say("power input gamma", gamma, "max relative difference", rel)
        assert np.array_equal(it_a, it_p)
        assert rel < 1e-12


# ------------------------------------------------------------------------------------------ G: mgcep sizes
@pytest.mark.parametrize("name", [c.name for c in cc.MGCEP_CASES])
def test_mgcep_sizes(gpu, name):
    from idiaptts_amd import ops
    case = cc.BY_NAME[name]
    ref, it_ref = cc.oracle_analysis(name)
    for n in cc.MGCEP_FRAMES:
        x = torch.from_numpy(cc.amp_of(case)[:n]).to(gpu)
        got, it = ops.mgcep(x, case.order, case.alpha, case.gamma, dtype=torch.float64, want_iters=True)
        _check_analysis(got.cpu().numpy(), it.cpu().numpy(), ref[:n], it_ref[:n], True, "%s T=%d" % (name, n))


# ------------------------------------------------------------------------------------------ H: decode sizes
def _check_decode(gpu, c, alpha, gamma, fftlen, ref, tag, entry=None):
    """All three outputs of ops.mgc2sp (gamma == 0) / ops.mgc2sp_gamma against the log amplitude `ref`."""
    from idiaptts_amd import ops
    x = torch.from_numpy(np.ascontiguousarray(c)).to(gpu)
    if entry is None:
        entry = "mgc2sp" if gamma == 0.0 else "mgc2sp_gamma"
    if entry == "mgc2sp":
        run = lambda **kw: ops.mgc2sp(x, alpha, fftlen, **kw).cpu().numpy()                      # noqa: E731
    else:
        run = lambda **kw: ops.mgc2sp_gamma(x, alpha, gamma, fftlen, **kw).cpu().numpy()         # noqa: E731
    bound = 1e-10 if gamma == 0.0 else 1e-9 * max(1.0, float(np.abs(ref).max()))
    la = run(want_logamp=True)
    diff = float(np.abs(la - ref).max())
    a32 = run()
    want32 = np.exp(ref.astype(np.float32))
    rel32 = float(np.abs(a32 / want32 - 1.0).max())
    pw = run(want_pow=True)
    _say(tag, "frames", len(ref), "max |log amp - ref|", diff, "bound", bound, "f32 max rel", rel32)
    assert la.shape == ref.shape and la.dtype == np.float64 and a32.dtype == np.float32 and pw.dtype == np.float64, tag
    assert diff < bound, tag
    assert np.allclose(a32, want32, rtol=2e-6, atol=0.0), tag
    assert np.array_equal(pw, a32.astype(np.float64) ** 2), tag          # the power is the f32 amplitude squared
    return la


@pytest.mark.parametrize("gamma", cc.DECODE_GAMMAS, ids=cc.gamma_tag)
@pytest.mark.parametrize("fftlen", cc.DECODE_GAMMA_FFT)
def test_mgc2sp_gamma_sizes(gpu, fftlen, gamma):
    alpha = cc.DECODE_ALPHA[fftlen]
    for order in cc.DECODE_GAMMA_ORDERS:
        if order > fftlen // 2:
            continue
        c = cc.decode_coefficients(order, alpha, gamma)
        ref = cc.oracle_decode(order, alpha, gamma, fftlen)
        for n in cc.DECODE_FRAMES if order == 19 else (cc.T,):
            _check_decode(gpu, c[:n], alpha, gamma, fftlen, ref[:n], "mgc2sp_gamma fft %d order %d %s T=%d" % (
                fftlen, order, cc.gamma_tag(gamma), n))


@pytest.mark.parametrize("fftlen", cc.DECODE_FFT)
def test_mgc2sp_sizes(gpu, fftlen):
    alpha = cc.DECODE_ALPHA[fftlen]
    for order in cc.DECODE_ORDERS:
        if order > fftlen // 2:
            continue
        c = cc.decode_coefficients(order, alpha, 0.0)
        ref = cc.oracle_decode(order, alpha, 0.0, fftlen)
        _check_decode(gpu, c, alpha, 0.0, fftlen, ref, "mgc2sp fft %d order %d" % (fftlen, order))


# ------------------------------------------------------------------------------------------ I: the closed-form pin
@pytest.mark.parametrize("p", cc.PIN_DECODE,
                         ids=lambda p: "g%.2f_a%.2f_o%d_fft%d" % (-p.gamma, p.alpha, p.order, p.fftlen))
def test_decoding_equals_the_closed_form(gpu, p):
    """The kernels against log|D| written out, not against the oracle: the GPU-vs-oracle bound plus the 1e-12 the
    oracle itself is held to (tests/test_cepstral_cases.py)."""
    from idiaptts_amd import ops
    c = cc.pin_coefficients(p.order)
    ref = cc.pin_decode_reference(p)
    x = torch.from_numpy(c).to(gpu)
    if p.gamma == 0.0:
        la = ops.mgc2sp(x, p.alpha, p.fftlen, want_logamp=True).cpu().numpy()
        bound = 1e-10 + cc.ORACLE_PIN
    else:
        la = ops.mgc2sp_gamma(x, p.alpha, p.gamma, p.fftlen, want_logamp=True).cpu().numpy()
        bound = 1e-9 * max(1.0, float(np.abs(ref).max())) + cc.ORACLE_PIN
    diff = float(np.abs(la - ref).max())
    _say("pin decode", p, "max |log amp - closed form|", diff, "bound", bound)
    assert diff < bound


@pytest.mark.parametrize("p", cc.PIN_RECOVER, ids=lambda p: "g%.2f_a%.2f_o%d_K%d" % (-p.gamma, p.alpha, p.order, p.K))
def test_analysis_recovers_the_closed_form(gpu, p):
    """A spectrum inside the model class, eps = 0, threshold 1e-13, at most 80 rounds: the generating coefficients come
    back.  Trip counts are only held below the cap: at 1e-13 the last round sits on the rounding floor."""
    c = cc.pin_coefficients(p.order)
    a = cc.pin_recover_amp(p)
    runs = [("mcep", None)] if p.gamma == 0.0 else []
    runs.append(("mgcep", p.gamma))
    for kind, gamma in runs:
        got, it = _analyse(gpu, kind, a, p.order, p.alpha, gamma, **cc.PIN_RULE)
        scale = 1.0 if kind == "mcep" else max(1.0, float(np.abs(c).max()))
        bound = 1e-8 * scale + cc.ORACLE_PIN * np.maximum(1.0, np.abs(c))
        err = np.abs(got - c)
        _say("pin recover", kind, p, "max |c - generating c|", float(err.max()), "bound", 1e-8 * scale,
             "trip counts", int(it.min()), "..", int(it.max()))
        assert it.max() < cc.PIN_MAXITER, kind
        assert (err < bound).all(), kind
