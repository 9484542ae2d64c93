"""The WORLD kernels (csrc/dio.hip, world_f0ap.hip, world_frame.hip, synth.hip) away from the one point the rest of
the suite holds them at -- 5 ms frames, DIO at 71 / 800 / 2 / 0.1, default q1 / threshold / transform size -- against
the C oracle, frame by frame and sample by sample, over tests/world_param_cases.py (tests/test_world_param_cases.py
shows from the oracle alone that no case is degenerate).  No frame, bin or case is exempt.

Bounds: those tests/test_gpu_world.py holds the 5 ms path to.  Voiced / unvoiced decisions identical; |f0 - ref| < 1e-7
for DIO and StoneMask; the envelope max |log(sp / ref)| < 1e-8 on synthetic audio and, on the fixture audio, the
three-part bound of test_cheaptrick_and_fused_mcep_match_oracle (a bin 1e-7 below its frame's peak carries the
rounding of the smoothing's running sums in the oracle as in the kernels: scripts/ct_error_probe.py); aperiodicity
within 1e-6 dB, LoveTrain's decisions identical; bap and mcep within 1e-6, Newton trip counts equal where the envelope
was computed from the oracle's contour; synthesis max |y - float32(ref)| < 1e-6 and RMSE < 1e-7, lengths equal.

A single-utterance case feeds each stage the oracle's output of the stage before (a stage is compared on its own
inputs); the ragged batch and itts_wav2world chain the device's own outputs, as their callers do.  The synthesis is
always fed the oracle's f0 / sp / ap.  With de-emphasis the kernel's output must be the sequential recurrence on its
own samples exactly, and stay within 1e-5 of the filtered oracle (the bounds of test_synthesis_matches_oracle:
1e-6 per sample through a filter of gain 1 / (1 - 0.97))."""
import ctypes

import numpy as np
import pytest
import torch

import world_param_cases as wc

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in wc.CASES]


def _say(*parts):
    print("[world_params]", *parts)


def _check_f0(got, ref, tag):
    diff = float(np.abs(got - ref).max()) if len(ref) else 0.0
    flips = int(((got == 0) != (ref == 0)).sum())
    _say(tag, "frames", len(ref), "voiced", int((ref > 0).sum()), "vuv flips", flips, "max |f0 - ref|", diff)
    assert len(got) == len(ref), tag
    assert flips == 0, tag
    assert diff < 1e-7, tag


def _check_sp(got, ref, fixture, tag):
    err = np.abs(got - ref)
    rel = err / ref
    peak = ref.max(axis=1, keepdims=True)
    logerr = float(np.abs(np.log(got / ref)).max())
    _say(tag, "sp max |log ratio|", logerr, "max rel", float(rel.max()), "q99.9 rel", float(np.quantile(rel, 0.999)),
         "max err / frame peak", float((err / peak).max()))
    assert got.shape == ref.shape, tag
    if fixture:
        assert rel.max() < 3e-8, tag
        assert np.quantile(rel, 0.999) < 2e-9, tag
        assert (err / peak).max() < 1e-11, tag
    else:
        assert logerr < 1e-8, tag


def _check_ap(got, ref, tag):
    db = float(np.abs(20 * np.log10(got / ref)).max())
    flips = int(((got[:, 0] > 0.999) != (ref[:, 0] > 0.999)).sum())
    _say(tag, "ap max dB", db, "LoveTrain flips", flips, "unvoiced by D4C", int((ref[:, 0] > 0.999).sum()))
    assert got.shape == ref.shape, tag
    assert flips == 0, tag
    assert db < 1e-6, tag


def _check_max(got, ref, bound, what, tag):
    diff = float(np.abs(got - ref).max())
    _say(tag, what, "max abs diff", diff)
    assert got.shape == ref.shape, tag
    assert diff < bound, (tag, what)


def _check_y(got, ref, tag):
    ref32 = ref.astype(np.float32).astype(np.float64)
    assert len(got) == len(ref), tag
    mx = float(np.abs(got - ref32).max())
    rmse = float(np.sqrt(np.mean((got - ref32) ** 2)))
    _say(tag, "samples", len(ref), "y max abs diff", mx, "rmse", rmse, "max |ref|", float(np.abs(ref).max()))
    assert mx < 1e-6, tag
    assert rmse < 1e-7, tag


def _dev(gpu, arrays):
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(arrays))).to(gpu)


def _batch(case, gpu):
    xs = wc.signals(case)
    x_off = wc.offsets([len(x) for x in xs])
    f_off = wc.offsets([wc.num_frames(len(x), case.fs, case.frame_period) for x in xs])
    return xs, _dev(gpu, xs), x_off, f_off


@pytest.mark.parametrize("name", NAMES)
def test_case_matches_oracle(gpu, name):
    from idiaptts_amd import ops
    case = wc.BY_NAME[name]
    ref = wc.oracle_run(name)
    fs, fp, fft = case.fs, case.frame_period, wc.fft_size_of(case)
    xs, x, x_off, f_off = _batch(case, gpu)
    U = len(xs)
    chain = U > 1                      # the ragged batch runs on the device's own contour
    cut = lambda t, u: t[f_off[u]:f_off[u + 1]].cpu().numpy()      # noqa: E731

    f0d = ops.dio(x, x_off, f_off, fs, fp, *case.dio)
    assert f0d.shape == (f_off[-1],)
    for u in range(U):
        _check_f0(cut(f0d, u), ref[u]["f0_dio"], "%s[%d] dio" % (name, u))
    if "stonemask" not in case.stages:
        return
    f0s = ops.stonemask(x, x_off, f0d if chain else _dev(gpu, [r["f0_dio"] for r in ref]), f_off, fs, fp)
    for u in range(U):
        _check_f0(cut(f0s, u), ref[u]["f0"], "%s[%d] stonemask" % (name, u))
    f0 = f0s if chain else _dev(gpu, [r["f0"] for r in ref])

    if "cheaptrick" in case.stages:
        order, alpha = case.mcep or (None, None)
        sp, mc, iters = ops.cheaptrick_mcep(x, x_off, f0, f_off, fs, fp, fft, case.q1, order=order, alpha=alpha,
                                            mc_dtype=torch.float64, want_iters=True)
        for u in range(U):
            tag = "%s[%d] cheaptrick" % (name, u)
            _check_sp(cut(sp, u), ref[u]["sp"], wc.uses_fixture(case, u), tag)
            if case.mcep:
                if not chain:
                    assert np.array_equal(cut(iters, u), ref[u]["iters"]), tag        # same Newton trip counts
                _check_max(cut(mc, u), ref[u]["mc"], 1e-6, "mcep", tag)
    if "d4c" in case.stages:
        ap, bap = ops.d4c(x, x_off, f0, f_off, fs, fp, fft, case.threshold,
                          want_bap=torch.float64 if case.want_bap else None)
        for u in range(U):
            tag = "%s[%d] d4c" % (name, u)
            _check_ap(cut(ap, u), ref[u]["ap"], tag)
            if case.want_bap:
                _check_max(cut(bap, u), ref[u]["bap"], 1e-6, "bap", tag)
    if "synth" in case.stages:
        args = (_dev(gpu, [r["f0"] for r in ref]), _dev(gpu, [r["sp"] for r in ref]),
                _dev(gpu, [r["ap"] for r in ref]), f_off, fs, fp)
        y, y_off = ops.world_synthesize(*args, dtype=torch.float64)
        y = y.cpu().numpy()
        assert y_off == wc.offsets([len(r["y"]) for r in ref])
        assert y_off == wc.offsets([wc.synth_length(f_off[u + 1] - f_off[u], fs, fp) for u in range(U)])
        for u in range(U):
            _check_y(y[y_off[u]:y_off[u + 1]], ref[u]["y"], "%s[%d] synth" % (name, u))
        if case.preemphasis:
            import scipy.signal
            pre = case.preemphasis
            yp, yp_off = ops.world_synthesize(*args, preemphasis=pre, dtype=torch.float64)
            yp = yp.cpu().numpy()
            assert yp_off == y_off
            for u in range(U):
                seg = y[y_off[u]:y_off[u + 1]]
                seq = np.empty(len(seg))
                prev = 0.0
                for i, v in enumerate(seg):
                    prev = v + pre * prev
                    seq[i] = prev
                assert np.array_equal(yp[y_off[u]:y_off[u + 1]], seq)
                filt = scipy.signal.lfilter([1], [1, -pre], ref[u]["y"].astype(np.float32))
                _check_max(yp[y_off[u]:y_off[u + 1]], filt, 1e-5, "de-emphasised y", "%s[%d] synth" % (name, u))


def test_wav2world_at_10_ms_and_an_explicit_fft_size(gpu):
    """itts_wav2world with frame_period 10 and fft_size 2048: the separate entry points bit for bit, and the oracle
    (DIO -> StoneMask -> CheapTrick -> D4C composed) within the bounds of the separate stages."""
    from idiaptts_amd import ops
    case = wc.BY_NAME[wc.WAV2WORLD_CASE]
    ref = wc.oracle_run(case.name)[0]
    fs, fp, fft = case.fs, case.frame_period, case.fft_size
    _, x, x_off, f_off = _batch(case, gpu)
    f0, sp, ap = ops.wav2world(x, x_off, f_off, fs, fp, fft)
    f0_s = ops.stonemask(x, x_off, ops.dio(x, x_off, f_off, fs, fp), f_off, fs, fp)
    sp_s, _, _ = ops.cheaptrick_mcep(x, x_off, f0_s, f_off, fs, fp, fft)
    ap_s, _ = ops.d4c(x, x_off, f0_s, f_off, fs, fp, fft)
    assert sp.shape == (f_off[-1], fft // 2 + 1) and ap.shape == sp.shape
    assert torch.equal(f0, f0_s) and torch.equal(sp, sp_s) and torch.equal(ap, ap_s)
    _check_f0(f0.cpu().numpy(), ref["f0"], "wav2world f0")
    _check_sp(sp.cpu().numpy(), ref["sp"], wc.uses_fixture(case, 0), "wav2world")
    _check_ap(ap.cpu().numpy(), ref["ap"], "wav2world")


def test_public_surface_at_10_ms_equals_the_ops_calls(gpu):
    """idiaptts_amd.world.analyse_batch (hop_ms) and WorldFeatLabelGen.extract_features_batch (hop_size_ms) at 10 ms:
    the same bits as the entry points called one by one, which test_case_matches_oracle holds to the oracle."""
    from idiaptts_amd import ops, world
    from idiaptts_amd.src.data_preparation.world.WorldFeatLabelGen import WorldFeatLabelGen
    case = wc.BY_NAME[wc.PUBLIC_CASE]
    fs, fp = case.fs, case.frame_period
    xs, x, x_off, f_off = _batch(case, gpu)
    f0 = ops.stonemask(x, x_off, ops.dio(x, x_off, f_off, fs, fp), f_off, fs, fp)
    sp, mc, _ = ops.cheaptrick_mcep(x, x_off, f0, f_off, fs, fp, order=19, alpha=0.58)
    ap, bap = ops.d4c(x, x_off, f0, f_off, fs, fp, want_bap=torch.float32)
    _check_f0(f0.cpu().numpy(), wc.oracle_run(case.name)[0]["f0"], "public f0")
    res = world.analyse_batch([xs[0]], fs, hop_ms=fp, want_sp=True, want_ap=True, want_bap=True, mcep_order=19,
                              mcep_alpha=0.58, device=gpu)[0]
    assert world.num_frames(len(xs[0]), fs, fp) == case.frames == len(res["f0"])
    for key, t in (("f0", f0), ("sp", sp), ("ap", ap), ("bap", bap), ("mcep", mc)):
        assert res[key].dtype == t.cpu().numpy().dtype, key
        assert np.array_equal(res[key], t.cpu().numpy()), key
    assert WorldFeatLabelGen.f0_estimator == "dio"
    coded, lf0, vuv, bap_f = WorldFeatLabelGen.extract_features_batch([xs[0]], fs, hop_size_ms=fp, num_coded_sps=20,
                                                                      mgc_alpha=0.58)[0]
    assert coded.shape == (case.frames, 20) and lf0.shape == (case.frames, 1)
    assert np.array_equal(coded, mc.cpu().numpy())
    assert np.array_equal(bap_f, bap.cpu().numpy())
    assert np.array_equal(vuv[:, 0] != 0, f0.cpu().numpy() > WorldFeatLabelGen.f0_silence_threshold)


def test_refused_dio_parameters_raise_and_hand_their_scratch_back(gpu):
    """What itts_dio's host checks refuse before any launch -- 20 bands (40 / 1100 / 4 channels) against MAXB = 16, a
    frame period <= 0, f0_ceil <= f0_floor -- raises the library's error; nothing stays marked busy in the scratch pool,
    and after each refusal a valid call at non-default parameters on the same stream still equals the oracle."""
    from idiaptts_amd import lib as _lib, ops
    L = _lib.load()

    def used():
        r, u, k = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _lib.check(L.itts_scratch_pool_stats(ctypes.byref(r), ctypes.byref(u), ctypes.byref(k)), "stats")
        return u.value

    case = wc.BY_NAME["dio_60_600_3_fp_7.3"]
    ref = wc.oracle_run(case.name)[0]
    fs, fp = case.fs, case.frame_period
    xs, x, x_off, f_off = _batch(case, gpu)
    f_off_5 = [0, wc.num_frames(len(xs[0]), fs, 5.0)]
    _check_f0(ops.dio(x, x_off, f_off, fs, fp, *case.dio).cpu().numpy(), ref["f0_dio"], "before any refusal")
    torch.cuda.synchronize()
    base = used()
    for tag, bad_fp, floor, ceil, ch in wc.REFUSED_DIO:
        with pytest.raises(_lib.IttsError):
            ops.dio(x, x_off, f_off_5, fs, bad_fp, floor, ceil, ch)
        torch.cuda.synchronize()
        assert used() == base, tag
        _check_f0(ops.dio(x, x_off, f_off, fs, fp, *case.dio).cpu().numpy(), ref["f0_dio"], "after " + tag)
    # the other entry points take the frame period too
    f0 = torch.zeros(f_off_5[1], dtype=torch.float64, device=gpu)
    K = 513
    for bad_fp in (0.0, -5.0):
        with pytest.raises(_lib.IttsError):
            ops.stonemask(x, x_off, f0, f_off_5, fs, bad_fp)
        with pytest.raises(_lib.IttsError):
            ops.cheaptrick_mcep(x, x_off, f0, f_off_5, fs, bad_fp)
        with pytest.raises(_lib.IttsError):
            ops.d4c(x, x_off, f0, f_off_5, fs, bad_fp)
        with pytest.raises(_lib.IttsError):
            sp = torch.ones((f_off_5[1], K), dtype=torch.float64, device=gpu)
            ops.world_synthesize(f0, sp, sp, f_off_5, fs, bad_fp, y_off=[0, len(xs[0])])
    torch.cuda.synchronize()
    assert used() == base
    f0s = ops.stonemask(x, x_off, _dev(gpu, [ref["f0_dio"]]), f_off, fs, fp)
    _check_f0(f0s.cpu().numpy(), ref["f0"], "stonemask after the refusals")
