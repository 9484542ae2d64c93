"""tests/world_param_cases.py reaches what it claims, by the C oracle alone (no GPU): the band count, the contour
kernel's window, the frame count and the synthesis length of every case from the closed formulas; a voiced share of
DIO + StoneMask within [0.25, 0.9] for every utterance that is neither silent nor too short to voice, so that no case
compares two all-unvoiced contours; a finite, non-zero synthesis."""
import numpy as np
import pytest

import world_param_cases as wc

NAMES = [c.name for c in wc.CASES]


def test_the_table_holds_what_the_issue_lists():
    by = wc.BY_NAME
    full = [c for c in wc.CASES if c.stages == wc.STAGES and len(c.signals) == 1]
    assert {(c.fs, c.frame_period) for c in full if c.dio == wc.DIO_DEFAULT} >= {
        (16000, 1.0), (16000, 2.5), (16000, 3.0), (16000, 7.3), (16000, 10.0), (16000, 12.5), (48000, 10.0)}
    # the synthesis: every period on the wave kernels (fft 1024), the sized (2048) and the generic (512) kernels
    assert {c.frame_period for c in full if wc.fft_size_of(c) == 1024} >= {1.0, 2.5, 3.0, 7.3, 10.0, 12.5}
    assert {(c.fs, c.frame_period, wc.fft_size_of(c)) for c in full} >= {
        (16000, 10.0, 2048), (16000, 2.5, 512), (48000, 10.0, 2048)}
    assert any(c.preemphasis == 0.97 for c in full)
    dios = {(c.frame_period,) + c.dio for c in wc.CASES}
    assert dios >= {(5.0, 50, 400, 2, 0.1), (5.0, 100, 300, 1, 0.2), (5.0, 40, 600, 3, 0.1), (5.0, 50, 790, 4, 0.1),
                    (5.0, 71, 800, 2, 0.02), (7.3, 60, 600, 3, 0.15)}
    assert by["dio_100_300_1"].nb == 2 and by["dio_40_600_3"].nb == 12 and by["dio_50_790_4"].nb == wc.MAXB
    assert [by[n].frames - by[n].vrm for n in ("short_T_below_vrm", "short_T_vrm_plus_1", "short_T_vrm_plus_2")] \
        == [-10, 1, 2] and by["short_T_below_vrm"].vrm == 51
    assert by["dio_9s_fp_1"].frames > 8192 and by["dio_9s_fp_1"].stages == ("dio",)
    ct = [c for c in wc.CASES if c.stages == wc.STAGES[:3]]
    assert {c.q1 for c in ct} >= {-0.09, 0.0} and {c.fft_size for c in ct} >= {2048, 512}
    assert any(c.mcep for c in ct)
    d4 = [c for c in wc.CASES if c.stages == ("dio", "stonemask", "d4c")]
    assert {c.threshold for c in d4} >= {0.0, 0.5, 1.0} and any(c.fft_size == 2048 for c in d4)
    assert any(c.want_bap for c in d4)
    rag = by["ragged_fp_7.3"]
    assert rag.voicing == ("normal", "short", "silent") and rag.stages == wc.STAGES and rag.dio == wc.RAGGED_DIO
    for c in wc.CASES:                                # 2 s at the most, but for the case that says otherwise
        for x in wc.signals(c):
            assert len(x) <= 2 * c.fs or c.name == "dio_9s_fp_1"
    w2w = by[wc.WAV2WORLD_CASE]
    assert w2w.frame_period == 10.0 and w2w.fft_size and w2w.dio == wc.DIO_DEFAULT
    assert by[wc.PUBLIC_CASE].frame_period == 10.0 and by[wc.PUBLIC_CASE].dio == wc.DIO_DEFAULT
    refused = {r[0]: r[1:] for r in wc.REFUSED_DIO}
    assert wc.dio_bands(*refused["nb_20"][1:]) == 20


@pytest.mark.parametrize("name", NAMES)
def test_case_geometry_and_voicing(name):
    case = wc.BY_NAME[name]
    floor, ceil, ch, _ = case.dio
    assert wc.dio_bands(floor, ceil, ch) == case.nb <= wc.MAXB
    assert wc.voice_range_minimum(case.frame_period, floor) == case.vrm
    res = wc.oracle_run(name)
    for u, (x, r) in enumerate(zip(wc.signals(case), res)):
        T = wc.num_frames(len(x), case.fs, case.frame_period)
        if case.frames is not None and len(case.signals) == 1:
            assert T == case.frames
        assert len(r["f0_dio"]) == T
        assert np.array_equal(r["tp"], np.arange(T) * case.frame_period / 1000.0)
        f0 = r.get("f0", r["f0_dio"])
        share = float((f0 > 0).mean())
        if case.voicing[u] == "normal":
            assert wc.VOICED_SHARE[0] <= share <= wc.VOICED_SHARE[1], share
            assert T > case.vrm
        else:
            assert share == 0.0
        if case.voicing[u] == "short":
            assert np.abs(x).max() > 0
        K = wc.fft_size_of(case) // 2 + 1
        for key in ("sp", "ap"):
            if key in r:
                assert r[key].shape == (T, K) and np.isfinite(r[key]).all() and (r[key] > 0).all()
        if "y" in r:
            assert len(r["y"]) == wc.synth_length(T, case.fs, case.frame_period)
            assert np.isfinite(r["y"]).all()
            if case.voicing[u] != "silent":
                assert np.abs(r["y"]).max() > 0
    if "synth" in case.stages:
        assert any(np.abs(r["y"]).max() > 0 for r in res)


def test_odd_periods_round_off_the_hop_grid():
    """3 and 7.3 ms: the signal is no whole number of hops, so the frame count comes from a rounding; at 7.3 ms the hop
    is 116.8 samples, so the synthesis length does too."""
    for name in ("fp_3", "fp_7.3"):
        case = wc.BY_NAME[name]
        n = len(wc.signals(case)[0])
        hop = case.frame_period * case.fs / 1000.0
        assert n / hop != int(n / hop)
        assert wc.synth_length(case.frames, case.fs, case.frame_period) != n
    case = wc.BY_NAME["fp_7.3"]
    exact = case.frames * 7.3 * 16.0
    assert exact != int(exact) and wc.synth_length(case.frames, case.fs, 7.3) == int(exact) == 30484


def test_fft_512_sends_low_frames_to_the_default_f0():
    """CheapTrick's F0 floor is 3 fs / (fft - 3): 94 Hz at 512; the case must hold voiced frames below it."""
    case = wc.BY_NAME["ct_fft512"]
    f0 = wc.oracle_run(case.name)[0]["f0"]
    floor = 3.0 * case.fs / (512 - 3.0)
    assert 94 < floor < 95
    assert ((f0 > 0) & (f0 <= floor)).any() and (f0 > floor).any()


def test_thresholds_change_lovetrain_decisions():
    """D4C's threshold decides which frames LoveTrain calls unvoiced (aperiodicity 1 - 1e-12 in every bin): 0 keeps
    all voiced frames, 1 rejects every frame, 0.5 sits between."""
    unv = {}
    for name in ("d4c_thr_0", "d4c_thr_0.5_bap", "d4c_thr_1"):
        r = wc.oracle_run(name)[0]
        unv[name] = int((r["ap"][:, 0] > 0.999).sum())
        voiced = int((r["f0"] > 0).sum())
    T = len(r["f0"])
    assert unv["d4c_thr_0"] == T - voiced
    assert unv["d4c_thr_1"] == T
    assert unv["d4c_thr_0"] <= unv["d4c_thr_0.5_bap"] < T
