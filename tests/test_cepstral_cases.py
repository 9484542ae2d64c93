"""tests/cepstral_cases.py reaches what it claims and the reference alone meets every condition that
tests/test_gpu_cepstral.py relies on, by the C oracle and numpy (no GPU):

* the tables hold every solve width, both fused forms on either side of their boundary, the sizes, stopping rules,
  exponents and frame counts they are meant to hold;
* every case's oracle output is finite, and well conditioned: it moves by less than 1e-10 max(1, |c|) when every input
  bin moves by one ulp, so that the 1e-8 the kernels are held to leaves a hundred such perturbations to their other
  order of summation;
* no case that asserts Newton trip counts sits on the stopping margin: the oracle's counts are the same at
  threshold (1 - 1e-6), threshold and threshold (1 + 1e-6);
* the oracle itself (orc_mcep, orc_mgcep, orc_mgc2sp_logamp, orc_mgc2sp_gamma) holds the closed form of the model
  spectrum to 1e-12: decoding, and recovery of the generating coefficients from a spectrum inside the model class.
  This pins the oracle for gamma != 0 with no third-party code.  The measured distances are printed (pytest -s)."""
import numpy as np
import pytest

import cepstral_cases as cc

COUNTED = [c.name for c in cc.COUNTED]
SHORT = [c.name for c in cc.COUNTED if c.frames == cc.T]


def _say(*parts):
    print("[cepstral_cases]", *parts)


def test_the_tables_hold_what_they_claim():
    orders = [c.order for c in cc.WIDTH_CASES]
    assert orders == [1, 5, 19, 20, 23, 24, 31, 32, 40, 47, 48, 59, 60, 61, 63, 64, 79, 127]
    assert all(c.K == 513 and c.alpha == 0.58 and c.kind == "mcep" and c.ripple == 0.0 for c in cc.WIDTH_CASES)
    # every solve kernel, each both full (m1 == width) and padded (m1 < width), and the LDS solver
    for w in cc.SOLVE_WIDTHS:
        m1s = [o + 1 for o in orders if cc.solve_width(o) == w]
        assert w in m1s and any(m1 < w for m1 in m1s), w
    assert [o for o in orders if cc.solve_width(o) is None] == [64, 79, 127]
    # the fused kernel's two forms meet between orders 31 and 32; above 63 there is none
    assert cc.fused_form(31) == 4 and cc.fused_form(32) == 8 and cc.fused_form(63) == 8 and cc.fused_form(64) is None
    assert {c.K for c in cc.SIZE_CASES} == {33, 65, 129, 257, 1025}
    for c in cc.SIZE_CASES + cc.MGCEP_CASES:
        assert 1 <= c.order < c.K - 1 and c.alpha == cc.ALPHA_OF_K[c.K]
    assert {c.order for c in cc.SIZE_CASES} == {1, 19, 31, 63, 127}
    assert [(c.order, c.frames) for c in cc.LONG_CASES] == [(79, 1100), (59, 1100)]
    assert cc.LONG_DECODE_ORDERS == (79, 64)
    assert cc.T % 4 and cc.T % 16 and cc.T % 128 and cc.T_LONG >= 1024 and cc.T_LONG % 16 and cc.T_LONG % 128 \
        and cc.T_LONG % cc.T
    assert len(cc.RULE_CASES) == 12 and all(c.order == 24 and c.alpha == 0.42 for c in cc.RULE_CASES)
    assert {c.gamma for c in cc.RULE_CASES} == {None, -1.0 / 3.0}
    assert {c.rule for c in cc.RULE_CASES} == {
        (("maxiter", 1),), (("miniter", 5),), (("maxiter", 8), ("threshold", 1e-12)), (("maxiter", 4), ("miniter", 6)),
        (("eps", 0.0),), (("eps", 1e-3),)}
    assert {c.K for c in cc.MGCEP_CASES} == {33, 65, 129, 257, 1025}
    assert {c.gamma for c in cc.MGCEP_CASES} == {-1.0 / 3.0, -0.5, -0.9, -1.0, 0.0}
    assert cc.MGCEP_FRAMES == (1, 3, 37)
    # orders 1, 5, 31, 62, 63 wherever order < K - 1, at every gamma: each is a case or is named as ill conditioned
    held = {(c.K, c.order, c.gamma) for c in cc.MGCEP_CASES}
    for K in (33, 65, 129, 257, 1025):
        for o in (1, 5, 31, 62, 63):
            for g in cc.GAMMAS:
                if o < K - 1:
                    assert ((K, o, g) in held) != ((K, o, g) in cc.MGCEP_ILL_CONDITIONED), (K, o, g)
    assert len(cc.MGCEP_ILL_CONDITIONED) == 15 and all(g != -1.0 for _, _, g in cc.MGCEP_ILL_CONDITIONED)
    assert (65, 63, -1.0) in held              # the smallest transform with 127 autocorrelation outputs
    # gamma = -1 is held to the oracle at every size, and is in no recovery case
    assert {c.K for c in cc.MGCEP_CASES if c.gamma == -1.0} == {33, 65, 129, 257, 1025}
    assert all(p.gamma != -1.0 for p in cc.PIN_RECOVER + cc.PIN_DECODE)
    for pins in (cc.PIN_DECODE, cc.PIN_RECOVER):
        assert {p.gamma for p in pins} == {0.0, -1.0 / 3.0, -0.5, -0.9}
    assert cc.DECODE_GAMMA_FFT == (64, 128, 2048, 4096) and cc.DECODE_FFT == (64, 512, 2048, 4096, 8192)
    assert cc.DECODE_GAMMA_ORDERS == (0, 19, 63, 64, 100) and cc.DECODE_ORDERS == (0, 18, 19, 63, 64)
    assert cc.DECODE_FRAMES == (1, 2, 3, 5, 37)


def test_envelopes_are_speech_like_at_every_size():
    """amp(): positive, finite, more than 10 dB of range, no two rows equal, and the same envelope at every K (the bins
    of a smaller transform are every other bin of the next)."""
    for K in (33, 65, 129, 257, 513, 1025):
        a = cc.amp(K)
        assert a.shape == (cc.T, K) and np.isfinite(a).all() and (a > 0).all()
        assert (20 * np.log10(a.max(axis=1) / a.min(axis=1)) > 10).all()
        assert len({r.tobytes() for r in a}) == cc.T
    assert np.allclose(cc.amp(1025)[:, ::2], cc.amp(513), rtol=1e-12)
    long = cc.amp_of(cc.LONG_CASES[0])
    assert long.shape == (cc.T_LONG, 513) and np.array_equal(long[cc.T:2 * cc.T], long[:cc.T])


@pytest.mark.parametrize("name", COUNTED)
def test_oracle_output_is_finite(name):
    out, it = cc.oracle_analysis(name)
    c = cc.BY_NAME[name]
    assert out.shape == (c.frames, c.order + 1) and np.isfinite(out).all()
    assert it.min() >= 0 and it.max() <= cc.rule_of(c)["maxiter"]


@pytest.mark.parametrize("name", SHORT)
def test_oracle_is_well_conditioned(name):
    from oracle import capi
    c = cc.BY_NAME[name]
    out, it = cc.oracle_analysis(name)
    a = cc.amp_of(c)
    sign = np.random.default_rng(5).choice([-1.0, 1.0], a.shape)
    moved = a * (1.0 + sign * 2.0 ** -52)
    if c.kind == "mcep":
        out2, it2 = capi.mcep(moved, c.order, c.alpha, return_iters=True, **cc.rule_of(c))
    else:
        out2, it2 = capi.mgcep(moved, c.order, c.alpha, c.gamma, return_iters=True, **cc.rule_of(c))
    change = float(np.abs(out2 - out).max() / max(1.0, np.abs(out).max()))
    _say(name, "change per ulp of the input", change, "max |c|", float(np.abs(out).max()))
    assert np.array_equal(it, it2)
    assert change < 1e-10


@pytest.mark.parametrize("name", COUNTED)
def test_trip_counts_are_off_the_stopping_margin(name):
    it = cc.oracle_analysis(name)[1]
    assert np.array_equal(it, cc.oracle_analysis(name, 1.0 - 1e-6)[1])
    assert np.array_equal(it, cc.oracle_analysis(name, 1.0 + 1e-6)[1])


def test_stopping_rules_do_what_their_names_say():
    for kind in ("mcep", "mgcep"):
        it = {tag: cc.oracle_analysis("rule_%s_%s" % (kind, tag))[1] for tag, _ in cc.RULES}
        assert (it["maxiter1"] == 1).all()
        assert (it["miniter5"] >= 5).all()
        assert (it["miniter6_maxiter4"] == 4).all()         # the floor is never reached: every frame hits the cap
    # threshold 1e-12 with a cap of 8: frames that stop at the cap AND frames that stop before it
    for kind in ("mcep", "mgcep"):
        it = cc.oracle_analysis("rule_%s_tight_capped" % kind)[1]
        _say("tight_capped", kind, "trip counts", np.bincount(it).tolist())
        assert (it == 8).any() and (it < 8).any(), kind
    # eps changes the result: the cases are not the default in disguise
    for kind in ("mcep", "mgcep"):
        a, b = (cc.oracle_analysis("rule_%s_%s" % (kind, t))[0] for t in ("eps0", "eps1e-3"))
        assert np.abs(a - b).max() > 1e-3


def test_degenerate_rows_are_finite_in_the_oracle():
    """An all-zero row, a flat 1e-6 row and a flat 1.0 row: with the default eps the periodogram is flat and positive,
    and the answer is log of its level in c0 and zeros."""
    from oracle import capi
    d = cc.DEGENERATE
    a = cc.degenerate_amp()
    mc = capi.mcep(a, d["order"], d["alpha"])
    mgc = capi.mgcep(a, d["order"], d["alpha"], d["gamma"])
    assert np.isfinite(mc).all() and np.isfinite(mgc).all()
    for r, v in cc.DEGENERATE_ROWS.items():
        assert (a[r] == v).all()
        assert abs(mc[r, 0] - 0.5 * np.log(v * v + 1e-8)) < 1e-9 and np.abs(mc[r, 1:]).max() < 1e-9
        assert np.abs(mgc[r, 1:]).max() < 1e-9
    others = [r for r in range(cc.DEGENERATE_FRAMES) if r not in cc.DEGENERATE_ROWS]
    assert len(others) >= 3 and (np.abs(mc[others, 1:]).max(axis=1) > 0.1).all()


def test_decode_cases_are_finite():
    for gamma in cc.DECODE_GAMMAS:
        for fftlen in cc.DECODE_GAMMA_FFT:
            for order in cc.DECODE_GAMMA_ORDERS:
                if order <= fftlen // 2:
                    ref = cc.oracle_decode(order, cc.DECODE_ALPHA[fftlen], gamma, fftlen)
                    assert ref.shape == (cc.T, fftlen // 2 + 1) and np.isfinite(ref).all(), (gamma, fftlen, order)
    for fftlen in cc.DECODE_FFT:
        for order in cc.DECODE_ORDERS:
            if order <= fftlen // 2:
                assert np.isfinite(cc.oracle_decode(order, cc.DECODE_ALPHA[fftlen], 0.0, fftlen)).all()


@pytest.mark.parametrize("p", cc.PIN_DECODE,
                         ids=lambda p: "g%.2f_a%.2f_o%d_fft%d" % (-p.gamma, p.alpha, p.order, p.fftlen))
def test_oracle_decoding_equals_the_closed_form(p):
    from oracle import capi
    c = cc.pin_coefficients(p.order)
    ref = cc.pin_decode_reference(p)
    got = capi.mgc2sp_logamp(c, p.alpha, p.fftlen) if p.gamma == 0.0 else \
        capi.mgc2sp_gamma_logamp(c, p.alpha, p.gamma, p.fftlen)
    dist = float(np.abs(got - ref).max())
    _say("decode", p, "max |oracle - closed form|", dist, "max |log D|", float(np.abs(ref).max()))
    assert np.isfinite(ref).all() and np.ptp(ref, axis=1).min() > 0.25         # envelopes, not constants
    assert dist < cc.ORACLE_PIN


@pytest.mark.parametrize("p", cc.PIN_RECOVER, ids=lambda p: "g%.2f_a%.2f_o%d_K%d" % (-p.gamma, p.alpha, p.order, p.K))
def test_oracle_analysis_recovers_the_closed_form(p):
    from oracle import capi
    c = cc.pin_coefficients(p.order)
    a = cc.pin_recover_amp(p)
    if p.gamma == 0.0:
        got, it = capi.mcep(a, p.order, p.alpha, return_iters=True, **cc.PIN_RULE)
    else:
        got, it = capi.mgcep(a, p.order, p.alpha, p.gamma, return_iters=True, **cc.PIN_RULE)
    err = float((np.abs(got - c) / np.maximum(1.0, np.abs(c))).max())
    _say("recover", p, "max |oracle - c| / max(1, |c|)", err, "trip counts", int(it.min()), "..", int(it.max()))
    assert it.max() < cc.PIN_MAXITER
    assert err < cc.ORACLE_PIN
