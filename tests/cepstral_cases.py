"""The case tables of tests/test_gpu_cepstral.py: the mel-cepstral kernels (csrc/mcep_lockstep.hip, itts_mgc2sp in
csrc/world_frame.hip, csrc/mgcep.hip) at every solve width, transform size, stopping rule and output form
(tests/test_cepstral_cases.py shows, from the C oracle alone, that no case is degenerate, that no case that asserts
Newton trip counts sits on the stopping margin, and that the oracle itself holds the closed form below to 1e-12).
Plain numpy: no GPU import.

The closed form.  A mel-generalized cepstrum c[0..m] at warping alpha and exponent gamma IS the spectrum
    log|D(w)| = Re C(w~)                      gamma = 0
              = (1 / gamma) log|1 + gamma C(w~)|  otherwise,
    C(w~) = sum_m c[m] exp(-j m w~),   w~ = w + 2 atan2(alpha sin w, 1 - alpha cos w),
so decoding (mgc2sp) has a reference with no recursion, no transform and no third-party code, and so has analysis
(mcep / mgcep) of a spectrum that lies inside the model class: with eps = 0 and a threshold on the rounding floor it
must return the generating coefficients.

Envelopes.  amp(K, n, seed) evaluates the closed form (gamma 0, alpha 0.58) at seeded rows of the mel-cepstrum columns
of the reference's fixture LJ001-0008.cmp, on the K bins w = pi k / (K - 1): speech envelopes at any transform size
without audio.  Every array handed out is read-only and computed once per process."""
import collections
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE_ALPHA = 0.58
FIXTURE_ORDER = 19              # amp() keeps the first 20 of the fixture's 60 mel-cepstrum columns
FIXTURE_COLUMNS = 60
T = 37                          # no multiple of 4 (frames per workgroup of the solvers), 16 (per wave) or 128
T_LONG = 1100                   # >= 1024: launch_gemm_f64's long-K kernels; no multiple of 16, 37 or 128
PIN_THRESHOLD, PIN_MAXITER = 1e-13, 80
ORACLE_PIN = 1e-12              # what test_cepstral_cases.py holds the oracle to, against the closed form


# ------------------------------------------------------------------------------------------ the closed form
def warped(w, alpha):
    return w + 2.0 * np.arctan2(alpha * np.sin(w), 1.0 - alpha * np.cos(w))


def log_model(c, alpha, gamma, K):
    """log|D| on the K bins w = pi k / (K - 1) of the model with coefficients c [n, m + 1] -> [n, K]."""
    c = np.atleast_2d(np.asarray(c, dtype=np.float64))
    wt = warped(np.pi * np.arange(K) / (K - 1), alpha)
    C = c.astype(np.complex128) @ np.exp(-1j * np.outer(np.arange(c.shape[1]), wt))
    if gamma == 0.0:
        return np.ascontiguousarray(C.real)
    return np.log(np.abs(1.0 + gamma * C)) / gamma


# ------------------------------------------------------------------------------------------ envelopes
@functools.lru_cache(maxsize=None)
def fixture_mcep():
    cmp_ = np.fromfile(os.path.join(GOLDEN, "LJ001-0008.cmp"), dtype=np.float32).reshape(-1, 67)
    mc = cmp_[:, :FIXTURE_COLUMNS].astype(np.float64)
    mc.setflags(write=False)
    return mc


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def amp(K, n_frames=T, seed=0, ripple=None):
    """Amplitude envelopes [n_frames, K]: the fixture's mel-cepstra at seeded rows (drawn with replacement, each with
    a seeded perturbation of 0.02, so that no two rows are equal).  ripple None: the first 20 columns, an envelope
    that a model of order >= 19 at alpha 0.58 holds exactly.  ripple r: all 60 columns plus r cos(2 pi k / period),
    period 8 .. 40 bins, on the log amplitude -- the harmonics of an STFT spectrum, outside every model of the tables,
    so that Newton's method takes more than three rounds."""
    rng = np.random.default_rng(20240 + seed)
    mc = fixture_mcep()[:, :FIXTURE_ORDER + 1 if ripple is None else FIXTURE_COLUMNS]
    rows = rng.integers(0, len(mc), n_frames)
    log_amp = log_model(mc[rows] + rng.normal(0.0, 0.02, (n_frames, mc.shape[1])), FIXTURE_ALPHA, 0.0, K)
    if ripple is not None:
        period = rng.uniform(8.0, 40.0, (n_frames, 1))
        log_amp = log_amp + ripple * np.cos(2.0 * np.pi * np.arange(K)[None, :] / period)
    return _frozen(np.exp(log_amp))


def pin_coefficients(order, n_frames=40, start=100):
    """Rows start .. start + n of the fixture's mel-cepstra cut to `order`: the generating coefficients of the pin."""
    assert order < FIXTURE_COLUMNS
    return _frozen(fixture_mcep()[start:start + n_frames, :order + 1])


# ------------------------------------------------------------------------------------------ analysis cases
# kind "mcep" (gamma is None) or "mgcep"; `rule` holds the stopping arguments that differ from the defaults
Analysis = collections.namedtuple("Analysis", "name kind K order alpha gamma frames seed ripple rule")
DEFAULT_RULE = dict(eps=1e-8, miniter=2, maxiter=30, threshold=1e-3)


def _an(name, kind, K, order, alpha, gamma=None, frames=T, seed=0, ripple=None, **rule):
    return Analysis(name, kind, K, order, alpha, gamma, frames, seed, ripple, tuple(sorted(rule.items())))


def tiled(a, n_frames):
    """n_frames rows that repeat the rows of a in turn.  A long batch is 37 distinct frames again and again (37 shares
    no factor with the 4, 16 or 128 frames a workgroup owns), so that the oracle, which takes 8 ms a frame at order 79,
    computes 37 frames and not 1100: frames are independent in the oracle and must be in the kernels."""
    return _frozen(a[np.arange(n_frames) % len(a)])


def amp_of(case):
    return tiled(amp(case.K, min(case.frames, T), case.seed, case.ripple), case.frames)


def rule_of(case):
    r = dict(DEFAULT_RULE)
    r.update(dict(case.rule))
    return r


# A: every solve kernel of mcep_lockstep at K = 513.  m1 = order + 1 picks mcls_solve_dpp_kernel<20|24|32|48|60|64> or
# the LDS solver (m1 > 64); 2 order + 1 <= 64 picks mcls_fused3_kernel<4>, otherwise <8>; order > 63: the unfused form
WIDTH_ORDERS = (1, 5, 19, 20, 23, 24, 31, 32, 40, 47, 48, 59, 60, 61, 63, 64, 79, 127)
SOLVE_WIDTHS = (20, 24, 32, 48, 60, 64)


def solve_width(order):
    """The template width of the solve kernel order runs on; None: the LDS solver."""
    return next((w for w in SOLVE_WIDTHS if order + 1 <= w), None)


def fused_form(order):
    """4 / 8: the column groups of mcls_fused3_kernel; None: the separate launches."""
    return None if order > 63 else (4 if 2 * order + 1 <= 64 else 8)


# one alpha per transform size: the warping tables are cached per (order, size, alpha)
ALPHA_OF_K = {33: 0.31, 65: 0.35, 129: 0.42, 257: 0.466, 513: 0.58, 1025: 0.77}
# seeds: a case whose oracle trip counts move within threshold (1 +- 1e-6) takes the next seed
#        (test_cepstral_cases.py::test_trip_counts_are_off_the_stopping_margin)
# The sweep runs on the 60-column envelopes (ripple 0): outside the model class below order 59, so that the upper
# coefficients are not zeros and frames leave the work list round by round
WIDTH_CASES = [_an("width_o%d" % o, "mcep", 513, o, ALPHA_OF_K[513], ripple=0.0) for o in WIDTH_ORDERS]
SIZE_ORDERS = {33: (1, 19, 31), 65: (1, 19, 31, 63), 129: (1, 31, 63, 127), 257: (19, 63, 127), 1025: (1, 31, 127)}
SIZE_CASES = [_an("size_K%d_o%d" % (K, o), "mcep", K, o, ALPHA_OF_K[K]) for K in sorted(SIZE_ORDERS)
              for o in SIZE_ORDERS[K]]
# C: T >= 1024 and K > 64 send launch_gemm_f64 to gemm_f64_lds_kernel: order 79 has no fused form, order 59 with
# ITTS_MCEP_FUSED=0 takes the same launches
LONG_CASES = [_an("long_o79", "mcep", 513, 79, 0.58, frames=T_LONG),
              _an("long_o59_unfused", "mcep", 513, 59, 0.58, frames=T_LONG)]
LONG_DECODE_ORDERS = (79, 64)          # ops.mgc2sp's fallback: m1 = 80 (vector loads, LDS kernel), 65 (staged kernel)

# D: the stopping rules, order 24, alpha 0.42, for mcep and mgcep (gamma -1/3), on envelopes outside the model class:
# threshold 1e-12 under a cap of 8 rounds must stop some frames at the cap and some before it.  mcep does on the
# 60-column envelopes (6 / 7 / 8 rounds); mgcep's criterion settles in 5 .. 7 rounds there and needs the ripple
RULES = [("maxiter1", dict(maxiter=1)), ("miniter5", dict(miniter=5)),
         ("tight_capped", dict(threshold=1e-12, maxiter=8)), ("miniter6_maxiter4", dict(miniter=6, maxiter=4)),
         ("eps0", dict(eps=0.0)), ("eps1e-3", dict(eps=1e-3))]
RULE_CASES = [_an("rule_%s_%s" % (kind, tag), kind, 513, 24, 0.42, gamma, ripple=ripple, **rule)
              for kind, gamma, ripple in (("mcep", None, 0.0), ("mgcep", -1.0 / 3.0, 3.0)) for tag, rule in RULES]

# G: mgcep_kernel away from K = 513: its NQ x 256 threads over f2 + 1 bins, its 2 x 64 lanes over 2 m + 1 outputs
GAMMAS = (-1.0 / 3.0, -0.5, -0.9, -1.0, 0.0)
# Orders 1, 5, 31, 62, 63 wherever order < K - 1, at every gamma, but for the (K, order, gamma) at which the ORACLE is
# ill conditioned.  An order within two of K - 1 (31 at K = 33; 62 and 63 at K = 65) makes its Newton system singular on
# these order-19 envelopes for every gamma but -1 (which takes one LPC step and no Newton round): NaN, or 30 rounds and
# coefficients that move by their own size when the input moves by one ulp.  So does gamma -0.9 at (65, 31), (129, 62)
# and (129, 63): 30 rounds, a relative change of 0.15 .. 1.7 per ulp.  No kernel can be held to 1e-8 there;
# test_cepstral_cases.py holds every kept case to a change below 1e-10 per ulp.  Order 11 at K = 33 stands in for the
# high order that K = 33 loses at gamma != -1 (order 15 at gamma -0.9 already changes by 0.7 per ulp).
MGCEP_ORDER_LIST = (1, 5, 31, 62, 63)
MGCEP_ORDERS = {K: tuple(o for o in MGCEP_ORDER_LIST if o < K - 1) for K in (33, 65, 129, 257, 1025)}
MGCEP_ORDERS[33] = (1, 5, 11, 31)
MGCEP_ILL_CONDITIONED = {(K, o, g) for K, o in ((33, 31), (65, 62), (65, 63))
                         for g in (-1.0 / 3.0, -0.5, -0.9, 0.0)} | {(65, 31, -0.9), (129, 62, -0.9), (129, 63, -0.9)}
MGCEP_FRAMES = (1, 3, T)               # the first 1 and 3 frames of the T: frames are independent


def gamma_tag(g):
    return "g%.2f" % -g


MGCEP_CASES = [_an("mgcep_K%d_o%d_%s" % (K, o, gamma_tag(g)), "mgcep", K, o, ALPHA_OF_K[K], g)
               for K in sorted(MGCEP_ORDERS) for o in MGCEP_ORDERS[K] for g in GAMMAS
               if (K, o, g) not in MGCEP_ILL_CONDITIONED]

COUNTED = WIDTH_CASES + SIZE_CASES + LONG_CASES + RULE_CASES + MGCEP_CASES      # cases that assert trip counts
BY_NAME = {c.name: c for c in COUNTED}
assert len(BY_NAME) == len(COUNTED)

# E: degenerate rows between fixture envelopes (an STFT of silence is an all-zero row)
DEGENERATE_ROWS = {2: 0.0, 4: 1e-6, 5: 1.0}
DEGENERATE_FRAMES = 8
DEGENERATE = dict(K=513, order=24, alpha=0.42, gamma=-1.0 / 3.0)


@functools.lru_cache(maxsize=None)
def degenerate_amp():
    a = amp(DEGENERATE["K"], DEGENERATE_FRAMES, seed=3).copy()
    for r, v in DEGENERATE_ROWS.items():
        a[r] = v
    return _frozen(a)


@functools.lru_cache(maxsize=None)
def oracle_analysis(name, threshold_scale=1.0):
    """(coefficients [frames, order + 1], trip counts) of a COUNTED case by the C oracle, once per process."""
    from oracle import capi
    c = BY_NAME[name]
    r = rule_of(c)
    r["threshold"] = r["threshold"] * threshold_scale
    a = amp_of(c)[:T]
    if c.kind == "mcep":
        out, it = capi.mcep(a, c.order, c.alpha, return_iters=True, **r)
    else:
        out, it = capi.mgcep(a, c.order, c.alpha, c.gamma, return_iters=True, **r)
    return tiled(out, c.frames), tiled(it, c.frames)


# ------------------------------------------------------------------------------------------ decode cases
# H: coefficients come from the oracle's analysis of amp(513) -- minimum phase by construction; random ones let
# 1 + gamma C cross zero.  Order 0 is the gain of the order 1 analysis.
DECODE_FRAMES = (1, 2, 3, 5, T)        # mg_gc2gc_rows_kernel: 4 frames per workgroup; the first n of the T
DECODE_GAMMA_FFT = (64, 128, 2048, 4096)
DECODE_GAMMA_ORDERS = (0, 19, 63, 64, 100)
DECODE_GAMMAS = (-1.0 / 3.0, -0.5, -1.0)
DECODE_FFT = (64, 512, 2048, 4096, 8192)
DECODE_ORDERS = (0, 18, 19, 63, 64)
DECODE_ALPHA = {64: 0.31, 128: 0.35, 512: 0.42, 2048: 0.77, 4096: 0.58, 8192: 0.466}


@functools.lru_cache(maxsize=None)
def decode_coefficients(order, alpha, gamma, n_frames=T):
    from oracle import capi
    a = amp(513, n_frames, seed=1)
    m = max(order, 1)
    c = capi.mcep(a, m, alpha) if gamma == 0.0 else capi.mgcep(a, m, alpha, gamma)
    return _frozen(c[:, :order + 1])


@functools.lru_cache(maxsize=None)
def oracle_decode(order, alpha, gamma, fftlen, n_frames=T):
    from oracle import capi
    c = decode_coefficients(order, alpha, gamma, n_frames)
    if gamma == 0.0:
        return _frozen(capi.mgc2sp_logamp(c, alpha, fftlen))
    return _frozen(capi.mgc2sp_gamma_logamp(c, alpha, gamma, fftlen))


# ------------------------------------------------------------------------------------------ the closed-form pin
# I: chosen from the measured table of the oracle's own distance to the closed form; every
# case here is one the ORACLE holds to ORACLE_PIN (test_cepstral_cases.py prints its distance).
# Decoding at fftlen 4096, where the truncation of the de-warped cepstrum is below rounding.
PinDecode = collections.namedtuple("PinDecode", "gamma alpha order fftlen")
PIN_DECODE = [PinDecode(g, a, o, 4096) for g in (0.0, -1.0 / 3.0, -0.5) for a, o in
              ((0.0, 19), (0.42, 5), (0.58, 31), (0.77, 19))] + \
             [PinDecode(-0.9, a, o, 4096) for a, o in ((0.1, 31), (0.58, 19))] + [PinDecode(0.0, 0.58, 19, 8192)]
# Recovery with eps = 0, threshold 1e-13, at most 80 rounds: (gamma, alpha, order, K)
PinRecover = collections.namedtuple("PinRecover", "gamma alpha order K")
PIN_RECOVER = [PinRecover(0.0, 0.58, 19, K) for K in (129, 257, 513, 1025)] + \
              [PinRecover(-1.0 / 3.0, 0.58, 19, 513), PinRecover(-1.0 / 3.0, 0.58, 19, 1025),
               PinRecover(-0.5, 0.58, 19, 1025), PinRecover(-0.9, 0.1, 19, 1025)]
PIN_RULE = dict(eps=0.0, miniter=2, maxiter=PIN_MAXITER, threshold=PIN_THRESHOLD)


def pin_decode_reference(p):
    return log_model(pin_coefficients(p.order), p.alpha, p.gamma, p.fftlen // 2 + 1)


def pin_recover_amp(p):
    return _frozen(np.exp(log_model(pin_coefficients(p.order), p.alpha, p.gamma, p.K)))
