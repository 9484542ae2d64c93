"""The case table of tests/test_gpu_world_params.py: the WORLD entry points away from 5 ms and DIO's 71 / 800 / 2 / 0.1
(tests/test_world_param_cases.py proves, from the C oracle alone, that every case reaches what it claims and does not
degenerate into an all-unvoiced contour).  Plain Python: no GPU import.

Vocabulary (csrc/dio.hip): `nb` = 1 + int(log2(f0_ceil / f0_floor) * channels_in_octave) is DIO's band count, capped
at MAXB = 16; `vrm` = int(0.5 + 1000 / frame_period / f0_floor) * 2 + 1 is the contour kernel's voice-range window: an
utterance of T <= vrm frames is unvoiced without a look at its candidates, and at T > 8192 the kernel's boundary masks
leave LDS for global scratch.  Frames sit at t * frame_period / 1000; an utterance of n samples has
int(1000 n / fs / frame_period) + 1 of them and is synthesised to int(T * frame_period * fs / 1000) samples.

Signals: the reference's fixture LJ001-0002.wav behind the pre-emphasis of tests/test_gpu_world.py -- the file is 1.9 s
(30 384 samples, a whole number of 3 ms hops), so its first 30 380 samples, which no frame period of the table
divides -- and that file's synthetic voice (harmonic source on an F0 random walk, plus noise) for other rates, lengths
and a lower voice.

The oracle is composed from the separate calls (DIO -> StoneMask -> CheapTrick -> D4C -> synthesis): its wav2world
takes neither an F0 range nor q1 nor a threshold.  oracle_run() computes a case once per process and hands out the
same arrays to every test: read, never written."""
import collections
import functools
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAXB = 16                                    # csrc/dio.hip
DIO_DEFAULT = (71.0, 800.0, 2.0, 0.1)        # f0_floor, f0_ceil, channels_in_octave, allowed_range
VOICED_SHARE = (0.25, 0.9)                   # of DIO + StoneMask's frames, for every "normal" utterance

# stages a case runs, in order; each needs the ones before it except "synth" (fed the oracle's f0 / sp / ap)
STAGES = ("dio", "stonemask", "cheaptrick", "d4c", "synth")
F0_ONLY = STAGES[:2]

# signals: ("lj", samples) | ("synthetic", seconds or ("samples", n), seed[, centre F0]) | ("silence", seconds)
# voicing (one per signal): "normal" -> voiced share within VOICED_SHARE; "silent" / "short" -> nothing voiced
Case = collections.namedtuple(
    "Case", "name fs signals voicing frame_period dio stages fft_size q1 threshold mcep want_bap preemphasis "
            "nb vrm frames")


def _case(name, signals, frame_period=5.0, dio=DIO_DEFAULT, fs=16000, stages=STAGES, fft_size=None, q1=-0.15,
          threshold=0.85, mcep=None, want_bap=False, preemphasis=0.0, voicing=None, nb=7, vrm=None, frames=None):
    if signals and not isinstance(signals[0], tuple):
        signals = (signals,)
    voicing = voicing or ("normal",) * len(signals)
    return Case(name, fs, tuple(signals), tuple(voicing), float(frame_period), tuple(float(v) for v in dio),
                tuple(stages), fft_size, q1, threshold, mcep, want_bap, preemphasis, nb, vrm, frames)


LJ = ("lj", 30380)
RAGGED_DIO = (60.0, 600.0, 3.0, 0.15)

CASES = [
    # ---- frame period, DIO's defaults, the whole chain at fft 1024 (the synthesis on its wave kernels).  3 and 7.3 ms
    # put neither the frame count nor the synthesis length on a multiple of the hop; 1 ms: five times the frames
    _case("fp_1", LJ, 1.0, vrm=29, frames=1899),
    _case("fp_2.5", LJ, 2.5, vrm=13, frames=760),
    _case("fp_3", LJ, 3.0, vrm=11, frames=633),
    _case("fp_7.3", LJ, 7.3, vrm=5, frames=261, preemphasis=0.97),
    _case("fp_10", LJ, 10.0, vrm=3, frames=190),
    _case("fp_12.5", LJ, 12.5, vrm=3, frames=152),
    _case("fp_10_48k", ("synthetic", 1.0, 2), 10.0, fs=48000, vrm=3, frames=101),      # fft 2048: sized synthesis
    # ---- other transform sizes through CheapTrick, D4C and the synthesis
    _case("fp_10_fft2048", LJ, 10.0, fft_size=2048, vrm=3, frames=190),                # sized pulse kernels
    _case("fp_2.5_fft512", LJ, 2.5, fft_size=512, vrm=13, frames=760),                 # generic pulse kernels
    # ---- DIO's range, channels and allowed range at 5 ms
    _case("dio_50_400_2", LJ, dio=(50, 400, 2, 0.1), stages=F0_ONLY, nb=7, vrm=9),
    _case("dio_100_300_1", LJ, dio=(100, 300, 1, 0.2), stages=F0_ONLY, nb=2, vrm=5),
    _case("dio_40_600_3", LJ, dio=(40, 600, 3, 0.1), stages=F0_ONLY, nb=12, vrm=11),
    _case("dio_50_790_4", LJ, dio=(50, 790, 4, 0.1), stages=F0_ONLY, nb=16, vrm=9),     # on the cap
    _case("dio_tight_range", LJ, dio=(71, 800, 2, 0.02), stages=F0_ONLY, nb=7, vrm=7),  # most candidates rejected
    _case("dio_60_600_3_fp_7.3", LJ, 7.3, dio=RAGGED_DIO, stages=F0_ONLY, nb=10, vrm=5, frames=261),
    # ---- the contour kernel's short branch (T <= vrm) away from the default vrm, and just above it
    _case("short_T_below_vrm", ("synthetic", 0.04, 6), 1.0, dio=(40, 800, 2, 0.1), stages=F0_ONLY,
          voicing=("short",), nb=9, vrm=51, frames=41),
    _case("short_T_vrm_plus_1", ("synthetic", ("samples", 816), 6), 1.0, dio=(40, 800, 2, 0.1), stages=F0_ONLY,
          voicing=("short",), nb=9, vrm=51, frames=52),
    _case("short_T_vrm_plus_2", ("synthetic", ("samples", 832), 6), 1.0, dio=(40, 800, 2, 0.1), stages=F0_ONLY,
          voicing=("short",), nb=9, vrm=51, frames=53),
    # ---- the contour kernel's masks in global scratch, reached through the frame period: 9 s at 1 ms, DIO only
    _case("dio_9s_fp_1", ("synthetic", 9.0, 9), 1.0, stages=("dio",), vrm=29, frames=9001),
    # ---- CheapTrick: q1, transform size (512 lifts its F0 floor to 94 Hz: lower frames take the default F0)
    _case("ct_q1_-0.09_mcep", LJ, q1=-0.09, stages=STAGES[:3], mcep=(19, 0.58), vrm=7),
    _case("ct_q1_0", LJ, q1=0.0, stages=STAGES[:3], vrm=7),
    _case("ct_fft2048", LJ, fft_size=2048, stages=STAGES[:3], vrm=7),
    _case("ct_fft512", ("synthetic", 2.0, 3, 100.0), fft_size=512, stages=STAGES[:3], vrm=7),   # a voice around 100 Hz
    # ---- D4C: LoveTrain's threshold, transform size, the fused band aperiodicity
    _case("d4c_thr_0", LJ, threshold=0.0, stages=("dio", "stonemask", "d4c"), vrm=7),
    _case("d4c_thr_0.5_bap", LJ, threshold=0.5, stages=("dio", "stonemask", "d4c"), want_bap=True, vrm=7),
    _case("d4c_thr_1", LJ, threshold=1.0, stages=("dio", "stonemask", "d4c"), vrm=7),
    _case("d4c_fft2048", LJ, fft_size=2048, stages=("dio", "stonemask", "d4c"), vrm=7),
    # ---- a ragged batch: every utterance must equal the oracle run on it alone
    _case("ragged_fp_7.3", (LJ, ("synthetic", 0.05, 6), ("silence", 0.4)), 7.3, dio=RAGGED_DIO,
          voicing=("normal", "short", "silent"), mcep=(19, 0.58), want_bap=True, nb=10, vrm=5),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# itts_wav2world (DIO's defaults by its interface) at 10 ms with an explicit transform size, and the public surface
# (idiaptts_amd.world.analyse_batch, hop_ms = 10): the oracle figures are those of these cases
WAV2WORLD_CASE = "fp_10_fft2048"
PUBLIC_CASE = "fp_10"

# what the host checks refuse before any launch: (frame_period, f0_floor, f0_ceil, channels_in_octave)
REFUSED_DIO = [
    ("nb_20", 5.0, 40.0, 1100.0, 4.0),           # nb = 20 > MAXB
    ("frame_period_0", 0.0, 71.0, 800.0, 2.0),
    ("frame_period_negative", -5.0, 71.0, 800.0, 2.0),
    ("ceil_equals_floor", 5.0, 200.0, 200.0, 2.0),
    ("ceil_below_floor", 5.0, 300.0, 100.0, 2.0),
]


# ------------------------------------------------------------------------------------------ closed formulas
def dio_bands(f0_floor, f0_ceil, channels_in_octave):
    return 1 + int(math.log(f0_ceil / f0_floor) / math.log(2.0) * channels_in_octave)


def voice_range_minimum(frame_period, f0_floor):
    return int(0.5 + 1000.0 / frame_period / f0_floor) * 2 + 1


def num_frames(n, fs, frame_period):
    return int(1000.0 * n / fs / frame_period) + 1


def synth_length(T, fs, frame_period):
    return int(T * frame_period * fs / 1000)


def default_fft_size(fs):
    return 2 ** (1 + int(math.log2(3.0 * fs / 71.0 + 1)))


def fft_size_of(case):
    return case.fft_size or default_fft_size(case.fs)


# ------------------------------------------------------------------------------------------ signals
def read_fixture(name, pre=0.97):
    """tests/test_gpu_world.py's _read: the fixture behind the reference's pre-emphasis."""
    from scipy.io import wavfile
    fs, w = wavfile.read(os.path.join(GOLDEN, name + ".wav"))
    raw = w.astype(np.float64) / 32768.0
    return np.append(raw[0], raw[1:] - pre * raw[:-1]), fs


def synthetic(fs, n, seed, centre=150.0):
    """tests/test_gpu_world.py's _synthetic for n samples (its F0 walk starts at 150 Hz and stays in [90, 300])."""
    rng = np.random.default_rng(1234 + seed)
    f0 = np.clip(centre + np.cumsum(rng.normal(0, 0.02, n)) * 20, 0.6 * centre, 2.0 * centre)
    voiced = (np.sin(2 * np.pi * np.arange(n) / fs * 1.3 + seed) > -0.3).astype(float)
    phase = 2 * np.pi * np.cumsum(f0) / fs
    src = sum(np.sin(k * phase) / k for k in range(1, 12)) * voiced
    return 0.3 * src / np.abs(src).max() + 10 ** (-40 / 20) * rng.normal(size=n)


@functools.lru_cache(maxsize=None)
def _signal(fs, spec):
    kind = spec[0]
    if kind == "lj":
        x, fs_file = read_fixture("LJ001-0002")
        assert fs_file == fs
        x = x[:spec[1]].copy()
        assert len(x) == spec[1]
    elif kind == "synthetic":
        n = spec[1][1] if isinstance(spec[1], tuple) else int(fs * spec[1])
        x = synthetic(fs, n, *spec[2:])
    elif kind == "silence":
        x = np.zeros(int(fs * spec[1]))
    else:
        raise ValueError(spec)
    x.setflags(write=False)
    return x


def signals(case):
    return [_signal(case.fs, s) for s in case.signals]


def uses_fixture(case, u):
    return case.signals[u][0] == "lj"


# ------------------------------------------------------------------------------------------ the oracle
def _oracle_utt(case, x):
    from oracle import capi
    fs, fp, fft = case.fs, case.frame_period, fft_size_of(case)
    r = {}
    r["f0_dio"], r["tp"] = capi.dio(x, fs, fp, *case.dio)
    f0 = r["f0_dio"]
    if "stonemask" in case.stages:
        f0 = r["f0"] = capi.stonemask(x, fs, r["tp"], r["f0_dio"])
    if "cheaptrick" in case.stages:
        r["sp"] = capi.cheaptrick(x, fs, r["tp"], f0, fft, case.q1)
        if case.mcep:
            r["mc"], r["iters"] = capi.mcep(np.sqrt(r["sp"]), case.mcep[0], case.mcep[1], return_iters=True)
    if "d4c" in case.stages:
        r["ap"] = capi.d4c(x, fs, r["tp"], f0, fft, case.threshold)
        if case.want_bap:
            r["bap"] = capi.code_aperiodicity(r["ap"], fs)
    if "synth" in case.stages:
        r["y"] = capi.synthesize(f0, r["sp"], r["ap"], fs, fp)
    for v in r.values():
        v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """One dict of read-only f64 arrays per utterance of the case: f0_dio, tp, and by its stages f0, sp, mc, iters, ap,
    bap, y (the synthesis of the oracle's own f0 / sp / ap, before the float32 cast and any de-emphasis)."""
    case = BY_NAME[name]
    return tuple(_oracle_utt(case, x) for x in signals(case))


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64).tolist()
