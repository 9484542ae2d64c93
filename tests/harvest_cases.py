"""The case table of tests/test_gpu_harvest_branches.py (tests/test_harvest_cases.py proves on the CPU, with the
branch counters of oracle/c/harvest.c, that the table reaches what it claims).

Harvest's contour fixing (FixF0Contour steps 1-4, SmoothF0Contour) is sequential and branchy; smooth voices take few
of its branches.  The signals here are short harmonic bursts over a noise floor: sections that ExtendSub rejects
(2200 / mean >= ed - st: short and low), selected sections behind rejected ones (real swaps), sections that grow into
each other (MergeF0's overlap branches) and sorted orders that differ from the identity.  Every generator is seeded
numpy; nothing is read from a file.

Margins (test_harvest_cases.py): the oracle and the kernels agree to rounding, not bit for bit, so a case is only
usable if none of its thresholded decisions sits on its threshold.  Decisions on F0 values (FixStep1's two 0.008
tests, SelectBestF0's 0.18 test inside Extend, ExtendSub's 2200 / mean against ed - st) keep F0_MARGIN = 1e-6 from
the threshold, 100 times the 1e-8 that the GPU tests allow on the candidates; MergeF0Sub's score sums keep
SCORE_MARGIN = 1e-4, 100 times the 1e-6 allowed on the scores, or are exact ties (both contours hold the same
candidates in the overlap, so both sums add the same numbers in the same order).  The two 0.008 tests and the 0.18
test are measured as the absolute distance of the relative F0 deviation from the threshold -- the quantity a
relative error of the candidates moves one to one -- which is stricter than the distance relative to the threshold.
A seed that misses a floor is replaced by another seed; the floors stay.

The exact score tie is reached (case "islands": two sections extend through the same candidates), so no row of
the table is left out.

What reaching a branch is worth was checked once with deliberately wrong copies of the oracle's contour code: the
1 ms contour of at least one case changes when ExtendSub's mean is not carried ("carried_mean"), when the selected
channels are read without the swaps (eight cases), when MergeF0 starts from the first channel of the sorted order
instead of channel 0 (three cases), when count == 0 does not fall back to step 2, when Extend allows 99 frames or 5
misses, when FixStep2 asks for 7 frames or FixStep4 for 8.  Three wrong versions change no contour here: s1 >= s2
for s1 > s2 (the ties found hold the same values on both sides), the earlier instead of the later of two equally
near candidates in SelectBestF0 (such candidates are copies of one value from neighbouring frames), and reading
channel 0's first boundaries instead of the rewritten boundary[0..1] when channel 0 comes later in the order (in each
of the 66 seeds found that reach the branch, the merge is a contained no-op either way)."""
import collections
import functools

import numpy as np

F0_MARGIN = 1e-6
SCORE_MARGIN = 1e-4
F0_MARGIN_KEYS = ("step1_slope", "step1_previous", "extend_select", "sub_length")
SCORE_MARGIN_KEYS = ("merge_score",)

# every decision of the contour code that the table must reach between its cases
BRANCHES = (
    "step2_removes_short_section",
    "extend_stops_after_4_misses", "extend_runs_100_frames", "extend_cut_by_contour_end",
    "extend_meets_contour_start", "extend_meets_contour_finish",
    "sub_rejects_section", "sub_real_swap", "sub_selects_nothing", "sub_first_rejected_later_selected",
    "sub_carried_mean_decides",
    "merge_disjoint", "merge_contained", "merge_overlap_first_wins", "merge_overlap_second_wins",
    "merge_order_not_identity", "merge_channel0_later_in_order", "merge_channel0_after_rewrite",
    "merge_score_tie",
    "step4_bridges_gap", "smooth_more_than_3_sections",
)
SIZES = ("sections", "selected_sections", "smooth_sections")

# sections entering FixStep3 are >= 7 frames long and >= 1 frame apart: the kernels size their section store for
# T1 / 8 of them.  The smoothing kernel walks its sections one after another in one wave: a stated cap keeps a
# replaced seed from making that test slow (sections there are >= 10 frames apart, FixStep4 bridges shorter gaps)
MAX_SMOOTH_SECTIONS = 12


def max_sections(T1):
    return T1 // 8


def _tone(rng, fs, n, f0, harmonics, ramp_ms=3.0):
    t = np.arange(n) / fs
    x = sum(np.sin(2 * np.pi * k * f0 * t + rng.uniform(0, 2 * np.pi)) / k for k in range(1, harmonics + 1))
    ramp = min(int(fs * ramp_ms / 1000.0), n // 2)
    if ramp > 0:
        w = 0.5 - 0.5 * np.cos(np.pi * (np.arange(ramp) + 0.5) / ramp)
        x[:ramp] *= w
        x[n - ramp:] *= w[::-1]
    return 0.3 * x / np.abs(x).max()


def bursts(seed, fs, n, f_range, dur_ms, gap_ms, floor_db=-70.0, harmonics=5, lead_ms=None):
    """harmonic bursts of dur_ms at a pitch from f_range, gap_ms apart, over a noise floor"""
    rng = np.random.default_rng(seed)
    x = 10.0 ** (floor_db / 20.0) * rng.normal(size=n)
    at = int(fs * (rng.uniform(*gap_ms) if lead_ms is None else lead_ms) / 1000.0)
    while at < n:
        m = min(int(fs * rng.uniform(*dur_ms) / 1000.0), n - at)
        if m >= 8:
            x[at:at + m] += _tone(rng, fs, m, rng.uniform(*f_range), harmonics)
        at += m + int(fs * rng.uniform(*gap_ms) / 1000.0)
    return x


def mixed_bursts(seed, fs, n, f_range, short_ms, long_ms, gap_ms, floor_db=-70.0, harmonics=5):
    """a short burst (a section ExtendSub rejects) before every long one (a section it selects: a real swap)"""
    rng = np.random.default_rng(seed)
    x = 10.0 ** (floor_db / 20.0) * rng.normal(size=n)
    at = int(fs * rng.uniform(*gap_ms) / 1000.0)
    k = 0
    while at < n:
        m = min(int(fs * rng.uniform(*(short_ms if k % 2 == 0 else long_ms)) / 1000.0), n - at)
        if m >= 8:
            x[at:at + m] += _tone(rng, fs, m, rng.uniform(*f_range), harmonics)
        at += m + int(fs * rng.uniform(*gap_ms) / 1000.0)
        k += 1
    return x


def edge_voice(seed, fs, n, f_range, floor_db=-60.0, harmonics=6):
    """one voice with a slow glide that is already running in the first sample and still running in the last"""
    rng = np.random.default_rng(seed)
    f0 = np.linspace(rng.uniform(*f_range), rng.uniform(*f_range), n)
    phase = 2 * np.pi * np.cumsum(f0) / fs + rng.uniform(0, 2 * np.pi)
    x = sum(np.sin(k * phase) / k for k in range(1, harmonics + 1))
    return 0.3 * x / np.abs(x).max() + 10.0 ** (floor_db / 20.0) * rng.normal(size=n)


# name, generator(seed, fs, n, **kwargs), its keyword arguments, seed, sampling rate, samples, frame period (ms),
# F0 range, the branch names the case claims
Case = collections.namedtuple("Case", "name gen kwargs seed fs n frame_period f0_floor f0_ceil claims")


def _case(name, gen, seed, n, claims, fs=16000, frame_period=5.0, f0_floor=71.0, f0_ceil=800.0, **kwargs):
    assert set(claims) <= set(BRANCHES), set(claims) - set(BRANCHES)
    return Case(name, gen, tuple(sorted(kwargs.items())), seed, fs, n, frame_period, f0_floor, f0_ceil,
                tuple(claims))


_COMMON = ("step2_removes_short_section", "extend_stops_after_4_misses")

CASES = [
    # 14 sections; ExtendSub rejects section 0, so every one of the 13 selected channels sits one index below its
    # section (ord[k] = k + 1); T1 = 1000
    _case("first_rejected", bursts, 39, 15985,
          _COMMON + ("sub_rejects_section", "sub_real_swap", "sub_first_rejected_later_selected", "merge_disjoint",
                     "merge_contained", "step4_bridges_gap", "smooth_more_than_3_sections"),
          f_range=(72.0, 95.0), dur_ms=(20.0, 45.0), gap_ms=(25.0, 70.0)),
    # the only section is rejected: count == 0, the contour falls back to step 2; T1 = 501
    _case("nothing_selected", bursts, 33, 8000, _COMMON + ("sub_rejects_section", "sub_selects_nothing"),
          f_range=(72.0, 85.0), dur_ms=(12.0, 22.0), gap_ms=(80.0, 160.0)),
    # 24 sections, 20 real swaps, a sorted order that brings channel 0 back later, both overlap branches, extensions
    # of 100 frames and extensions that meet either end of the contour
    _case("many_swaps", mixed_bursts, 148, 15985,
          _COMMON + ("extend_runs_100_frames", "extend_cut_by_contour_end", "extend_meets_contour_start",
                     "extend_meets_contour_finish", "sub_rejects_section", "sub_real_swap", "merge_disjoint",
                     "merge_contained", "merge_overlap_first_wins", "merge_overlap_second_wins",
                     "merge_order_not_identity", "merge_channel0_later_in_order", "step4_bridges_gap",
                     "smooth_more_than_3_sections"),
          f_range=(100.0, 250.0), short_ms=(10.0, 20.0), long_ms=(40.0, 80.0), gap_ms=(10.0, 40.0)),
    # channel 0 later in the order while ord is not the identity (one rejected section, four swaps)
    _case("channel0_later", mixed_bursts, 199, 15985,
          _COMMON + ("extend_runs_100_frames", "extend_meets_contour_start", "sub_rejects_section", "sub_real_swap",
                     "merge_overlap_first_wins", "merge_overlap_second_wins", "merge_order_not_identity",
                     "merge_channel0_later_in_order", "step4_bridges_gap", "smooth_more_than_3_sections"),
          f_range=(150.0, 300.0), short_ms=(8.0, 14.0), long_ms=(30.0, 50.0), gap_ms=(30.0, 60.0)),
    # 23 sections, 16 swaps; channel 0 comes third in the sorted order, after MergeF0 has rewritten boundary[0..1]
    _case("channel0_after_rewrite", bursts, 342, 15985,
          _COMMON + ("extend_runs_100_frames", "extend_meets_contour_start", "extend_meets_contour_finish",
                     "sub_rejects_section", "sub_real_swap", "merge_disjoint", "merge_contained",
                     "merge_overlap_first_wins", "merge_overlap_second_wins", "merge_order_not_identity",
                     "merge_channel0_later_in_order", "merge_channel0_after_rewrite", "step4_bridges_gap"),
          f_range=(120.0, 300.0), dur_ms=(25.0, 60.0), gap_ms=(10.0, 40.0)),
    # ExtendSub's mean carried over from the section before decides a section the other way than the section's own
    # mean would, and the contour shows it (25 frames)
    _case("carried_mean", bursts, 119, 15985,
          _COMMON + ("sub_rejects_section", "sub_real_swap", "sub_carried_mean_decides", "merge_disjoint",
                     "merge_overlap_second_wins"),
          f_range=(72.0, 95.0), dur_ms=(20.0, 45.0), gap_ms=(25.0, 70.0)),
    # islands of 70-110 ms at 250-400 Hz: two exact score ties, five sections in the smoothing call
    _case("islands", bursts, 3, 15985,
          _COMMON + ("extend_runs_100_frames", "merge_contained", "merge_overlap_first_wins",
                     "merge_overlap_second_wins", "merge_score_tie", "step4_bridges_gap",
                     "smooth_more_than_3_sections"),
          f_range=(250.0, 400.0), dur_ms=(70.0, 110.0), gap_ms=(90.0, 130.0), lead_ms=40.0),
    # sparse bursts: T1 = 701
    _case("sparse", bursts, 1, 11200, _COMMON + ("merge_disjoint", "merge_contained", "step4_bridges_gap"),
          f_range=(72.0, 95.0), dur_ms=(20.0, 40.0), gap_ms=(50.0, 150.0)),
    # one voice from the first sample to the last: the contour is voiced in frame 1 and in frame T1 - 2, and both
    # extensions run into the end of the contour; T1 = 402
    _case("edge_voice", edge_voice, 0, 6417,
          ("extend_cut_by_contour_end", "extend_meets_contour_start", "extend_meets_contour_finish"),
          f_range=(110.0, 220.0)),
    # a frame period that is no whole number of 1 ms frames
    _case("frame_period_2p5", bursts, 15, 12008,
          _COMMON + ("sub_rejects_section", "sub_real_swap", "sub_first_rejected_later_selected", "merge_disjoint"),
          frame_period=2.5, f_range=(72.0, 95.0), dur_ms=(20.0, 40.0), gap_ms=(50.0, 150.0)),
    # 44.1 kHz: decimation by 6 to 7350 Hz
    _case("rate_44k1", bursts, 12, 30870,
          _COMMON + ("extend_meets_contour_finish", "sub_rejects_section", "sub_real_swap",
                     "sub_first_rejected_later_selected", "merge_disjoint"),
          fs=44100, f_range=(72.0, 95.0), dur_ms=(20.0, 40.0), gap_ms=(50.0, 150.0)),
    # another channel count and longer refinement windows
    _case("low_range", bursts, 14, 11200,
          _COMMON + ("sub_rejects_section", "sub_real_swap", "sub_first_rejected_later_selected", "merge_contained",
                     "merge_overlap_second_wins"),
          f0_floor=40.0, f0_ceil=400.0, f_range=(42.0, 70.0), dur_ms=(30.0, 60.0), gap_ms=(50.0, 150.0)),
]

# what the issue names beyond the table's rows, as (case, minimum of a counter) pairs
REQUIRED = (
    ("first_rejected", "sub_first_rejected_later_selected", 1),
    ("nothing_selected", "sub_selects_nothing", 1),
    ("nothing_selected", "sections", 1),
    ("many_swaps", "sections", 8),
    ("many_swaps", "sub_real_swap", 3),
    ("channel0_later", "merge_channel0_later_in_order", 1),
    ("channel0_later", "sub_real_swap", 1),
    ("channel0_after_rewrite", "merge_channel0_after_rewrite", 1),
    ("channel0_after_rewrite", "sub_real_swap", 3),
    ("channel0_after_rewrite", "sections", 8),
    ("carried_mean", "sub_carried_mean_decides", 1),
    ("edge_voice", "extend_meets_contour_start", 1),
    ("edge_voice", "extend_meets_contour_finish", 1),
)

ALL_CASES = {c.name: c for c in CASES}


def signal(case):
    return case.gen(case.seed, case.fs, case.n, **dict(case.kwargs))


def num_frames_1ms(case):
    return int(1000.0 * case.n / case.fs) + 1


def group_key(case):
    return (case.fs, case.frame_period, case.f0_floor, case.f0_ceil)


def groups():
    """the cases of one (fs, frame period, F0 range) in table order: one ragged batch each"""
    out = collections.OrderedDict()
    for c in CASES:
        out.setdefault(group_key(c), []).append(c)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(signal, f0, stages incl. branches and margins) of a case from oracle/c/harvest.c, computed once"""
    from oracle import capi
    c = ALL_CASES[name]
    x = signal(c)
    f0, _, ref = capi.harvest(x, c.fs, c.frame_period, f0_floor=c.f0_floor, f0_ceil=c.f0_ceil, debug=True)
    for a in (x, f0, ref["raw"], ref["cand"], ref["score"], ref["best"]):
        a.setflags(write=False)
    return x, f0, ref
