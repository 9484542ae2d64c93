"""The case table of tests/harvest_cases.py reaches what it claims: every case runs through oracle/c/harvest.c, whose
contour code counts the branches it takes and records how close each thresholded decision comes to its threshold.
No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import harvest_cases as hc  # noqa: E402

NAMES = [c.name for c in hc.CASES]


def test_case_names_are_unique_and_signals_short():
    assert len(hc.ALL_CASES) == len(hc.CASES)
    for c in hc.CASES:
        assert hc.num_frames_1ms(c) <= 1000 and c.n / c.fs <= 1.0, c.name
        x = hc.signal(c)
        assert x.shape == (c.n,) and np.isfinite(x).all() and np.abs(x).max() < 1.0, c.name
        assert np.array_equal(x, hc.signal(c)), c.name                       # seeded: the same signal every time


def test_the_counters_name_every_row_and_start_from_zero():
    from oracle import capi
    _, _, ref = capi.harvest(np.zeros(1600), 16000, debug=True)
    assert set(ref["branches"]) == set(hc.BRANCHES) | set(hc.SIZES)
    assert all(v == 0 for v in ref["branches"].values())                     # silence decides nothing ...
    assert set(ref["margins"]) == set(hc.F0_MARGIN_KEYS) | set(hc.SCORE_MARGIN_KEYS)
    assert all(math.isinf(v) for v in ref["margins"].values())               # ... and a call resets what the last left
    hc.oracle("many_swaps")
    _, _, again = capi.harvest(np.zeros(1600), 16000, debug=True)
    assert again["branches"] == ref["branches"] and again["margins"] == ref["margins"]


@pytest.mark.parametrize("name", NAMES)
def test_every_claimed_branch_is_taken(name):
    c = hc.ALL_CASES[name]
    _, f0, ref = hc.oracle(name)
    b = ref["branches"]
    print(name, {k: v for k, v in b.items() if v})
    for claim in c.claims:
        assert b[claim] > 0, (name, claim)
    T1 = hc.num_frames_1ms(c)
    assert len(ref["best"]) == T1
    assert b["sections"] <= hc.max_sections(T1), name
    assert b["selected_sections"] <= b["sections"], name
    assert b["smooth_sections"] <= hc.MAX_SMOOTH_SECTIONS, name
    assert (b["smooth_more_than_3_sections"] > 0) == (b["smooth_sections"] > 3), name
    assert (f0 > 0).any(), name                                              # every case leaves something voiced


@pytest.mark.parametrize("name", NAMES)
def test_no_decision_sits_on_its_threshold(name):
    _, _, ref = hc.oracle(name)
    m = ref["margins"]
    print(name, m, "ties", ref["branches"]["merge_score_tie"])
    for k in hc.F0_MARGIN_KEYS:
        assert m[k] >= hc.F0_MARGIN, (name, k, m[k])
    for k in hc.SCORE_MARGIN_KEYS:                                           # exact ties are counted, not measured
        assert m[k] >= hc.SCORE_MARGIN, (name, k, m[k])


def test_the_union_of_the_claims_is_the_full_list():
    claimed = set()
    for c in hc.CASES:
        claimed.update(c.claims)
    assert claimed == set(hc.BRANCHES), set(hc.BRANCHES) - claimed


def test_the_cases_the_table_must_include():
    for name, key, least in hc.REQUIRED:
        assert hc.oracle(name)[2]["branches"][key] >= least, (name, key)
    # count == 0 while sections exist
    b = hc.oracle("nothing_selected")[2]["branches"]
    assert b["selected_sections"] == 0 and b["sections"] > 0
    # a voiced run from frame 1 and one up to frame T1 - 2: the extension meets the contour end on both sides
    best = hc.oracle("edge_voice")[2]["best"]
    assert best[1] > 0 and best[len(best) - 2] > 0
    # parameters
    by = hc.ALL_CASES
    assert by["frame_period_2p5"].frame_period == 2.5 and by["rate_44k1"].fs == 44100
    assert (by["low_range"].f0_floor, by["low_range"].f0_ceil) == (40.0, 400.0)
    for name in ("frame_period_2p5", "rate_44k1", "low_range"):              # and each takes the ord indirection
        assert hc.oracle(name)[2]["branches"]["sub_real_swap"] > 0, name
    # the ragged batch of the default parameters holds odd and even frame counts (the contour scratch packs its
    # int arrays behind the double arrays) and more than one utterance
    main = hc.groups()[(16000, 5.0, 71.0, 800.0)]
    assert len(main) >= 6
    assert {hc.num_frames_1ms(c) % 2 for c in main} == {0, 1}
    assert len(hc.groups()) == 4
