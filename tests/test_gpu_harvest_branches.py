"""The contour kernels of Harvest (hv_contour1 / hv_extend / hv_contour2 / hv_smooth in csrc/harvest.hip) on inputs
that take every branch of FixF0Contour and SmoothF0Contour: the case table of tests/harvest_cases.py, whose reach
tests/test_harvest_cases.py proves on the CPU with the branch counters of oracle/c/harvest.c.  Every stage is compared
with the oracle under the bounds tests/test_gpu_harvest.py uses on the fixture audio; the ragged batches cover the
per-utterance offsets of the contour scratch; the refusals of the entry point are checked by name.

Worst ratio |gpu / oracle - 1| per stage over the 12 cases, measured on an MI355X (bounds in brackets), with the
voicing pattern identical at every stage:
    raw 3.1e-10 (1e-9)   cand 8.3e-13 (1e-8)   score 9.0e-9 (1e-6)   best 1.2e-13 (1e-8)   f0 2.6e-14 (1e-8)
    ragged batches: f0 2.6e-14 (1e-7), every utterance bit for bit the same as its single call
    the 12-channel range: f0 3.6e-15 (1e-7)
No case failed: the contour kernels take every branch of the table as the oracle does."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import harvest_cases as hc  # noqa: E402
from test_gpu_harvest import _close, _run  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in hc.CASES]
STAGE_BOUNDS = (("raw", 1e-9), ("cand", 1e-8), ("score", 1e-6), ("best", 1e-8), ("f0", 1e-8))
BATCH_BOUND = 1e-7

_single = {}


def _kw(case):
    return dict(f0_floor=case.f0_floor, f0_ceil=case.f0_ceil)


def _single_f0(gpu, case):
    """the F0 of a call with this utterance alone (no stage outputs), once per case"""
    if case.name not in _single:
        f0, _ = _run(gpu, [hc.oracle(case.name)[0]], case.fs, case.frame_period, **_kw(case))
        _single[case.name] = f0.clone()
    return _single[case.name]


def _worst(a, b):
    """largest |a / b - 1| where both are voiced (the voicing pattern itself is _close's to judge)"""
    m = (a > 0) & (b > 0)
    return float(np.abs(a[m] / b[m] - 1).max()) if m.any() else 0.0


@pytest.mark.parametrize("name", NAMES)
def test_every_stage_matches_the_oracle(gpu, name):
    c = hc.ALL_CASES[name]
    x, f0_ref, ref = hc.oracle(name)
    (f0, dbg), _ = _run(gpu, [x], c.fs, c.frame_period, stages=True, **_kw(c))
    nc = ref["n_cand"]
    got = dict(raw=dbg["raw"].cpu().numpy(), cand=dbg["cand"].cpu().numpy()[:, :nc],
               score=dbg["score"].cpu().numpy()[:, :nc], best=dbg["best"].cpu().numpy(), f0=f0.cpu().numpy())
    want = dict(raw=ref["raw"], cand=ref["cand"][:, :nc], score=ref["score"][:, :nc], best=ref["best"], f0=f0_ref)
    print(json.dumps(dict(case=name, **{k: _worst(got[k], want[k]) for k, _ in STAGE_BOUNDS})))
    assert (dbg["cand"].cpu().numpy()[:, nc:] == 0).all() and (dbg["score"].cpu().numpy()[:, nc:] == 0).all()
    for stage, bound in STAGE_BOUNDS:
        try:
            _close(got[stage], want[stage], bound)      # the voicing pattern exactly, voiced values within the bound
        except AssertionError as e:
            raise AssertionError("{}: stage {}: {}".format(name, stage, e))
    assert len(got["f0"]) == hc.oracle(name)[1].shape[0]
    # the stage outputs change nothing: the same utterance without them gives the same F0, bit for bit
    assert torch.equal(f0, _single_f0(gpu, c))


@pytest.mark.parametrize("reverse", [False, True], ids=["table_order", "reversed"])
@pytest.mark.parametrize("key", list(hc.groups()), ids=lambda k: "fs{}_fp{}_f0_{:g}_{:g}".format(*k))
def test_ragged_batch_equals_single_calls_and_the_oracle(gpu, key, reverse):
    cases = hc.groups()[key]
    cases = cases[::-1] if reverse else cases
    fs, fp = key[0], key[1]
    f0, f_off = _run(gpu, [hc.oracle(c.name)[0] for c in cases], fs, fp, **_kw(cases[0]))
    worst = {}
    for u, c in enumerate(cases):
        mine = f0[f_off[u]:f_off[u + 1]]
        assert torch.equal(mine, _single_f0(gpu, c)), c.name
        worst[c.name] = _worst(mine.cpu().numpy(), hc.oracle(c.name)[1])
    print(json.dumps(dict(batch=list(key), reverse=reverse, f0=worst)))
    for u, c in enumerate(cases):
        _close(f0[f_off[u]:f_off[u + 1]].cpu().numpy(), hc.oracle(c.name)[1], BATCH_BOUND)


def test_the_narrowest_f0_range_runs_on_its_12_channels(gpu):
    """1.1 / 0.9 of any f0_ceil > f0_floor already spans 11.6 of the 40 channels per octave, so 12 channels is the
    least a valid range gives: the refusal below 12 cannot be reached through a range, and the 12 themselves (one
    partly filled tile of 16, 7 candidate slots) must work"""
    from oracle import capi
    fs, lo, hi = 16000, 100.0, 100.5
    x = hc.edge_voice(1, fs, 6400, (100.2, 100.2))
    ref, _, stages = capi.harvest(x, fs, f0_floor=lo, f0_ceil=hi, debug=True)
    assert stages["raw"].shape[0] == 12 and (ref > 0).sum() > 50
    f0, _ = _run(gpu, [x], fs, f0_floor=lo, f0_ceil=hi)
    print(json.dumps(dict(case="12_channels", f0=_worst(f0.cpu().numpy(), ref))))
    _close(f0.cpu().numpy(), ref, BATCH_BOUND)


def _used():
    from idiaptts_amd import lib as _lib
    L = _lib.load()
    r, u, k = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _lib.check(L.itts_scratch_pool_stats(ctypes.byref(r), ctypes.byref(u), ctypes.byref(k)), "stats")
    return u.value


# what is refused, the sampling rate, the samples, frame period, F0 range, and what the error says
REFUSALS = [
    ("floor_equals_ceil", 16000, 16000, 5.0, 200.0, 200.0, "need 0 < f0_floor < f0_ceil"),
    ("floor_above_ceil", 16000, 16000, 5.0, 800.0, 71.0, "need 0 < f0_floor < f0_ceil"),
    # below 12 channels: only f0_ceil <= f0_floor * 0.99 gives that, which the range check turns away first
    ("fewer_than_12_channels", 16000, 16000, 5.0, 100.0, 98.0, "need 0 < f0_floor < f0_ceil"),
    ("more_than_512_channels", 16000, 16000, 5.0, 1.0, 8000.0, "unsupported number of channels"),      # 531
    ("floor_too_low_at_48k", 48000, 48000, 5.0, 10.0, 800.0, "f0_floor too low for the refinement window"),
    ("frame_period_zero", 16000, 16000, 0.0, 71.0, 800.0, "fs and frame_period_ms must be positive"),
    ("frame_period_negative", 16000, 16000, -5.0, 71.0, 800.0, "fs and frame_period_ms must be positive"),
    # 6 samples at 16 kHz decimate by 2 to 3; found after the first scratch blocks have been taken
    ("fewer_than_4_decimated_samples", 16000, 6, 5.0, 71.0, 800.0, "utterance too short"),
]


@pytest.mark.parametrize("what,fs,n,fp,lo,hi,says", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_by_name_hand_their_scratch_back(gpu, what, fs, n, fp, lo, hi, says):
    from idiaptts_amd import lib as _lib, ops
    good = torch.from_numpy(np.random.default_rng(0).normal(size=16000) * 0.1).to(gpu)
    T_good = ops.harvest_num_frames(16000, 16000)
    ops.harvest(good, [0, 16000], [0, T_good], 16000)        # a good call: the pool holds what a call needs
    torch.cuda.synchronize()
    base = _used()
    x = torch.from_numpy(np.random.default_rng(1).normal(size=n) * 0.1).to(gpu)
    T = ops.harvest_num_frames(n, fs, fp if fp > 0 else 5.0)
    for _ in range(3):
        with pytest.raises(_lib.IttsError, match=says):
            ops.harvest(x, [0, n], [0, T], fs, fp, f0_floor=lo, f0_ceil=hi)
    torch.cuda.synchronize()
    assert _used() == base
    f0 = ops.harvest(good, [0, 16000], [0, T_good], 16000)   # and the library still works
    assert f0.shape[0] == T_good
