"""CPU-side checks of MLPG's choice of form (itts_mlpg_choose_form, the function the dispatcher itself calls): every
threshold pinned on both sides, every override and its fallbacks, the benchmark's shapes.  No device is touched."""
import ctypes
import os
import subprocess
import sys
import threading

import pytest

from idiaptts_amd import lib, ops
from idiaptts_amd.ops import (MLPG_F32_ROWS, MLPG_NT_IN, MLPG_RING, MLPG_STREAM, MLPG_SWEEPS, MLPG_WIDE,
                              MLPG_WIDENED_COPY)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = MLPG_F32_ROWS | MLPG_WIDENED_COPY          # float32 rows of the forms that read a widened copy
MIB192 = 192 << 20


@pytest.fixture(autouse=True)
def auto():
    """Every test starts from the library's own choice (whatever the environment seeded) and leaves the override
    as it found it."""
    with ops.mlpg_forced():
        yield


def choose(n_utts, dim, t_max, t_total=None, f32=False):
    return ops.mlpg_choose_form(n_utts, dim, t_max, n_utts * t_max if t_total is None else t_total, f32)


def test_header_constants_match_python():
    text = open(os.path.join(ROOT, "include", "idiaptts_amd.h")).read()
    for name, value in (("SWEEPS", MLPG_SWEEPS), ("STREAM", MLPG_STREAM), ("RING", MLPG_RING), ("WIDE", MLPG_WIDE),
                        ("F32_ROWS", MLPG_F32_ROWS), ("NT_IN", MLPG_NT_IN), ("WIDENED_COPY", MLPG_WIDENED_COPY)):
        assert "#define ITTS_MLPG_FORM_%s %d\n" % (name, value) in text, name


def test_sweeps_below_194_frames():
    for f32 in (False, True):
        extra = F32 if f32 else 0
        for n_utts, dim in ((1, 1), (256, 62), (4096, 62), (70000, 3)):
            assert choose(n_utts, dim, 193, f32=f32) == MLPG_SWEEPS | extra
            assert choose(n_utts, dim, 0, 0, f32=f32) == MLPG_SWEEPS | extra
        assert choose(256, 62, 194, f32=f32) & 3 == MLPG_RING
        assert choose(8, 62, 194, f32=f32) == MLPG_STREAM | extra


@pytest.mark.parametrize("dim", [1, 62, 64, 65, 128, 129, 130])
def test_ring_from_128_units(dim):
    """(utterance, 64-dimension block) units: 127 or fewer take the stream form, 128 and more the ring; dim 64 / 65 /
    129 are one, two and three blocks."""
    blocks = (dim + 63) // 64
    first = -(-128 // blocks)                     # fewest utterances with >= 128 units
    assert (first - 1) * blocks <= 127 < first * blocks
    for t_max in (194, 2000):
        assert choose(first - 1, dim, t_max) == MLPG_STREAM
        assert choose(first, dim, t_max) & 3 == MLPG_RING
        assert choose(first - 1, dim, t_max, f32=True) == MLPG_STREAM | F32
        assert choose(first, dim, t_max, f32=True) & 3 == MLPG_RING


def test_units_at_127_and_128_exactly():
    assert choose(127, 64, 500) == MLPG_STREAM
    assert choose(128, 64, 500) == MLPG_RING | MLPG_NT_IN
    assert choose(63, 65, 500) == MLPG_STREAM           # 126 units
    assert choose(64, 65, 500) == MLPG_RING | MLPG_NT_IN
    assert choose(42, 129, 500) == MLPG_STREAM          # 126 units
    assert choose(43, 129, 500) == MLPG_RING | MLPG_NT_IN


def test_more_than_65535_utterances_take_the_stream_form():
    assert choose(65535, 1, 194) == MLPG_RING | MLPG_NT_IN
    assert choose(65536, 1, 194) == MLPG_STREAM
    assert choose(65535, 2, 194, f32=True) == MLPG_RING | MLPG_F32_ROWS | MLPG_WIDE
    assert choose(65536, 2, 194, f32=True) == MLPG_STREAM | F32
    with ops.mlpg_forced(solve="ring"):
        assert choose(65535, 1, 194) == MLPG_RING | MLPG_NT_IN
        assert choose(65536, 1, 194) == MLPG_STREAM


@pytest.mark.parametrize("dim,per_1023,per_1024", [(62, 1023, 1024), (2, 1023, 1024), (130, 341, 342)])
def test_float32_rows_wide_from_1024_units_even_dim(dim, per_1023, per_1024):
    """(130 dimensions are three blocks: 341 utterances 1 023 units, 342 1 026)"""
    ring32 = MLPG_RING | MLPG_F32_ROWS
    assert choose(per_1023, dim, 300, f32=True) == ring32
    assert choose(per_1024, dim, 300, f32=True) == ring32 | MLPG_WIDE
    assert choose(per_1024, dim + 1, 300, f32=True) == ring32          # odd dim: narrow however many units
    assert choose(per_1024 * 4, dim + 1, 300, f32=True) == ring32
    assert choose(per_1024, dim, 300) == MLPG_RING | MLPG_NT_IN         # float64 rows: narrow
    assert choose(4 * per_1024, dim, 300) & MLPG_WIDE == 0


@pytest.mark.parametrize("dim", [62, 64, 1, 187])
def test_nt_in_up_to_192_mib_of_rows(dim):
    frames = MIB192 // (8 * dim)                 # the most frames with t_total * dim * 8 <= 192 MiB
    assert frames * dim * 8 <= MIB192 < (frames + 1) * dim * 8
    n = 256 if dim < 65 else 128
    assert choose(n, dim, 2000, frames) == MLPG_RING | MLPG_NT_IN
    assert choose(n, dim, 2000, frames + 1) == MLPG_RING
    assert choose(n, dim, 2000, frames, f32=True) & MLPG_NT_IN == 0


def test_nt_in_at_exactly_192_mib():
    assert 393216 * 64 * 8 == MIB192
    assert choose(256, 64, 2000, 393216) == MLPG_RING | MLPG_NT_IN
    assert choose(256, 64, 2000, 393217) == MLPG_RING


def test_bench_shapes():
    """bench.py's MLPG batch (256 utterances of 2 - 10 s, 62 dimensions) and its 4 096-utterance point."""
    from idiaptts_amd.bench_support import utterance_lengths
    for n_utts, f64_form, f32_form in ((256, MLPG_RING | MLPG_NT_IN, MLPG_RING | MLPG_F32_ROWS),
                                       (1024, MLPG_RING, MLPG_RING | MLPG_F32_ROWS | MLPG_WIDE),
                                       (4096, MLPG_RING, MLPG_RING | MLPG_F32_ROWS | MLPG_WIDE)):
        lens = utterance_lengths(n_utts, seed=5)
        t_max, t_total = int(lens.max()), int(lens.sum())
        assert choose(n_utts, 62, t_max, t_total) == f64_form, n_utts
        assert choose(n_utts, 62, t_max, t_total, f32=True) == f32_form, n_utts


def test_forced_solve():
    with ops.mlpg_forced(solve="stream"):
        assert choose(256, 62, 2000) == MLPG_STREAM
        assert choose(4096, 62, 2000, f32=True) == MLPG_STREAM | F32
        assert choose(256, 62, 193) == MLPG_SWEEPS                     # short batches keep the sweeps
    with ops.mlpg_forced(solve="ring"):
        assert choose(1, 1, 194) == MLPG_RING | MLPG_NT_IN
        assert choose(1, 1, 194, f32=True) == MLPG_RING | MLPG_F32_ROWS
        assert choose(3, 62, 193) == MLPG_SWEEPS
        assert choose(3, 62, 193, f32=True) == MLPG_SWEEPS | F32
    assert choose(1, 1, 194) == MLPG_STREAM                            # restored


def test_forced_width():
    with ops.mlpg_forced(solve="ring", width="wide"):
        assert choose(3, 62, 300) == MLPG_RING | MLPG_WIDE                # float64 wide: no non-temporal variant
        assert choose(3, 62, 300, f32=True) == MLPG_RING | MLPG_F32_ROWS | MLPG_WIDE
        assert choose(3, 63, 300) == MLPG_RING | MLPG_NT_IN               # odd dim: narrow
        assert choose(3, 1, 300, f32=True) == MLPG_RING | MLPG_F32_ROWS
        assert choose(3, 62, 150) == MLPG_SWEEPS
    with ops.mlpg_forced(width="narrow"):
        assert choose(4096, 62, 300, f32=True) == MLPG_RING | MLPG_F32_ROWS
        assert choose(8, 62, 300) == MLPG_STREAM                           # width does not move the solve
    with ops.mlpg_forced(width="wide"):
        assert choose(8, 62, 300) == MLPG_STREAM


def test_forced_nt():
    big = MIB192 // (8 * 62) + 1
    with ops.mlpg_forced(nt=False):
        assert choose(256, 62, 2000, 2000) == MLPG_RING
    with ops.mlpg_forced(nt=True):
        assert choose(256, 62, 2000, big) == MLPG_RING | MLPG_NT_IN
        assert choose(256, 62, 2000, big, f32=True) == MLPG_RING | MLPG_F32_ROWS
        assert choose(8, 62, 2000) == MLPG_STREAM
    with ops.mlpg_forced(solve="ring", width="wide", nt=True):
        assert choose(3, 62, 300) == MLPG_RING | MLPG_WIDE
    with ops.mlpg_forced(solve="ring", width="narrow", nt=False):
        assert choose(3, 62, 300) == MLPG_RING
        assert choose(3, 62, 300, f32=True) == MLPG_RING | MLPG_F32_ROWS


def _override():
    vals = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int()]
    assert lib.load().itts_mlpg_get_override(*[ctypes.byref(v) for v in vals]) == 0
    return tuple(v.value for v in vals)


def test_override_rejects_unknown_values_and_restores():
    L = lib.load()
    assert _override() == (0, 0, 0)
    for bad in ((1, 0, 0), (4, 0, 0), (-1, 0, 0), (0, 3, 0), (0, -1, 0), (0, 0, 3), (0, 0, -2)):
        assert L.itts_mlpg_set_override(*bad) == -1, bad
        assert b"itts_mlpg_set_override" in L.itts_last_error()
        assert _override() == (0, 0, 0)
    with pytest.raises(ValueError):
        with ops.mlpg_forced(solve="sweeps"):
            pass
    with ops.mlpg_forced(solve="ring", width="wide", nt=False):
        assert _override() == (MLPG_RING, 2, 1)
        with ops.mlpg_forced(solve="stream"):
            assert _override() == (MLPG_STREAM, 0, 0)
        assert _override() == (MLPG_RING, 2, 1)
        with pytest.raises(KeyError):
            with ops.mlpg_forced(width="narrow"):
                raise KeyError("inside")
        assert _override() == (MLPG_RING, 2, 1)
    assert _override() == (0, 0, 0)


def test_choose_form_rejects_bad_sizes():
    L = lib.load()
    for args in ((-1, 62, 300, 300), (1, 0, 300, 300), (1, 62, -1, 0), (2, 62, 300, 299)):
        assert L.itts_mlpg_choose_form(*args, 0) == -1, args
    with pytest.raises(lib.IttsError):
        ops.mlpg_choose_form(1, 0, 300, 300)


def test_last_form_is_per_thread_and_zero_before_any_call():
    got = []
    t = threading.Thread(target=lambda: got.append(ops.mlpg_last_form()))
    t.start()
    t.join()
    assert got == [0]


def test_form_names():
    assert ops.mlpg_form_name(0) == "none"
    assert ops.mlpg_form_name(MLPG_RING | MLPG_F32_ROWS | MLPG_WIDE) == "ring wide f32"
    assert ops.mlpg_form_name(MLPG_STREAM | F32) == "stream f32 widened"
    assert ops.mlpg_form_name(MLPG_RING | MLPG_NT_IN) == "ring nt-in"


def test_environment_seeds_the_override():
    """ITTS_MLPG_RING / STREAM / NARROW / WIDE / NO_NT (scripts/mlpg_time.py, the DESIGN notes) seed the override at
    its first use, in a fresh process (RING before STREAM, NARROW before WIDE, as before the override existed)."""
    code = ("import ctypes\n"
            "L = ctypes.CDLL(%r); v = [ctypes.c_int() for _ in range(3)]\n"
            "L.itts_mlpg_get_override(*[ctypes.byref(x) for x in v]); print([x.value for x in v])\n" % lib.LIB_PATH)
    base = {k: v for k, v in os.environ.items() if not k.startswith("ITTS_MLPG_")}
    for env, want in (({}, [0, 0, 0]),
                      ({"ITTS_MLPG_RING": "1"}, [MLPG_RING, 0, 0]),
                      ({"ITTS_MLPG_STREAM": "1"}, [MLPG_STREAM, 0, 0]),
                      ({"ITTS_MLPG_RING": "1", "ITTS_MLPG_STREAM": "1"}, [MLPG_RING, 0, 0]),
                      ({"ITTS_MLPG_WIDE": "1"}, [0, 2, 0]),
                      ({"ITTS_MLPG_NARROW": "1", "ITTS_MLPG_WIDE": "1"}, [0, 1, 0]),
                      ({"ITTS_MLPG_NO_NT": "1", "ITTS_MLPG_STREAM": "1"}, [MLPG_STREAM, 0, 1])):
        res = subprocess.run([sys.executable, "-c", code], env=dict(base, **env), stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True, timeout=120)
        assert res.returncode == 0, res.stdout[-2000:]
        assert res.stdout.strip().splitlines()[-1] == str(want), (env, res.stdout[-500:])
