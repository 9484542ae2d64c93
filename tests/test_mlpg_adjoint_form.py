"""The MLPG adjoint's choice of form without a GPU: sweeps under 194 frames and the stream form from there, an
override of its own that round-trips, refuses other values and leaves the forward's alone, and a scratch size that has
not grown with the second form."""
import ctypes
import os
import re

import pytest

from idiaptts_amd import lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("itts_mlpg_adjoint_choose_form", "itts_mlpg_adjoint_set_override", "itts_mlpg_adjoint_get_override",
           "itts_mlpg_adjoint_last_form")


def test_header_binding_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "idiaptts_amd.h")).read()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in SYMBOLS:
        proto = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", text)
        assert proto, name + " is not declared in the header"
        assert hasattr(cdll, name), "missing export " + name
        restype, argtypes = lib._SIGNATURES[name]
        args = [a for a in proto.group(1).split(",") if a.strip() != "void"]
        assert restype is ctypes.c_int and len(argtypes) == len(args), name


@pytest.mark.parametrize("t_max,form", [(0, ops.MLPG_SWEEPS), (1, ops.MLPG_SWEEPS), (193, ops.MLPG_SWEEPS),
                                        (194, ops.MLPG_STREAM), (5000, ops.MLPG_STREAM)])
def test_choice_changes_at_194_frames(t_max, form):
    for n_utts, dim in ((1, 1), (64, 60), (4096, 130)):          # neither the batch size nor the width matters: no ring form
        assert ops.mlpg_adjoint_choose_form(n_utts, dim, t_max, max(t_max, 1) * n_utts) == form


def test_bad_sizes_are_refused():
    L = lib.load()
    for args in ((-1, 4, 5, 5), (1, 0, 5, 5), (1, 4, -1, 5), (1, 4, 6, 5)):
        assert L.itts_mlpg_adjoint_choose_form(*args) == -1
        assert "bad sizes" in L.itts_last_error().decode()
    with pytest.raises(lib.IttsError):
        ops.mlpg_adjoint_choose_form(1, 0, 5, 5)


def test_override_round_trips_and_refuses_other_values():
    L = lib.load()
    assert L.itts_mlpg_adjoint_get_override() == 0
    forward = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int()]
    L.itts_mlpg_get_override(*[ctypes.byref(p) for p in forward])
    with ops.mlpg_adjoint_forced(ops.MLPG_SWEEPS):
        assert L.itts_mlpg_adjoint_get_override() == ops.MLPG_SWEEPS
        assert ops.mlpg_adjoint_choose_form(64, 60, 5000, 320000) == ops.MLPG_SWEEPS
        with ops.mlpg_adjoint_forced("stream"):
            assert ops.mlpg_adjoint_choose_form(64, 60, 1, 64) == ops.MLPG_STREAM
            with ops.mlpg_adjoint_forced(None):
                assert ops.mlpg_adjoint_choose_form(64, 60, 193, 320000) == ops.MLPG_SWEEPS
                assert ops.mlpg_adjoint_choose_form(64, 60, 194, 320000) == ops.MLPG_STREAM
            assert L.itts_mlpg_adjoint_get_override() == ops.MLPG_STREAM
        assert L.itts_mlpg_adjoint_get_override() == ops.MLPG_SWEEPS
        # the forward's word is another one
        now = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int()]
        L.itts_mlpg_get_override(*[ctypes.byref(p) for p in now])
        assert [p.value for p in now] == [p.value for p in forward]
        assert ops.mlpg_choose_form(4, 60, 5000, 20000) & ops.MLPG_SOLVE_MASK == ops.MLPG_STREAM
    assert L.itts_mlpg_adjoint_get_override() == 0
    for bad in (ops.MLPG_RING, -1, 4, ops.MLPG_STREAM | ops.MLPG_F32_ROWS):
        assert L.itts_mlpg_adjoint_set_override(bad) == -1
        assert "sweeps or stream" in L.itts_last_error().decode()
        assert L.itts_mlpg_adjoint_get_override() == 0
    for bad in (ops.MLPG_RING, "ring", True, 7):
        with pytest.raises(ValueError, match="mlpg_adjoint_forced"):
            with ops.mlpg_adjoint_forced(bad):
                pass
    with pytest.raises(RuntimeError):                     # the previous value comes back when the body raises
        with ops.mlpg_adjoint_forced("sweeps"):
            raise RuntimeError("body")
    assert L.itts_mlpg_adjoint_get_override() == 0


def test_last_form_is_zero_when_no_call_ran_on_the_thread():
    import threading
    seen = []
    worker = threading.Thread(target=lambda: seen.append(ops.mlpg_adjoint_last_form()))
    worker.start()
    worker.join()
    assert seen == [0]
    # a call that is refused, or has nothing to solve, leaves 0 behind
    L = lib.load()
    offs = (ctypes.c_int64 * 2)(0, 0)
    P = ctypes.c_void_p(64)                               # never dereferenced
    assert L.itts_mlpg_adjoint(P, 0, 4, 0, 4, P, offs, 1, P, 0, 12, 0, P, None) == 0
    assert ops.mlpg_adjoint_last_form() == 0
    assert L.itts_mlpg_adjoint(P, 0, 3, 0, 4, P, offs, 1, P, 0, 12, 0, P, None) == -1
    assert ops.mlpg_adjoint_last_form() == 0


def test_scratch_has_not_grown():
    """The formula of the header before the stream form: the forward's scratch -- three factor planes, the device copy of
    the offsets (t_total + 2 entries), nconv padded to 8 bytes, 8 spare -- plus ONE [t_total, dim] float64 plane (y of
    the sweeps, z of the stream form)."""
    L = lib.load()
    for t_total, dim in ((1, 1), (6660, 130), (6660, 63), (70000, 60), (946, 65)):
        forward = 3 * t_total * dim * 8 + (t_total + 2) * 8 + (dim * 4 + 16) // 8 * 8 + 8
        assert L.itts_mlpg_adjoint_scratch_bytes(t_total, dim) == forward + t_total * dim * 8
    assert L.itts_mlpg_adjoint_scratch_bytes(-1, 3) == 0 and L.itts_mlpg_adjoint_scratch_bytes(5, 0) == 0
