"""The C boundary of the MLPG adjoint without a GPU: header, ctypes binding and exports agree on the three entry points;
bad sizes, pitches, pointers and offsets come back as ITTS_E_INVALID with a message before any device work (the
pointers handed in are bogus: a call that got as far as a launch would not return -1); empty calls succeed."""
import ctypes
import os
import re

import pytest
import torch

from idiaptts_amd import lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"itts_mlpg_adjoint_scratch_bytes": "int64_t", "itts_mlpg_adjoint": "int", "itts_mlpg_adjoint_planned": "int"}
P = ctypes.c_void_p(64)       # never dereferenced: every call below is refused or empty


def _offsets(values):
    return (ctypes.c_int64 * len(values))(*values)


def _call(L, gout=P, g32=0, ldg=4, gcol0=0, dim=4, var=P, offsets=(0, 5), gfeat=P, o32=0, ldo=12, col0=0, scratch=P):
    offs = _offsets(offsets) if offsets is not None else None
    n_utts = len(offsets) - 1 if offsets is not None else 1
    return L.itts_mlpg_adjoint(gout, g32, ldg, gcol0, dim, var, offs, n_utts, gfeat, o32, ldo, col0, scratch, None)


def test_header_binding_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "idiaptts_amd.h")).read()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name, ret in SYMBOLS.items():
        proto = re.search(r"\b" + ret + " " + name + r"\s*\(([^)]*)\)", text)
        assert proto, name + " is not declared in the header"
        assert hasattr(cdll, name), "missing export " + name
        restype, argtypes = lib._SIGNATURES[name]
        assert restype is (ctypes.c_int64 if ret == "int64_t" else ctypes.c_int)
        assert len(argtypes) == len(proto.group(1).split(",")), name + ": binding and header differ in arity"
    hip = open(os.path.join(ROOT, "idiaptts_amd", "csrc", "mlpg.hip")).read()
    assert hip.count('#include "mlpg_adjoint.h"') == 1
    for other in os.listdir(os.path.join(ROOT, "idiaptts_amd", "csrc")):
        if other not in ("mlpg.hip", "mlpg_adjoint.h"):
            assert "mlpg_adjoint.h" not in open(os.path.join(ROOT, "idiaptts_amd", "csrc", other), errors="replace").read()


def test_scratch_is_the_forwards_plus_one_plane():
    L = lib.load()
    for t_total, dim in ((0, 3), (1, 1), (946, 65), (70000, 60)):
        assert L.itts_mlpg_adjoint_scratch_bytes(t_total, dim) == L.itts_mlpg_scratch_bytes(t_total, dim) + t_total * dim * 8
    assert L.itts_mlpg_adjoint_scratch_bytes(-1, 3) == 0 and L.itts_mlpg_adjoint_scratch_bytes(5, 0) == 0


@pytest.mark.parametrize("kwargs,needle", [
    (dict(dim=0, ldg=4, ldo=12), "bad sizes"),
    (dict(dim=-2), "bad sizes"),
    (dict(gcol0=-1), "bad sizes"),
    (dict(col0=-1), "bad sizes"),
    (dict(ldg=3), "leading dimension too small"),
    (dict(gcol0=1, ldg=4), "leading dimension too small"),
    (dict(ldo=11), "leading dimension too small"),
    (dict(col0=2, ldo=13), "leading dimension too small"),
    (dict(gout=None), "null pointer"),
    (dict(gfeat=None), "null pointer"),
    (dict(scratch=None), "null pointer"),
    (dict(var=None), "null pointer"),
    (dict(offsets=None), "null pointer"),
    (dict(offsets=(1, 5)), "offsets must start at 0"),
    (dict(offsets=(0, 5, 3)), "offsets must be non-decreasing"),
    (dict(offsets=(0, 0, 0, 1)), "more utterances than frames"),
    (dict(dim=16 * 65535 + 1, ldg=1 << 21, ldo=1 << 23), "too many dimensions"),
])
def test_refusals_come_with_a_message_before_any_device_work(kwargs, needle):
    L = lib.load()
    assert _call(L, **kwargs) == -1
    assert needle in L.itts_last_error().decode(), L.itts_last_error()


def test_empty_calls_succeed_and_a_missing_plan_is_refused():
    L = lib.load()
    assert _call(L, offsets=(0,), gout=None, gfeat=None, scratch=None) == 0          # no utterances
    assert _call(L, offsets=(0, 0)) == 0                                             # one empty utterance, no frames
    assert _call(L, offsets=(0,), dim=0) == -1                                       # the sizes are still checked
    assert L.itts_mlpg_adjoint_planned(None, P, 0, 4, 0, 4, P, P, 0, 12, 0, P, None) == -1
    assert "null pointer" in L.itts_last_error().decode()
    plan = ctypes.c_void_p()
    assert L.itts_mlpg_plan_create(_offsets((0,)), 0, ctypes.byref(plan)) == 0       # (no utterances: no device memory)
    try:
        assert L.itts_mlpg_adjoint_planned(plan, None, 0, 4, 0, 4, P, None, 0, 12, 0, None, None) == 0
        assert L.itts_mlpg_adjoint_planned(plan, None, 0, 3, 0, 4, P, None, 0, 12, 0, None, None) == -1
    finally:
        L.itts_mlpg_plan_destroy(plan)


def test_the_wrapper_checks_shapes_and_has_no_cpu_path():
    var = torch.ones(6, dtype=torch.float64)
    with pytest.raises(lib.IttsError, match="GPU"):
        ops.mlpg_adjoint(torch.zeros(5, 2, dtype=torch.float64), var, 2, [0, 5])
    with pytest.raises(TypeError, match="float32 or float64"):
        ops.mlpg_adjoint(torch.zeros(5, 2, dtype=torch.float16), var, 2, [0, 5])
