"""The C boundary of the all-pass warping kernels without a GPU: header, ctypes binding and exports agree on the two
entry points, every refusal comes back as ITTS_E_INVALID with a message naming the offending value before any device
work (the pointers handed in are null or bogus: a call that got as far as a launch would not return -1), and an
empty call succeeds."""
import ctypes
import os
import re

import pytest

from idiaptts_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("itts_allpass_warp_fwd", "itts_allpass_warp_bwd")
P = ctypes.c_void_p(64)       # never dereferenced: every call below is refused or empty


def _fwd(L, M=4, D=10, N=5, ldx=None, ldy=None, x=P, alpha=P, y=P):
    return L.itts_allpass_warp_fwd(x, D if ldx is None else ldx, alpha, None, None, y, D if ldy is None else ldy,
                                   M, D, N, None)


def _bwd(L, M=4, D=10, N=5, lddy=None, ldx=None, lddx=None, dy=P, x=P, alpha=P, dx=P, da=P):
    return L.itts_allpass_warp_bwd(dy, D if lddy is None else lddy, x, D if ldx is None else ldx, alpha, None, None,
                                   dx, D if lddx is None else lddx, da, M, D, N, None)


def test_header_binding_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "idiaptts_amd.h")).read()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in SYMBOLS:
        proto = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", text)
        assert proto, name + " is not declared in the header"
        assert hasattr(cdll, name), "missing export " + name
        restype, argtypes = lib._SIGNATURES[name]
        assert restype is ctypes.c_int
        assert len(argtypes) == len(proto.group(1).split(",")), name + ": binding and header differ in arity"
    # each cites its reference call site
    for cite in ("layers/AllPassWarp.py:148-173", "layers/AllPassWarpLayer.py:141-150", "layers/AllPassWarp.py:157-171"):
        assert cite in text


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
@pytest.mark.parametrize("kwargs,needle", [
    (dict(N=0, D=10), "N = 0"),
    (dict(N=-3, D=9), "N = -3"),
    (dict(N=65, D=130), "N = 65"),
    (dict(N=5, D=12), "D = 12"),
    (dict(N=5, D=0), "D = 0"),
    (dict(N=5, D=10, ldx=9), "pitch 9"),
    (dict(N=5, D=10, M=-1), "M = -1"),
    (dict(N=5, D=10, x=None), "null pointer with M = 4"),
    (dict(N=5, D=10, alpha=None), "null pointer with M = 4"),
])
def test_refusals_name_the_value(call, kwargs, needle):
    L = lib.load()
    assert call(L, **kwargs) == -1
    msg = L.itts_last_error().decode()
    assert msg.startswith("itts_allpass_warp_" + ("fwd" if call is _fwd else "bwd")), msg
    assert needle in msg, msg


def test_every_pitch_and_pointer_is_checked():
    L = lib.load()
    assert _fwd(L, ldy=9) == -1 and "pitch 9" in L.itts_last_error().decode()
    assert _fwd(L, y=None) == -1
    for name in ("lddy", "lddx"):
        assert _bwd(L, **{name: 7}) == -1 and "pitch 7" in L.itts_last_error().decode()
    for name in ("dy", "dx", "da"):
        assert _bwd(L, **{name: None}) == -1 and "null pointer" in L.itts_last_error().decode()


def test_limits_are_inclusive_and_an_empty_call_succeeds():
    L = lib.load()
    # M == 0: nothing to do, whatever the pointers; the sizes are still checked
    assert _fwd(L, M=0, N=64, D=256, x=None, alpha=None, y=None) == 0
    assert _bwd(L, M=0, N=1, D=3, dy=None, x=None, alpha=None, dx=None, da=None) == 0
    assert _fwd(L, M=0, N=65, D=65) == -1
    assert _bwd(L, M=0, N=5, D=11) == -1


def test_module_refuses_what_the_kernel_does_not_take():
    from idiaptts_amd import ops
    from idiaptts_amd.nn import AllPassWarp
    assert ops.ALLPASS_MAX_SIZE == 64
    AllPassWarp(64)
    with pytest.raises(NotImplementedError, match="65"):
        AllPassWarp(65)
    import torch
    with pytest.raises(ValueError, match="32.*5|5.*32"):
        AllPassWarp(5)(torch.zeros(2, 3, 32), torch.zeros(2, 3, 1))
    assert not list(AllPassWarp(30).buffers()) and not list(AllPassWarp(30).parameters())
    a1, a2 = torch.tensor([[[0.1]]]), torch.tensor([[[0.2]]])
    assert AllPassWarp.combine_warping_parameters(a1) is a1
    assert torch.allclose(AllPassWarp.combine_warping_parameters([a1, a2, a1]),
                          ((a1 + a2) / (1 + a1 * a2) + a1) / (1 + (a1 + a2) / (1 + a1 * a2) * a1))
