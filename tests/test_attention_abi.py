"""The C boundary of csrc/attention.hip without a GPU: header, ctypes binding and exports agree; every refusal comes
back as ITTS_E_INVALID with a message naming the offending value before any device work (the pointers handed in are
null or bogus: a call that got as far as a launch would not return -1); empty batches succeed; the workspace size is
the one written out by hand."""
import ctypes
import os
import re

import pytest

from idiaptts_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("itts_attention_workspace_bytes", "itts_attention_fwd", "itts_attention_bwd")
P = ctypes.c_void_p(64)       # never dereferenced: every call below is refused or empty


def _fwd(L, qkv=P, o=P, klen=P, lse=P, B=2, T=9, H=2, dh=16, sb=9, st=1, p=0.0):
    return L.itts_attention_fwd(qkv, o, klen, lse, B, T, H, dh, sb, st, p, 1, 0, None)


def _bwd(L, do=P, qkv=P, o=P, klen=P, lse=P, dqkv=P, B=2, T=9, H=2, dh=16, sb=9, st=1, p=0.0):
    return L.itts_attention_bwd(do, qkv, o, klen, lse, dqkv, B, T, H, dh, sb, st, p, 1, 0, None)


def test_header_binding_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "idiaptts_amd.h")).read()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in SYMBOLS:
        proto = re.search(r"\b(int|int64_t) " + name + r"\s*\(([^)]*)\)", text)
        assert proto, name + " is not declared in the header"
        assert hasattr(cdll, name), "missing export " + name
        restype, argtypes = lib._SIGNATURES[name]
        assert restype is (ctypes.c_int if proto.group(1) == "int" else ctypes.c_int64)
        assert len(argtypes) == len(proto.group(2).split(",")), name + ": binding and header differ in arity"
    for cite in ("torch.nn.MultiheadAttention", "torch.nn.TransformerEncoderLayer", "rnn_dyn/FFWrapper.py:62-73"):
        assert cite in text, cite
    from idiaptts_amd import ops
    assert ops.ATTENTION_MAX_HEAD_DIM == 128 and ops.ATTENTION_MIN_HEAD_DIM == 4 and ops.ATTENTION_HEAD_DIM_STEP == 4
    assert (ops.ATTENTION_MAX_WIDTH, ops.ATTENTION_MAX_TIME, ops.ATTENTION_MAX_BATCH_HEADS) == (1024, 32768, 65535)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
@pytest.mark.parametrize("kwargs,needle", [
    (dict(dh=6), "dh = 6"),
    (dict(dh=136), "dh = 136"),
    (dict(dh=2), "dh = 2"),
    (dict(dh=132), "dh = 132"),
    (dict(dh=0), "dh = 0"),
    (dict(H=65, dh=16), "D = 1040"),
    (dict(H=0), "H = 0"),
    (dict(T=0), "T = 0"),
    (dict(T=32769), "T = 32769"),
    (dict(B=65536, H=1), "B * H = 65536"),
    (dict(B=21846, H=3), "B * H = 65538"),
    (dict(B=-1), "B = -1"),
    (dict(sb=0), "row strides 0, 1"),
    (dict(p=1.0), "dropout p must be in [0, 1)"),
    (dict(p=-0.5), "dropout p must be in [0, 1)"),
    (dict(qkv=None), "null pointer"),
    (dict(o=None), "null pointer"),
    (dict(lse=None), "null pointer"),
    (dict(qkv=ctypes.c_void_p(68)), "16-byte aligned"),
])
def test_refusals_name_the_value_before_any_device_work(call, kwargs, needle):
    L = lib.load()
    assert call(L, **kwargs) == -1
    message = L.itts_last_error().decode()
    assert needle in message, message
    assert ("itts_attention_fwd" if call is _fwd else "itts_attention_bwd") in message


def test_backward_null_pointers():
    L = lib.load()
    for kwargs in (dict(do=None), dict(dqkv=None)):
        assert _bwd(L, **kwargs) == -1
        assert "null pointer" in L.itts_last_error().decode()


def test_empty_batches_succeed_without_device_work():
    L = lib.load()
    assert _fwd(L, qkv=None, o=None, klen=None, lse=None, B=0) == 0
    assert _bwd(L, do=None, qkv=None, o=None, klen=None, lse=None, dqkv=None, B=0) == 0


def test_workspace_bytes():
    L = lib.load()
    # one float per utterance, head and query: the log-sum-exp
    assert L.itts_attention_workspace_bytes(64, 8, 1977) == 64 * 8 * 1977 * 4
    assert L.itts_attention_workspace_bytes(3, 2, 1) == 24
    assert L.itts_attention_workspace_bytes(65535, 1, 32768) == 65535 * 32768 * 4           # beyond 2^31
    assert L.itts_attention_workspace_bytes(0, 8, 5) == 0 and L.itts_attention_workspace_bytes(2, 8, 0) == 0
