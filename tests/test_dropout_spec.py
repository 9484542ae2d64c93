"""The dropout rule without a GPU: the numpy restatement (dropout_spec.py) against Philox4x32-10's published known
answers, the threshold at its edges, the keep rate and the independence of salts and seeds; FlatFFModel.from_module
reading a model's nn.Dropout modules; the C boundary of the new entry points (header, binding, exports, refusals
before any device work)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from dropout_spec import keep_mask, philox4x32_10, scale_f32, threshold
from idiaptts_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("itts_dropout_apply", "itts_dropout_act_bwd", "itts_linear_fwd_dropout", "itts_linear_fwd_sparse_dropout",
           "itts_linear_bwd_input_dropout", "itts_linear_bwd_dropout")
P = ctypes.c_void_p(64)       # never dereferenced: every call below is refused or empty


def _hex(words):
    return " ".join("{:08x}".format(int(w)) for w in words)


def test_philox_known_answers():
    # Random123 kat_vectors, philox4x32 10 rounds
    assert _hex(philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(philox4x32_10((ones,) * 4, (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_threshold_edges():
    assert threshold(0.0) == 0
    assert threshold(2.0 ** -32) == 1
    assert threshold(0.5) == 2 ** 31
    assert threshold(1.0 - 2.0 ** -33) == 2 ** 32 - 1
    assert scale_f32(0.0) == np.float32(1) and scale_f32(0.5) == np.float32(2)
    assert scale_f32(0.2) == np.float32(1) / np.float32(0.8)


@pytest.mark.parametrize("seed", [0, 1, 0x123456789abcdef])
@pytest.mark.parametrize("salt", [0, 1, 2])
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_rate(seed, salt, p):
    M, N = 301, 97
    kept = keep_mask(M, N, p, seed, salt).mean()
    sd = np.sqrt(p * (1 - p) / (M * N))
    print("keep rate seed {:#x} salt {} p {}: {:.4f} ({:+.2f} sd)".format(seed, salt, p, kept, (kept - (1 - p)) / sd))
    assert abs(kept - (1 - p)) < 3 * sd


def test_salts_and_seeds_give_unrelated_masks():
    a = keep_mask(64, 64, 0.5, 5, 0)
    for other in (keep_mask(64, 64, 0.5, 5, 1), keep_mask(64, 64, 0.5, 6, 0)):
        agree = (a == other).mean()
        print("agreement", agree)
        assert 0.45 < agree < 0.55


def test_mask_depends_on_position_only():
    # the row of a matrix alone equals the same row inside it, given the offset; the row word carries over at 2^32
    full = keep_mask(17, 97, 0.3, 9, 4, row_offset=2 ** 32 - 3)
    assert (keep_mask(1, 97, 0.3, 9, 4, row_offset=2 ** 32 - 3 + 16) == full[16:]).all()
    assert not (full[2] == full[3]).all()        # rows 2^32 - 1 and 2^32


def test_flat_model_reads_the_dropouts_of_a_module_stack():
    from idiaptts_amd.native_ff import FlatFFModel
    from idiaptts_amd.src.neural_networks.pytorch.models import rnn_dyn
    hp = types.SimpleNamespace(model_type="RNNDYN-2_TANH_8-1_FC_3", batch_first=False, dropout=0.2)
    model = rnn_dyn.convert_legacy_to_config((5,), hp).create_model()
    mods = [type(m).__name__ for g in model.layer_groups for m in g.module]
    assert mods == ["LinearAct", "FusedActivation", "Dropout"] * 2 + ["LinearAct", "Dropout"]
    assert all(isinstance(m, torch.nn.Dropout) for g in model.layer_groups for m in g.module
               if type(m).__name__ == "Dropout")
    # the salt of a dropout is the index in the model of the layer in front of it
    assert [m.salt for g in model.layer_groups for m in g.module if isinstance(m, torch.nn.Dropout)] == [0, 1, 2]
    flat = FlatFFModel.from_module(model, "cpu")
    assert flat is not None and flat.dropouts == [0.2, 0.2, 0.2]
    assert flat.dims == (5, 8, 8, 3) and flat.has_dropout()
    for i, m in enumerate(m for g in model.layer_groups for m in g.module if type(m).__name__ == "LinearAct"):
        assert torch.equal(flat.weight(i), m.weight.detach()) and torch.equal(flat.bias(i), m.bias.detach())
    # p = 1 stays with torch's module on the module path
    model.layer_groups[0].module[2].p = 1.0
    assert FlatFFModel.from_module(model, "cpu") is None
    with pytest.raises(ValueError):
        FlatFFModel((5, 8, 3), ("tanh", None), device="cpu", dropouts=(0.1, 1.0))
    with pytest.raises(ValueError):
        FlatFFModel((5, 8, 3), ("tanh", None), device="cpu", dropouts=(0.1,))
    assert FlatFFModel((5, 8, 3), ("tanh", None), device="cpu").dropouts == [0.0, 0.0]


def test_dropout_stream_is_private_and_repeatable():
    from idiaptts_amd.nn.functional import DropoutStream
    state = torch.get_rng_state()
    a, b = DropoutStream(), DropoutStream()
    a.reseed(1234)
    b.reseed(1234)
    first = [a.next() for _ in range(4)]
    assert first == [b.next() for _ in range(4)] and len(set(first)) == 4
    assert all(0 <= v < 2 ** 63 for v in first)
    assert torch.equal(torch.get_rng_state(), state)          # torch's own generator was not consumed
    c = DropoutStream()
    lazy = [c.next() for _ in range(2)]                       # seeded from torch.initial_seed()
    c.restart()
    assert [c.next() for _ in range(2)] == lazy


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
        assert "double p, uint64_t seed, uint32_t salt, int64_t row_offset" in " ".join(proto.group(1).split())


def _rule(p=0.5):
    return (ctypes.c_double(p), ctypes.c_uint64(7), ctypes.c_uint32(1), ctypes.c_int64(0))


def _apply(L, x=P, ldi=8, out=P, ldo=8, M=4, N=8, mask_only=0, p=0.5):
    return L.itts_dropout_apply(x, ldi, out, ldo, M, N, mask_only, *_rule(p), None)


def _act_bwd(L, dy=P, lddy=8, d=P, ldd=8, dz=P, lddz=8, M=4, N=8, act=1, p=0.5):
    return L.itts_dropout_act_bwd(dy, lddy, d, ldd, dz, lddz, M, N, act, *_rule(p), None)


def _fwd(L, x=P, ldx=8, w=P, b=P, y=P, ldy=8, M=4, N=8, K=8, act=1, p=0.5):
    return L.itts_linear_fwd_dropout(x, ldx, w, b, y, ldy, M, N, K, act, *_rule(p), None)


def _fwd_sparse(L, lists=P, x=P, ldx=8, w=P, b=P, y=P, ldy=8, M=4, N=8, K=8, act=1, p=0.5):
    return L.itts_linear_fwd_sparse_dropout(lists, x, ldx, w, b, y, ldy, M, N, K, act, *_rule(p), None)


def _bwd_input(L, dz=P, lddz=8, w=P, dx=P, lddx=8, yprev=P, ldyp=8, act=1, M=4, N=8, K=8, p=0.5):
    return L.itts_linear_bwd_input_dropout(dz, lddz, w, dx, lddx, yprev, ldyp, act, M, N, K, *_rule(p), None)


def _bwd(L, dz=P, lddz=8, x=P, ldx=8, w=P, dw=P, db=P, dx=P, lddx=8, yprev=P, ldyp=8, act=1, M=4, N=8, K=8, ws=P,
         p=0.5):
    return L.itts_linear_bwd_dropout(dz, lddz, x, ldx, w, dw, db, dx, lddx, yprev, ldyp, act, M, N, K, ws, 0, *_rule(p),
                                     None)


CALLS = (_apply, _act_bwd, _fwd, _fwd_sparse, _bwd_input, _bwd)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5, float("nan")])
def test_bad_probabilities_are_refused(call, p):
    L = lib.load()
    assert call(L, p=p) == -1
    assert "dropout p must be in [0, 1)" in L.itts_last_error().decode()


@pytest.mark.parametrize("call,kwargs,needle", [
    (_apply, dict(ldi=7), "bad sizes"),
    (_apply, dict(ldo=7), "bad sizes"),
    (_apply, dict(N=0), "bad sizes"),
    (_apply, dict(M=-1), "bad sizes"),
    (_apply, dict(x=None), "null pointer"),
    (_apply, dict(out=None), "null pointer"),
    (_apply, dict(out=None, mask_only=1), "null pointer"),
    (_act_bwd, dict(lddy=7), "bad sizes"),
    (_act_bwd, dict(ldd=7), "bad sizes"),
    (_act_bwd, dict(lddz=7), "bad sizes"),
    (_act_bwd, dict(d=None), "null pointer"),
    (_act_bwd, dict(act=99), "unknown activation"),
    (_fwd, dict(ldx=7), "bad sizes"),
    (_fwd, dict(ldy=7), "bad sizes"),
    (_fwd, dict(w=None), "null pointer"),
    (_fwd, dict(y=None), "null pointer"),
    (_fwd, dict(act=-1), "unknown activation"),
    (_fwd_sparse, dict(ldy=7), "bad sizes"),
    (_fwd_sparse, dict(lists=None), "null pointer"),
    (_fwd_sparse, dict(K=70000, ldx=70000), "bad sizes"),
    (_bwd_input, dict(lddz=7), "bad sizes"),
    (_bwd_input, dict(lddx=7), "bad sizes"),
    (_bwd_input, dict(ldyp=7), "bad sizes"),
    (_bwd_input, dict(dx=None), "null pointer"),
    (_bwd_input, dict(yprev=None), "previous layer's output"),
    (_bwd_input, dict(act=99), "unknown activation"),
    (_bwd, dict(ldx=7), "bad sizes"),
    (_bwd, dict(ldyp=7), "bad sizes"),
    (_bwd, dict(ws=None), "null pointer"),
    (_bwd, dict(dw=None), "null pointer"),
    (_bwd, dict(yprev=None), "previous layer's output"),
    # p == 0 is the plain entry point, refusals included
    (_fwd, dict(p=0.0, ldx=7), "itts_linear_fwd: bad sizes"),
    (_fwd_sparse, dict(p=0.0, ldy=7), "itts_linear_fwd_sparse: bad sizes"),
    (_bwd_input, dict(p=0.0, lddx=7), "itts_linear_bwd_input: bad sizes"),
    (_bwd, dict(p=0.0, ws=None), "itts_linear_bwd: null pointer"),
])
def test_refusals_come_with_a_message_before_any_device_work(call, kwargs, needle):
    L = lib.load()
    assert call(L, **kwargs) == -1
    message = L.itts_last_error().decode()
    assert needle in message and message.startswith("itts_"), message


def test_empty_calls_succeed_without_device_work():
    L = lib.load()
    assert _apply(L, x=None, out=None, M=0) == 0
    assert _act_bwd(L, dy=None, d=None, dz=None, M=0) == 0
    assert _fwd(L, x=None, y=None, M=0) == 0
    assert _fwd_sparse(L, lists=None, x=None, y=None, M=0) == 0
    assert _bwd_input(L, dz=None, dx=None, M=0) == 0
