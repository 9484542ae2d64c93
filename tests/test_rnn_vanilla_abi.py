"""The vanilla RNN layer entry points without a GPU: bad arguments come back as ITTS_E_INVALID (-1) with a message
before any device is touched (the device pointers handed over here are not addresses of anything), the scratch size
follows the header's formula, refused calls are not counted, and nn.RNN layers are never widened to the persistent
kernels' 512."""
import ctypes

import numpy as np
import pytest
import torch

from idiaptts_amd import lib, ops
from idiaptts_amd.nn import modules

FAKE = ctypes.c_void_p(4096)       # stands for a device pointer: a call that got as far as using it would fault


def _lengths(values):
    arr = np.asarray(values, dtype=np.int32)
    return arr, ctypes.c_void_p(arr.ctypes.data)


def _fwd(L, h_lengths, T=3, B=2, H=16, ndir=2, act=ops.ACT_TANH, **nulls):
    p = {k: FAKE for k in ("gin", "whh", "h0", "d_lengths", "row_off", "rev_row", "y", "hn", "state")}
    p.update(nulls)
    return L.itts_rnn_layer_fwd(p["gin"], p["whh"], p["h0"], p["d_lengths"], h_lengths, p["row_off"], p["rev_row"], T, B,
                                H, ndir, act, p["y"], p["hn"], p["state"], None)


def _bwd(L, h_lengths, T=3, B=2, H=16, ndir=2, act=ops.ACT_RELU, **nulls):
    p = {k: FAKE for k in ("dy", "whh", "y", "row_off", "rev_row", "dg", "state")}
    p.update(nulls)
    return L.itts_rnn_layer_bwd(p["dy"], p["whh"], p["y"], h_lengths, p["row_off"], p["rev_row"], T, B, H, ndir, act,
                                p["dg"], p["state"], None)


def _refused(L, status, name):
    """-1 and a message; the entry point's own checks name it (the geometry checks are the recurrences' shared ones)"""
    assert status == -1
    msg = L.itts_last_error()
    assert msg and (msg.startswith(name.encode()) or msg.startswith(b"rnn_check")), msg


def test_bad_arguments_are_refused_before_any_device_work():
    L = lib.load()
    assert L.itts_abi_version() == 1
    keep, h_len = _lengths([3, 2])
    before = ops.rnn_layer_counts()
    for call, name, operands in ((_fwd, "itts_rnn_layer_fwd", ("gin", "whh", "d_lengths", "row_off", "y", "state")),
                                 (_bwd, "itts_rnn_layer_bwd", ("dy", "whh", "y", "row_off", "dg", "state"))):
        _refused(L, call(L, h_len, H=40), name)
        assert b"multiple of 16" in L.itts_last_error()
        _refused(L, call(L, h_len, H=0), name)
        for act in (ops.ACT_NONE, ops.ACT_SIGMOID, -1, 99):
            _refused(L, call(L, h_len, act=act), name)
            assert b"activation" in L.itts_last_error()
        for operand in operands:
            _refused(L, call(L, h_len, **{operand: None}), name)
            assert b"null pointer" in L.itts_last_error()
        _refused(L, call(L, h_len, rev_row=None), name)                  # two directions need the reverse row table
        _refused(L, call(L, None), name)                                 # no host copy of the lengths
        _refused(L, call(L, h_len, T=4), name)                           # T is not the longest length
        _refused(L, call(L, h_len, ndir=3), name)
        _refused(L, call(L, _lengths([2, 3])[1], T=2), name)             # not sorted by decreasing length
        _refused(L, call(L, _lengths([3, 0])[1]), name)                  # an empty row
    assert L.itts_rnn_layer_counts(None) == -1
    assert ops.rnn_layer_counts() == before                              # refused calls are not layer calls
    del keep


@pytest.mark.parametrize("B,H,ndir", [(1, 16, 1), (17, 48, 2), (64, 512, 2), (70, 576, 1)])
def test_state_bytes_follow_the_header_formula(B, H, ndir):
    """running state and carried gradient, two step parities each, and one re-tiled W_hh -- a quarter of the re-tiled
    weights the LSTM / GRU entry points reserve"""
    L = lib.load()
    assert L.itts_rnn_layer_state_bytes(B, H, ndir) == 4 * (4 * ndir * B * H + ndir * H * H)
    assert L.itts_rnn_layer_state_bytes(B, H, ndir) < L.itts_gru_state_bytes(B, H, ndir)
    for bad in ((0, H, ndir), (B, 0, ndir), (B, H, 0)):
        assert L.itts_rnn_layer_state_bytes(*bad) == 0


def test_rnn_layers_are_never_widened_to_the_persistent_width(monkeypatch):
    monkeypatch.setenv("ITTS_RNN_PAD_HIDDEN", "1")
    monkeypatch.setenv("ITTS_RNN_PERSISTENT", "1")
    H, F = 288, 8
    operands = (torch.zeros(2, H, F), torch.zeros(2, H, H), [torch.zeros(2, H)] * 2, [None])
    assert modules._pad_hidden(*operands, 1, H, rows=4)[-1] == 512       # what an LSTM / GRU layer would get
    assert modules._pad_hidden(*operands, 1, H, rows=4, persistent=False)[-1] == H
    assert modules._pad_hidden(torch.zeros(2, 40, F), torch.zeros(2, 40, 40), [torch.zeros(2, 40)] * 2, [None], 1, 40,
                               rows=4, persistent=False)[-1] == 48
    assert modules.RNN._persistent is False and modules.LSTM._persistent and modules.GRU._persistent
    assert modules.RNN._layer_function.__name__ == "RNNLayerFunction"
