"""The C boundary of csrc/fixed_attention.hip and csrc/rnn_cell.hip without a GPU: the plan query, and every refusal
by name -- they come back as ITTS_E_INVALID with a message before any device work, so null pointers are enough."""
import pytest

from idiaptts_amd import lib, ops

INVALID = -1


def _fwd(B=1, T=4, P=4, C=4, n=1, partial=0, ldA=None, ldE=None):
    L = lib.load()
    K = -(-T // n) if partial else T // max(n, 1)
    rc = L.itts_fixed_attention_fwd(None, P if ldA is None else ldA, T * P, None, C if ldE is None else ldE, P * C, B, T,
                                    P, C, n, partial, None, P, K * P, None, C, K * C, None)
    return rc, L.itts_last_error().decode()


def test_plan_reports_grids_lds_and_access_width():
    plan = ops.fixed_attention_plan(64, 1977, 150, 512, 1)
    assert plan == {"K": 1977, "fwd_grid": 64 * 495, "fwd_lds_bytes": 4 * 150 * 8, "bwd_grid": (64 * 10, 2),
                    "vec_p": False, "vec_c": True}
    plan = ops.fixed_attention_plan(2, 7, 2048, 4096, 5, partial_last=True)         # the envelope's corner
    assert plan["K"] == 2 and plan["fwd_lds_bytes"] == 65536 and plan["bwd_grid"] == (2 * 128, 16) and plan["vec_p"]
    assert ops.fixed_attention_plan(3, 0, 5, 7, 64)["K"] == 0
    for bad in (dict(P=2049), dict(P=0), dict(C=4097), dict(C=0), dict(n=65), dict(n=0), dict(T=7, n=2), dict(B=-1)):
        with pytest.raises(ValueError, match="no fixed-attention plan"):
            ops.fixed_attention_plan(**{**dict(B=1, T=4, P=4, C=4, n=1), **bad})


def test_forward_refusals_name_what_is_wrong():
    for kwargs, text in ((dict(P=2049), "P = 2049 is outside 1 .. 2048"), (dict(C=4097), "C = 4097 is outside 1 .. 4096"),
                         (dict(T=130, n=65), "n_frames_per_step = 65 is outside 1 .. 64"), (dict(n=0), "n_frames_per_step = 0"),
                         (dict(T=7, n=2), "T = 7 is not a multiple of n_frames_per_step = 2 and partial_last is not set"),
                         (dict(ldA=3), "pitch ldA = 3 is below the width 4"), (dict(ldE=2), "pitch ldE = 2 is below"),
                         (dict(B=-1), "B = -1 is negative"), (dict(), "null pointer")):
        rc, msg = _fwd(**kwargs)
        assert rc == INVALID and "itts_fixed_attention_fwd" in msg and text in msg, (kwargs, msg)
    assert _fwd(B=0)[0] == 0 and _fwd(T=0)[0] == 0                                   # nothing to do: no pointer is read


def test_backward_and_cell_step_refusals():
    L = lib.load()
    assert L.itts_fixed_attention_bwd(None, 2049, 0, None, 4, 0, 1, 2, 2049, 4, None, 4, 0, None) == INVALID
    assert "P = 2049" in L.itts_last_error().decode()
    assert L.itts_fixed_attention_bwd(None, 4, 8, None, 4, 8, 1, 2, 4, 4, None, 3, 12, None) == INVALID
    assert "pitch ldE = 3" in L.itts_last_error().decode()
    assert L.itts_fixed_attention_bwd(None, 4, 8, None, 4, 8, 1, 2, 4, 4, None, 4, 16, None) == INVALID
    assert "null pointer" in L.itts_last_error().decode()
    assert L.itts_fixed_attention_bwd(None, 4, 8, None, 4, 8, 0, 2, 4, 4, None, 4, 16, None) == 0

    def step(kind=0, act=1, ld=80, H=20, B=2):
        rc = L.itts_rnn_cell_step(kind, act, None, ld, None, ld, None, None, H, None, H, B, H, None, H, None, H, None)
        return rc, L.itts_last_error().decode()
    for kwargs, text in ((dict(kind=3), "unknown cell kind = 3"), (dict(kind=2, act=5), "neither tanh nor ReLU"),
                         (dict(ld=79), "pitch ldgi = 79 is below 80"), (dict(H=0), "H = 0 is not positive"),
                         (dict(), "null pointer")):
        rc, msg = step(**kwargs)
        assert rc == INVALID and "itts_rnn_cell_step" in msg and text in msg, (kwargs, msg)
    assert step(B=0)[0] == 0
    assert (ops.CELL_LSTM, ops.CELL_GRU, ops.CELL_RNN) == (0, 1, 2)
