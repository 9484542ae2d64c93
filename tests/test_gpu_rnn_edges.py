"""Edges of the recurrent layers against torch.nn.LSTM / GRU / RNN in float64 on the CPU (tests/rnn_cases.py: the
case table and compare(); tests/test_rnn_cases.py proves what the table reaches):

* the inference path (torch.no_grad(): gates == csave == NULL) by VALUE, on both kernel families, and bit for bit
  against the training-mode forward;
* one direction at H = 512: 8 tiles per round, 128 rows per round, rev_row == NULL, a (H/4, 1) step grid;
* gradients of the initial states through the persistent backward (the d0 store, the row sums, the padded h0s);
* rounds and tiles of the persistent kernels: a one-step round followed by another, tiles of 1, 2, 3, 4, 5, 8, 9
  and 11+ steps, T = 1, B = 1, batches without a partial tile, lengths=None, batch_first;
* the step kernels' K loops with a partly empty chunk (kiter 3 and 9 at every ksplit), five batch tiles;
* which path ran, from ops.rnn_path_counts(): a "persistent" test that fell back to the step kernels fails.

Budget (asserted; tests/test_gpu_rnn_config3.py's): outputs and final states 2e-5 absolute, every gradient tensor
1e-4 of max(1, its largest reference entry).  Every test prints the figures it asserts on as one JSON line (output,
states, dx, worst parameter gradient, dh0, dc0, each in units of its bound's scale); the worst of them per path are
NOT recorded here yet: this file has not run on an MI355X so far.  For scale, tests/test_gpu_rnn_long.py measures
outputs 5e-7 .. 9e-7 and gradients 6e-7 .. 3e-6 with the same kernels at H = 512.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rnn_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

CELLS = ["LSTM", "GRU"]


def _set_env(monkeypatch, case, persistent):
    monkeypatch.setenv("ITTS_RNN_PERSISTENT", "1" if persistent else "0")      # the library reads it per call
    monkeypatch.delenv("ITTS_RNN_PAD_HIDDEN", raising=False)
    for k, v in case.env:
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("path", ["persistent", "steps"])
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", rc.CASES_512, ids=lambda c: c.name)
def test_hidden_512_edges_match_torch_float64(gpu, monkeypatch, case, cell, path):
    _set_env(monkeypatch, case, path == "persistent")
    rc.compare(case, cell, gpu, path=path)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", rc.CASES_WIDTHS, ids=lambda c: c.name)
def test_step_kernel_k_loops_match_torch_float64(gpu, monkeypatch, case, cell):
    """H = 48, 96, 288, 576 at their own width: the persistent launch declines (H != 512) with the switch left on"""
    _set_env(monkeypatch, case, True)
    rc.compare(case, cell, gpu, path="steps")


@pytest.mark.parametrize("cell", CELLS)
def test_padded_hidden_size_with_initial_states_matches_torch_float64(gpu, monkeypatch, cell):
    """H = 256 zero-padded to 512 (nn/modules.py, _pad_hidden pads the initial states too) on the persistent kernels"""
    _set_env(monkeypatch, rc.CASE_PADDED, True)
    rc.compare(rc.CASE_PADDED, cell, gpu, path="persistent")


@pytest.mark.parametrize("nonlinearity", ["tanh", "relu"])
def test_vanilla_rnn_matches_torch_float64(gpu, nonlinearity):
    rc.compare(rc.CASE_RNN, "RNN", gpu, kwargs=(("nonlinearity", nonlinearity),))


def _small(cell, gpu, B=3, T=5, H=16):
    from idiaptts_amd import nn as inn
    torch.manual_seed(5)
    layer = getattr(inn, cell)(8, H, 2, bidirectional=True).to(gpu)
    x = torch.randn(T, B, 8, device=gpu, requires_grad=True)
    lens = torch.tensor([T, 2, 4][:B], dtype=torch.int64)
    shared = [torch.randn(4, 1, H, device=gpu) * 0.3 for _ in range(2 if cell == "LSTM" else 1)]
    return layer, x, lens, shared


@pytest.mark.parametrize("cell", CELLS)
def test_per_row_initial_states_are_refused_and_a_copy_of_an_expanded_state_is_taken(gpu, cell):
    layer, x, lens, shared = _small(cell, gpu)
    as_hx = (lambda s: tuple(s)) if cell == "LSTM" else (lambda s: s[0])
    expanded = [s.expand(-1, 3, -1) for s in shared]
    copies = [s.contiguous() for s in expanded]                        # materialised: stride(1) != 0, rows equal
    assert all(c.stride(1) != 0 for c in copies)
    out_e, st_e = layer(x, as_hx(expanded), lens)
    out_c, st_c = layer(x, as_hx(copies), lens)
    assert torch.equal(out_e, out_c)
    for a, b in zip(st_e if cell == "LSTM" else [st_e], st_c if cell == "LSTM" else [st_c]):
        assert torch.equal(a, b)
    for which in range(len(shared)):
        rows = [c.clone() for c in copies]
        rows[which][1, 2, 3] += 0.5                                    # one row of one layer / direction differs
        with pytest.raises(NotImplementedError, match="initial states"):
            layer(x, as_hx(rows), lens)


@pytest.mark.parametrize("cell,state", [("LSTM", 0), ("LSTM", 1), ("GRU", 0)])
def test_a_loss_on_the_final_states_is_refused_in_backward(gpu, cell, state):
    layer, x, lens, _ = _small(cell, gpu)
    out, st = layer(x, None, lens)
    final = st[state] if cell == "LSTM" else st
    assert final.requires_grad
    with pytest.raises(NotImplementedError, match="final state"):
        (out.sum() + final.sum()).backward()
    out, st = layer(x, None, lens)
    out.sum().backward()                                              # the output alone is fine
    assert x.grad is not None
