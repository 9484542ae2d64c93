"""The case table of tests/test_gpu_rnn_edges.py and its comparison routine (tests/test_rnn_cases.py proves, from
the lengths alone, that the table reaches what it claims).

Vocabulary (csrc/rnn_persist.h): the batch is sorted by decreasing length; a *tile* is 16 consecutive rows of it, its
*t_tile* the length of its first (longest) row -- the number of steps its workgroups run; a *round* is 8 / ndir
consecutive tiles, one launch of a persistent kernel.  The exchange buffer is cleared between rounds because a
round that is one step long leaves the tag of step 0 behind; the forward exchange has 4 step slots and the backward
exchange 2: slots wrap, and the use tag flips, at t_tile between 2 and 9 -- hence tiles of 1, 2, 3, 4, 5, 8 and 9 steps.

The reference is torch.nn.LSTM / GRU / RNN in float64 on the CPU, fed pack_padded_sequence(enforce_sorted=False).
Tolerances are those of tests/test_gpu_rnn_config3.py: 2e-5 absolute on outputs and final states (O(1) values),
1e-4 * max(1, max |ref|) on every gradient tensor."""
import collections
import functools
import json

import numpy as np
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

IN_DIM = 24
OUT_ABS = 2e-5
GRAD_REL = 1e-4
PAD_VALUE = 3.0          # what the padding of x holds: it must not matter

# name, ndir, hidden size, lengths (as written: shuffled before use), layers, batch_first, the module is handed
# lengths=None, environment of the run
Case = collections.namedtuple("Case", "name ndir H lengths layers batch_first lengths_none env")


def _case(name, ndir, lengths, H=512, layers=1, batch_first=False, lengths_none=False, env=()):
    return Case(name, ndir, H, tuple(lengths), layers, batch_first, lengths_none, tuple(env))


_RAGGED20 = [12, 12, 11, 9, 9, 8, 7, 7, 6, 5, 5, 4, 3, 3, 2, 2, 1, 1, 1, 12]      # T = 12, a second tile of 4 rows

# ---- H = 512: both kernel families
CASES_512 = [
    # t_tile 11, 4, 3, 2, then 1; three rounds: the second (rows 64..127) is one step long and a third (5 rows) follows
    _case("short_tiles", 2, [11, 9, 9, 7] + [5] * 12 + [4] * 16 + [3] * 16 + [2] * 16 + [1] * 69),
    # one round, t_tile 9 / 8 / 5 / 4
    _case("mid_tiles", 2, [9] * 16 + [8] * 16 + [5] * 16 + [4] * 3),
    # 9 tiles in one direction: a full round of 8 tiles, then a round of one row of length 1
    _case("unidir_two_rounds", 1, [21] * 2 + list(range(20, 2, -1)) * 7 + [1]),
    _case("full_round", 2, [6] * 64, batch_first=True, lengths_none=True),
    _case("one_frame", 2, [1] * 70),                                   # two one-step rounds
    _case("one_frame_one_row", 1, [1]),                                # B = 1, T = 1
    _case("single_row_1dir", 1, [13]),
    _case("single_row_2dir", 2, [13]),
    _case("exact_tile", 2, (list(range(10, 0, -1)) * 2)[:16]),
    _case("unidir_full", 1, (list(range(7, 0, -1)) * 19)[:128]),       # exactly one full round, no partial tile
    _case("two_layers_states", 2, _RAGGED20, layers=2),
]

# ---- other widths, on the step kernels at the layer's own width
_NO_PAD = (("ITTS_RNN_PAD_HIDDEN", "0"),)
WIDTH_LENGTHS = [13, 13, 9, 4, 1, 1, 2] * 3
CASES_WIDTHS = [_case("width_%d" % H, 2, WIDTH_LENGTHS, H=H, env=_NO_PAD) for H in (48, 96, 288, 576)] + [
    # five tiles in one direction: the NT = 4 instantiation of the forward step kernel makes a second pass
    _case("width_576_five_tiles", 1, [6, 5, 4, 3, 2, 1, 1] * 10, H=576, env=_NO_PAD)]

# (ksplit, kiter) of the forward and of the backward step kernel these widths are meant to reach (rnn_step.h:
# the forward K loop runs kiter steps in chunks of 8 with `c + s < kiter` guards, so 3 and 9 leave a chunk partly empty)
STEP_SPLITS = {
    48: {"LSTM": ((1, 3), (4, 3)), "GRU": ((1, 3), (3, 3))},
    96: {"LSTM": ((2, 3), (8, 3)), "GRU": ((2, 3), (6, 3))},
    288: {"LSTM": ((2, 9), (8, 9)), "GRU": ((2, 9), (6, 9))},
    576: {"LSTM": ((4, 9), (16, 9)), "GRU": ((4, 9), (12, 9))},
}

# ---- a hidden size that runs zero-padded to 512 on the persistent kernels, with initial states
CASE_PADDED = _case("padded_256", 2, _RAGGED20, H=256, env=(("ITTS_RNN_PAD_HIDDEN", "1"),))

# ---- vanilla RNN (no recurrence kernel of its own: one fused GEMM launch per step)
CASE_RNN = _case("rnn_40", 2, [14, 14, 13, 11, 10, 9, 9, 8, 7, 6, 5, 5, 4, 3, 2, 2, 1, 1, 14], H=40, layers=2)

ALL_CASES = {c.name: c for c in CASES_512 + CASES_WIDTHS + [CASE_PADDED, CASE_RNN]}


def case_lengths(case):
    """The lengths in the order the batch is built in: shuffled with a fixed seed, so that the sort is exercised."""
    order = np.random.default_rng(len(case.lengths) * 131 + case.ndir).permutation(len(case.lengths))
    return [case.lengths[i] for i in order]


def tiles(case):
    """(t_tile of every tile, rows of the last tile, rounds as lists of t_tile), from the lengths alone"""
    srt = sorted(case.lengths, reverse=True)
    t_tiles = [srt[i] for i in range(0, len(srt), 16)]
    per_round = 8 // case.ndir
    rounds = [t_tiles[i:i + per_round] for i in range(0, len(t_tiles), per_round)]
    return t_tiles, len(srt) - 16 * (len(t_tiles) - 1), rounds


Reference = collections.namedtuple(
    "Reference", "state lens x w h0 c0 out hn cn dx grads dh0 dc0 kwargs")


def _new_module(namespace, cell, case, kwargs):
    return getattr(namespace, cell)(IN_DIM, case.H, case.layers, bidirectional=case.ndir == 2,
                                    batch_first=case.batch_first, **dict(kwargs))


def _padded_mask(lens, T, batch_first):
    valid = torch.arange(T)[:, None] < torch.as_tensor(lens)[None, :]          # [T, B]
    return valid.t() if batch_first else valid


@functools.lru_cache(maxsize=None)
def reference(case_name, cell, kwargs=()):
    """The float64 side of one (case, cell), computed once and shared by the tests of both paths (its tensors are
    never written again): parameters drawn by this package's own module on the CPU, inputs, and what
    torch.nn.<cell>.double() makes of them."""
    from idiaptts_amd import nn as inn
    case = ALL_CASES[case_name]
    lens = case_lengths(case)
    B, T, D = len(lens), max(lens), case.ndir * case.H
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(sum(map(ord, case_name + cell)))
        state = {k: v.detach().clone() for k, v in _new_module(inn, cell, case, kwargs).state_dict().items()}
        x = torch.randn(T, B, IN_DIM)
        w = torch.randn(T, B, D)
        h0 = torch.randn(case.layers * case.ndir, 1, case.H) * 0.3
        c0 = torch.randn(case.layers * case.ndir, 1, case.H) * 0.3 if cell == "LSTM" else None
    x[~_padded_mask(lens, T, False)] = PAD_VALUE
    if case.batch_first:
        x, w = x.transpose(0, 1).contiguous(), w.transpose(0, 1).contiguous()
    ref = _new_module(torch.nn, cell, case, kwargs).double()
    ref.load_state_dict({k: v.double() for k, v in state.items()})
    xr = x.double().requires_grad_(True)
    h0r = h0.double().requires_grad_(True)
    c0r = c0.double().requires_grad_(True) if c0 is not None else None
    hx = h0r.expand(-1, B, -1)
    if c0r is not None:
        hx = (hx, c0r.expand(-1, B, -1))
    out_p, st = ref(pack_padded_sequence(xr, torch.tensor(lens), batch_first=case.batch_first, enforce_sorted=False),
                    hx)
    out, _ = pad_packed_sequence(out_p, batch_first=case.batch_first, total_length=T)
    (out * w.double()).sum().backward()
    hn, cn = (st[0], st[1]) if cell == "LSTM" else (st, None)
    return Reference(state, lens, x, w, h0, c0, out.detach(), hn.detach(), cn.detach() if cn is not None else None,
                     xr.grad, {n: p.grad for n, p in ref.named_parameters()}, h0r.grad,
                     c0r.grad if c0r is not None else None, kwargs)


def _abs_err(got, want):
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    return (got.detach().cpu().double() - want).abs().max().item()


def _grad_err(got, want):
    """error of a gradient tensor in units of max(1, max |ref|): the bound is GRAD_REL"""
    assert got is not None, "no gradient arrived"
    return _abs_err(got, want) / max(1.0, want.abs().max().item())


def compare(case, cell, device, path=None, kwargs=()):
    """Runs this package's <cell> on `device` in training mode and under torch.no_grad() and checks both against
    reference(): output, h_n, c_n, dx, every parameter gradient, dh0 and dc0; the inference results equal the
    training-mode ones bit for bit and hold exact zeros in the padding.  path "persistent" / "steps": the counts of
    ops.rnn_path_counts() must have moved by exactly the layer calls made, on that path.  (The caller has set the
    environment.)  Returns the figures it asserted on."""
    from idiaptts_amd import nn as inn
    from idiaptts_amd import ops
    r = reference(case.name, cell, kwargs)
    B, T = len(r.lens), max(r.lens)
    mine = _new_module(inn, cell, case, kwargs)
    mine.load_state_dict(r.state)
    mine = mine.to(device)
    lens_arg = None if case.lengths_none else torch.tensor(r.lens, dtype=torch.int64)
    x = r.x.to(device).requires_grad_(True)
    h0 = r.h0.to(device).requires_grad_(True)
    c0 = r.c0.to(device).requires_grad_(True) if r.c0 is not None else None

    def states():
        h = h0.expand(-1, B, -1)
        return (h, c0.expand(-1, B, -1)) if c0 is not None else h

    before = ops.rnn_path_counts()
    out, st = mine(x, states(), lens_arg)
    (out * r.w.to(device)).sum().backward()
    with torch.no_grad():
        out_i, st_i = mine(x.detach(), states(), lens_arg)
    torch.cuda.synchronize()
    after = ops.rnn_path_counts()
    hn, cn = (st[0], st[1]) if cell == "LSTM" else (st, None)
    hn_i, cn_i = (st_i[0], st_i[1]) if cell == "LSTM" else (st_i, None)

    fig = {"case": case.name, "cell": cell, "path": path}
    fig["out"] = _abs_err(out, r.out)
    fig["states"] = max(_abs_err(hn, r.hn), _abs_err(cn, r.cn) if cn is not None else 0.0)
    fig["out_inference"] = _abs_err(out_i, r.out)
    fig["states_inference"] = max(_abs_err(hn_i, r.hn), _abs_err(cn_i, r.cn) if cn_i is not None else 0.0)
    fig["dx"] = _grad_err(x.grad, r.dx)
    per_param = {n: _grad_err(p.grad, r.grads[n]) for n, p in mine.named_parameters()}
    fig["params"] = max(per_param.values())
    fig["dh0"] = _grad_err(h0.grad, r.dh0)
    if c0 is not None:
        fig["dc0"] = _grad_err(c0.grad, r.dc0)
    print(json.dumps(fig))

    if path is not None:
        moved = [a - b for a, b in zip(after, before)]
        fwd_calls, bwd_calls = 2 * case.layers, case.layers       # forward in both modes, backward in training
        want = [fwd_calls, 0, 0, bwd_calls, 0, 0] if path == "persistent" else [0, fwd_calls, 0, 0, bwd_calls, 0]
        if path == "persistent" and moved != want:
            raise AssertionError("the persistent recurrence did not run every layer call: the layer fell back to the "
                                 "step kernels (ran / declined / gave_up moved by forward {}, backward {}; expected "
                                 "forward {}, backward {})".format(moved[:3], moved[3:], want[:3], want[3:]))
        assert moved == want, "step path expected: ran / declined / gave_up moved by {}, expected {}".format(moved,
                                                                                                             want)
    for k in ("out", "states", "out_inference", "states_inference"):
        assert fig[k] < OUT_ABS, (k, fig)
    assert fig["dx"] < GRAD_REL, fig
    for n, e in per_param.items():
        assert e < GRAD_REL, (n, e, fig)
    assert fig["dh0"] < GRAD_REL, fig
    assert fig.get("dc0", 0.0) < GRAD_REL, fig
    # same kernel, same arithmetic: only the stores of the saved tensors differ
    assert torch.equal(out_i, out.detach()), "inference output differs from the training-mode forward"
    assert torch.equal(hn_i, hn.detach()), "inference h_n differs from the training-mode forward"
    if cn is not None:
        assert torch.equal(cn_i, cn.detach()), "inference c_n differs from the training-mode forward"
    pad = ~_padded_mask(r.lens, T, case.batch_first)
    assert not out_i.cpu()[pad].any(), "inference output is not exactly 0 in the padding"
    assert not out.detach().cpu()[pad].any(), "training output is not exactly 0 in the padding"
    return fig
