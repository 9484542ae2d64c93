"""csrc/xent.hip on the GPU, through `ops` (the ctypes binding of the C ABI), against the float64 restatement in
xent_cases.py (pinned to torch in float64 by tests/test_xent_config.py): every width class of the class-contiguous
form and its edges at 1, 2, 7 and 69 rows, the class-strided form with every shift, the named hazards, an
out-of-range target, determinism, and the class counts against torch.argmax and numpy.add.at."""
import numpy as np
import pytest
import torch

import xent_cases as xc
from idiaptts_amd import lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _call(x, t, w, cw=None, **kw):
    return ops.softmax_xent(x.to(DEV), t.to(DEV), w.to(DEV), None if cw is None else cw.to(DEV), xc.IGNORE, **kw)


def _check_all(got, ref, case=None, t32=None):
    loss, grad, elem = got
    k = {} if t32 is None else dict(case=case)
    xc.check("elem", elem, ref["elem"], torch32=None if t32 is None else t32["elem"], **k)
    xc.check("grad", grad, ref["grad"], torch32=None if t32 is None else t32["grad"], **k)
    xc.check("loss", loss, ref["loss"], torch32=None if t32 is None else t32["loss"], **k)


# ---- class-contiguous rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", xc.ROWS_C)
@pytest.mark.parametrize("N", xc.ROWS_N)
def test_rows_sweep(N, C):
    assert ops.xent_plan(N, C, "rows") == xc.expected_plan(C)
    x, t, cw, w = xc.rows_inputs(torch, N, C)
    # without and with class weights
    base = _call(x, t, w, want_elem=True)
    _check_all(base, xc.reference64(torch, x, t, None, w))
    _check_all(_call(x, t, w, cw, want_elem=True), xc.reference64(torch, x, t, cw, w))
    # rows whose target is ignore_index: loss 0, gradient 0
    ti = t.clone()
    ti[::3] = xc.IGNORE
    got = _call(x, ti, w, cw, want_elem=True)
    _check_all(got, xc.reference64(torch, x, ti, cw, w))
    assert got[2].cpu()[::3].abs().max() == 0 and got[1].cpu()[::3].abs().max() == 0
    # gradient absent, per-row values absent: the same bits where they are present
    l1, g1, e1 = _call(x, t, w, want_grad=False, want_elem=True)
    assert g1 is None and _same_bits(l1, base[0]) and _same_bits(e1, base[2])
    l2, g2, e2 = _call(x, t, w, want_elem=False)
    assert e2 is None and _same_bits(l2, base[0]) and _same_bits(g2, base[1])


@pytest.mark.parametrize("C", (1, 3, 5, 17, 64, 65, 257, 4096))
@pytest.mark.parametrize("N", (2, 7, 69))
def test_rows_of_weight_zero_may_hold_anything(N, C):
    x, t, cw, w = xc.rows_inputs(torch, N, C, seed=1)
    dead = torch.arange(N) % 3 == 1
    w0 = torch.where(dead, torch.zeros_like(w), w)
    clean = _call(x, t, w0, cw, want_elem=True)
    xd, td = x.clone(), t.clone()
    xd[dead] = float("nan")
    xd[dead, 0] = float("inf")
    td[dead] = C + 5                      # out of range, and never used as an index
    td[1] = -7
    dirty = _call(xd, td, w0, cw, want_elem=True)
    for a, b in zip(clean, dirty):
        assert _same_bits(a, b)
    assert bool(torch.isfinite(dirty[0]).all())
    assert dirty[1].cpu()[dead].abs().max() == 0 and dirty[2].cpu()[dead].abs().max() == 0
    _check_all(dirty, xc.reference64(torch, x, t, cw, w0))


@pytest.mark.parametrize("N,C,pitch", [(7, 5, 7), (7, 64, 67), (7, 65, 68), (5, 257, 261), (3, 1024, 1028),
                                       (69, 17, 17)])
def test_pitched_misaligned_rows(N, C, pitch):
    """pitch > C (or a pitch that is no multiple of 4 floats) and a base 4 bytes off the 16-byte grid: the plain-load
    form.  The sentinels around d_grad stay untouched and the bits are those of the aligned call."""
    x, t, cw, w = xc.rows_inputs(torch, N, C, seed=2)
    aligned = _call(x, t, w, cw, want_elem=True)
    sentinel = 12345.0
    xbuf = torch.full((N * pitch + 8,), sentinel, device=DEV)
    gbuf = torch.full((N * pitch + 8,), sentinel, device=DEV)
    xv = xbuf.as_strided((N, C), (pitch, 1), 1)
    gv = gbuf.as_strided((N, C), (pitch, 1), 1)
    assert xv.data_ptr() % 16 == 4 and gv.data_ptr() % 16 == 4
    xv.copy_(x)
    loss, grad, elem = ops.softmax_xent(xv, t.to(DEV), w.to(DEV), cw.to(DEV), xc.IGNORE, want_elem=True, grad=gv)
    assert grad.data_ptr() == gv.data_ptr()
    assert _same_bits(loss, aligned[0]) and _same_bits(elem, aligned[2]) and _same_bits(gv, aligned[1])
    inside = torch.zeros(N * pitch + 8, dtype=torch.bool)
    inside.as_strided((N, C), (pitch, 1), 1).fill_(True)
    assert bool((gbuf.cpu()[~inside] == sentinel).all()), "the kernel wrote outside the gradient's rows"
    assert bool((xbuf.cpu()[~inside] == sentinel).all())


# ---- class-strided ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", xc.SHIFTS)
@pytest.mark.parametrize("T", xc.STRIDED_T)
@pytest.mark.parametrize("C", xc.STRIDED_C)
def test_strided_sweep(C, T, shift):
    B = xc.STRIDED_B
    x, onehot, idx, cw = xc.strided_inputs(torch, B, C, T)
    if (shift or 0) >= T:
        w = torch.ones(B * T)
        with pytest.raises((lib.IttsError, ValueError), match="shift = {}".format(shift)):
            ops.softmax_xent_strided(x.to(DEV), onehot.to(DEV), w.to(DEV), shift=shift)
        L = lib.load()
        p = lambda v: v.data_ptr()
        xd, od, wd = x.to(DEV), onehot.to(DEV), w.to(DEV)
        out = torch.zeros(1, device=DEV)
        assert L.itts_softmax_xent_strided(p(xd), p(od), None, p(wd), B, C, T, shift, xc.IGNORE, p(out), None, None,
                                           p(wd), None) == -1
        assert "shift = {}".format(shift) in L.itts_last_error().decode()
        return
    assert ops.xent_plan(B * T, C, "strided") == xc.expected_strided_plan(C)
    Tn = T - (shift or 0)
    g = torch.Generator().manual_seed(5 + T)
    w = 0.5 + torch.rand(B, Tn, generator=g)
    w[0, Tn // 2] = 0.0                       # a masked frame
    for weights in (None, cw):
        ref = xc.reference64_strided(torch, x, onehot, weights, w, xc.IGNORE, shift)
        assert torch.equal(ref["target"], idx[:, (shift or 0):])
        got = ops.softmax_xent_strided(x.to(DEV), onehot.to(DEV), w.to(DEV),
                                       None if weights is None else weights.to(DEV), xc.IGNORE, shift, want_elem=True)
        assert got[1].shape == (B, C, T) and got[2].shape == (B, Tn)
        _check_all(got, ref)
        if shift:
            assert got[1].cpu()[:, :, Tn:].abs().max() == 0
        assert got[1].cpu()[0, :, Tn // 2].abs().max() == 0 and got[2].cpu()[0, Tn // 2] == 0
    # evaluation: no gradient, the same loss bits; and ignore_index on the arg-max's class
    l1, g1, _ = ops.softmax_xent_strided(x.to(DEV), onehot.to(DEV), w.to(DEV), cw.to(DEV), xc.IGNORE, shift,
                                         want_grad=False)
    assert g1 is None and _same_bits(l1, got[0])
    ign = int(idx[1, shift or 0])
    ref = xc.reference64_strided(torch, x, onehot, cw, w, ign, shift)
    _check_all(ops.softmax_xent_strided(x.to(DEV), onehot.to(DEV), w.to(DEV), cw.to(DEV), ign, shift,
                                        want_elem=True), ref)


def test_strided_target_ties_take_the_lowest_index():
    B, C, T = 3, 5, 65
    x, onehot, idx, cw = xc.strided_inputs(torch, B, C, T, seed=3)
    soft = torch.zeros(B, C, T)
    soft[:, 3, :] = 0.5
    soft[:, 1, :] = 0.5                       # two equal maxima: class 1 wins
    soft[2, 4, :] = 0.5                       # three
    soft[1, 0, 7] = 0.5
    ref = xc.reference64_strided(torch, x, soft, cw, None, xc.IGNORE, 1)
    assert torch.equal(ref["target"], soft.max(dim=1)[1][:, 1:])
    assert int(ref["target"][0, 0]) == 1 and int(ref["target"][1, 6]) == 0
    w = torch.ones(B, T - 1)
    _check_all(ops.softmax_xent_strided(x.to(DEV), soft.to(DEV), w.to(DEV), cw.to(DEV), xc.IGNORE, 1,
                                        want_elem=True), ref)


# ---- hazards ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", xc.HAZARDS)
def test_hazards(name):
    x, t = xc.hazard_inputs(torch, name)
    N, C = x.shape
    w = torch.ones(N)
    ref = xc.reference64(torch, x, t, None, w)
    t32 = xc.torch32(torch, x, t)
    got = _call(x, t, w, want_elem=True)
    for v in got:
        assert bool(torch.isfinite(v).all()), name
    _check_all(got, ref, case=name, t32=t32)
    loss, grad, elem = (v.cpu() for v in got)
    if name == "C1":
        assert elem.abs().max() == 0 and grad.abs().max() == 0 and loss.item() == 0
    if name == "all_equal":
        assert _same_bits(elem, elem[:1].expand(N)) and abs(elem[0].item() / np.log(C) - 1) < 3e-7
    if name == "neg_inf_logit":
        hit = torch.isinf(x)
        assert int(hit.sum()) == N and grad[hit].abs().max() == 0
    if name == "confident":
        assert 0 < elem.min() and elem.max() < 1e-2
    # the strided form on the same rows ([1, C, N]): the same hazards
    soft = torch.zeros(1, C, N).scatter_(1, t[None, None, :], 1.0)
    xs = x.t().contiguous()[None]
    gs = ops.softmax_xent_strided(xs.to(DEV), soft.to(DEV), w.to(DEV), None, xc.IGNORE, None, want_elem=True)
    sref = dict(elem=ref["elem"], loss=ref["loss"], grad=ref["grad"].t().contiguous())
    s32 = dict(elem=t32["elem"], loss=t32["loss"], grad=t32["grad"].t().contiguous())
    _check_all(gs, sref, case=name, t32=s32)


def test_out_of_range_target_on_a_live_row():
    """loss NaN, gradient row zeros, every other row unchanged; one call"""
    N, C = 7, 17
    x, t, cw, w = xc.rows_inputs(torch, N, C, seed=4)
    good = _call(x, t, w, cw, want_elem=True)
    tb = t.clone()
    tb[3] = C                                 # one past the last class
    loss, grad, elem = (v.cpu() for v in _call(x, tb, w, cw, want_elem=True))
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(elem[3]))
    assert grad[3].abs().max() == 0
    keep = torch.arange(N) != 3
    assert _same_bits(grad[keep], good[1].cpu()[keep]) and _same_bits(elem[keep], good[2].cpu()[keep])


# ---- determinism ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (3, 5, 64, 65, 257, 1025))
def test_bits_repeat_and_a_row_depends_on_the_row_alone(C):
    x69, t69, cw, w69 = xc.rows_inputs(torch, 69, C, seed=5)
    row, trow, wrow = x69[11:12], t69[11:12], w69[11:12]
    alone = _call(row, trow, wrow, cw, want_elem=True)
    again = _call(row, trow, wrow, cw, want_elem=True)
    for a, b in zip(alone, again):
        assert _same_bits(a, b)
    for N in (7, 69):
        x, t, w = x69[:N].clone(), t69[:N].clone(), w69[:N].clone()
        x[5], t[5], w[5] = row[0], trow[0], wrow[0]
        first = _call(x, t, w, cw, want_elem=True)
        second = _call(x, t, w, cw, want_elem=True)
        for a, b in zip(first, second):
            assert _same_bits(a, b)
        assert _same_bits(first[1][5], alone[1][0]) and _same_bits(first[2][5], alone[2][0])


def test_empty_call_writes_a_zero_loss():
    loss, grad, elem = ops.softmax_xent(torch.empty(0, 5, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV),
                                        torch.empty(0, device=DEV), want_elem=True)
    assert loss.item() == 0.0 and grad.shape == (0, 5) and elem.shape == (0,)
    loss, grad, elem = ops.softmax_xent_strided(torch.empty(0, 5, 9, device=DEV), torch.empty(0, 5, 9, device=DEV),
                                                torch.empty(0, device=DEV), shift=1, want_elem=True)
    assert loss.item() == 0.0 and grad.shape == (0, 5, 9)


# ---- arg-max and confusion counts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (1, 2, 3, 5, 17, 63, 64, 65, 256, 257, 1024))
@pytest.mark.parametrize("N", (1, 7, 69))
def test_class_counts(N, C):
    x, t, _, _ = xc.rows_inputs(torch, N, C, seed=6)
    if C > 1:
        x[0, C // 2] = x[0].max() + 1
        x[0, C - 1] = x[0, C // 2]            # a tie: the lower index
        if N > 1:
            x[1, C - 1] = float("nan")        # a NaN beats every number; the first NaN
            x[1, C // 3] = float("nan")
    expect = torch.argmax(x, dim=-1)
    assert torch.equal(expect, xc.first_argmax(torch, x, -1))
    if C > 1:
        assert int(expect[0]) == C // 2 and (N == 1 or int(expect[1]) == C // 3)
    t[-1] = expect[-1]                        # at least one correct row
    pred, correct, conf = ops.class_counts(x.to(DEV), t.to(DEV))
    assert pred.dtype == torch.int64 and torch.equal(pred.cpu(), expect)
    ref_conf, ref_correct = xc.confusion64(expect.numpy(), t.numpy(), C)
    assert correct.item() == ref_correct and np.array_equal(conf.cpu().numpy(), ref_conf)
    # a second batch adds onto the first; a target outside [0, C) is counted nowhere
    x2, t2, _, _ = xc.rows_inputs(torch, N, C, seed=7)
    t2[0] = C
    _, correct, conf = ops.class_counts(x2.to(DEV), t2.to(DEV), want_pred=False, correct=correct, conf=conf)
    c2, n2 = xc.confusion64(torch.argmax(x2, dim=-1).numpy(), t2.numpy(), C)
    assert correct.item() == ref_correct + n2 and np.array_equal(conf.cpu().numpy(), ref_conf + c2)
    assert int(conf.sum()) == 2 * N - 1
    # predictions alone
    pred, correct, conf = ops.class_counts(x.to(DEV))
    assert correct is None and conf is None and torch.equal(pred.cpu(), expect)


def test_class_counts_pitched_rows_and_the_cap():
    N, C = 9, 67
    x, t, _, _ = xc.rows_inputs(torch, N, C, seed=8)
    wide = torch.full((N, C + 5), 1e9, device=DEV)
    wide[:, :C] = x.to(DEV)
    pred, _, _ = ops.class_counts(wide[:, :C], t.to(DEV))
    assert torch.equal(pred.cpu(), torch.argmax(x, dim=-1))
    x = torch.randn(2, 1025, device=DEV)
    with pytest.raises(ValueError, match="C = 1025"):
        ops.class_counts(x, torch.zeros(2, dtype=torch.int64, device=DEV))
    assert torch.equal(ops.class_counts(x)[0].cpu(), torch.argmax(x.cpu(), dim=-1))
