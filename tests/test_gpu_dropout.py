"""Dropout fused into the dense layers (csrc/dropout.h) on the GPU, against the numpy restatement of the rule
(dropout_spec.py): the mask bit for bit, the forward products against their undropped selves bit for bit, the input
gradient against float64 at the dense layers' bounds, p = 0 against the plain entry points, the flat step, the
module path and the trainer."""
import os
import types

import numpy as np
import pytest
import torch

from dropout_spec import chain_backward, chain_forward, keep_mask, masked_mse, scale_f32
from gemm_harness import check_out_frame, flat_in, frame_in, frame_out
from lnorm_cases import check
from idiaptts_amd import ops
from idiaptts_amd.native_ff import FlatFFModel

pytestmark = pytest.mark.gpu

ACT_NAMES = {ops.ACT_NONE: None, ops.ACT_TANH: "tanh", ops.ACT_SIGMOID: "sigmoid"}
SEED = 0x1234567890abcdef
BIG = 2 ** 32 - 3            # a row offset at which the counter's row word carries over inside the matrix


def _bits(t):
    return t.contiguous().view(torch.int32)


def _mask(M, N, p, seed, salt, row_offset=0, dev=None):
    m = torch.from_numpy(keep_mask(M, N, p, seed, salt, row_offset))
    return m if dev is None else m.to(dev)


# ------------------------------------------------------------------------------------------------ the mask
@pytest.mark.parametrize("row_offset", [0, BIG])
def test_mask_equals_the_restatement(gpu, row_offset):
    for M in (1, 63, 65, 301):
        for N in (1, 3, 4, 5, 97, 187, 512):
            got = ops.dropout_mask(M, N, 0.3, SEED, 5, row_offset, device=gpu)
            assert got.dtype == torch.bool and got.shape == (M, N)
            assert torch.equal(got.cpu(), _mask(M, N, 0.3, SEED, 5, row_offset)), (M, N, row_offset)


@pytest.mark.parametrize("p", [0.0, 2.0 ** -32, 0.5, 0.9, 1.0 - 2.0 ** -33])
def test_mask_at_the_threshold_edges(gpu, p):
    got = ops.dropout_mask(65, 97, p, 3, 1, device=gpu).cpu()
    assert torch.equal(got, _mask(65, 97, p, 3, 1))
    if p == 0.0:
        assert bool(got.all())


def test_elementwise_pitched_and_in_place(gpu):
    g = torch.Generator().manual_seed(3)
    for M, N in ((65, 97), (301, 5), (63, 512), (1, 1)):
        x = torch.randn(M, N, generator=g)
        m = _mask(M, N, 0.4, SEED, 2, BIG)
        want = torch.where(m, x * float(scale_f32(0.4)), torch.zeros(()))
        xin, xv = frame_in(x, "u", gpu)          # a pitch and a base off the 16-byte grid
        out, ov = frame_out(M, N, "v", gpu)
        before = xin.clone()
        ops.dropout_apply(xv, 0.4, SEED, 2, BIG, out=ov)
        assert torch.equal(_bits(ov.cpu()), _bits(want)), (M, N)           # +0.0 where dropped, also for x < 0
        assert torch.equal(_bits(xin), _bits(before))
        check_out_frame(out, N, "v", False, ("apply", M, N))
        # in place, inside a frame that must stay as it is
        buf, v = frame_out(M, N, "u", gpu)
        v.copy_(x.to(gpu))
        assert ops.dropout_apply(v, 0.4, SEED, 2, BIG, out=v) is v
        assert torch.equal(_bits(v.cpu()), _bits(want))
        check_out_frame(buf, N, "u", False, ("apply in place", M, N))
        # the default output keeps 16-byte rows with zero pad columns
        y = ops.dropout_apply(xv, 0.4, SEED, 2, BIG)
        assert torch.equal(_bits(y.cpu()), _bits(want)) and y.stride(0) % 4 == 0


def test_a_rows_mask_does_not_depend_on_its_place(gpu):
    whole = ops.dropout_mask(17, 187, 0.5, SEED, 1, 1000, device=gpu)
    alone = ops.dropout_mask(1, 187, 0.5, SEED, 1, 1016, device=gpu)
    assert torch.equal(whole[16:], alone)
    g = torch.Generator().manual_seed(4)
    x, w, b = torch.rand(17, 32, generator=g).to(gpu), (torch.rand(187, 32, generator=g) - 0.5).to(gpu), None
    yw = ops.linear_fwd_dropout(x, w, b, ops.ACT_TANH, p=0.5, seed=SEED, salt=1, row_offset=1000)
    ya = ops.linear_fwd_dropout(x[16:], w, b, ops.ACT_TANH, p=0.5, seed=SEED, salt=1, row_offset=1016)
    assert torch.equal((yw[16:] != 0), (ya != 0)) and torch.equal((ya != 0), alone)


# --------------------------------------------------------------------------------------------- the forward
def _one(plan):
    assert len(plan) == 1, plan
    return plan[0]


@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_TANH, ops.ACT_SIGMOID])
@pytest.mark.parametrize("kernel", ["ring", "staged"])
def test_forward_is_the_plain_forward_under_the_mask(gpu, kernel, act):
    lay = "v" if kernel == "ring" else "u"
    p, salt = 0.3, 1
    scale = float(scale_f32(p))
    g = torch.Generator().manual_seed(11 + act)
    for M in (65, 301):
        for K in (13, 32):
            for N in (32, 97, 187):
                # K = 13 as the flat model holds it: rows of 16 floats, the pad columns of x and w zero
                Kp = (K + 3) // 4 * 4
                x, w = torch.zeros(M, Kp), torch.zeros(N, Kp)
                x[:, :K] = 1.0 - torch.rand(M, K, generator=g)
                w[:, :K] = (torch.rand(N, K, generator=g) - 0.5) * (2.0 / K ** 0.5)
                b = torch.rand(N, generator=g) - 0.5
                (xb, xv), (wb, wv), (bb, bv) = frame_in(x, lay, gpu), flat_in(w, lay, gpu), flat_in(b, lay, gpu)
                before = [t.clone() for t in (xb, wb, bb)]
                plain, pv = frame_out(M, N, lay, gpu)
                drop, dv = frame_out(M, N, lay, gpu)
                ops.linear_fwd(xv, wv, bv, act, out=pv)
                e0 = _one(ops.gemm_last_plan())
                ops.linear_fwd_dropout(xv, wv, bv, act, p=p, seed=SEED, salt=salt, row_offset=BIG, out=dv)
                e1 = _one(ops.gemm_last_plan())
                what = (kernel, act, M, K, N)
                assert e1.kernel == kernel and e1.epi == "bias_act" and e1.dropout and not e0.dropout, (what, e0, e1)
                assert e1._replace(dropout=False, grouped=e0.grouped) == e0, (what, e0, e1)   # the same variant ran
                m = _mask(M, N, p, SEED, salt, BIG, gpu)
                got = dv.clone()
                assert bool((_bits(got)[~m] == 0).all()), (what, "a dropped element is not +0.0")
                assert torch.equal(_bits(got[m]), _bits((pv * scale)[m])), (what, "a kept element is not plain * scale")
                for t, t0 in zip((xb, wb, bb), before):
                    assert torch.equal(_bits(t), _bits(t0)), (what, "an input was written")
                check_out_frame(drop, N, lay, kernel == "ring", what)


@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_TANH, ops.ACT_SIGMOID])
def test_sparse_forward_is_its_plain_self_under_the_mask(gpu, act):
    p, salt = 0.5, 0
    scale = float(scale_f32(p))
    g = torch.Generator().manual_seed(21 + act)
    for M in (65, 301):
        for N in (32, 97, 187):
            K = 13
            x = torch.zeros(M, 16)
            x[:, :K] = (torch.rand(M, K, generator=g) < 0.2).float() * (1.0 - torch.rand(M, K, generator=g))
            x = x.to(gpu)
            w = torch.zeros(N, 16)
            w[:, :K] = (torch.rand(N, K, generator=g) - 0.5)
            w, b = w.to(gpu), (torch.rand(N, generator=g) - 0.5).to(gpu)
            lists = ops.sparse_rows_build(x)
            before = ops.sparse_path_counts()
            plain, pv = frame_out(M, N, "v", gpu)
            drop, dv = frame_out(M, N, "v", gpu)
            ops.linear_fwd_sparse(lists, x, w, b, act, out=pv)
            ops.linear_fwd_sparse_dropout(lists, x, w, b, act, p=p, seed=SEED, salt=salt, out=dv)
            after = ops.sparse_path_counts()
            assert after.fwd_sparse == before.fwd_sparse + 2 and after.fwd_dense == before.fwd_dense
            m = _mask(M, N, p, SEED, salt, 0, gpu)
            assert bool((_bits(dv.clone())[~m] == 0).all()), (M, N)
            assert torch.equal(_bits(dv[m]), _bits((pv * scale)[m])), (M, N)
            check_out_frame(drop, N, "v", True, ("sparse", act, M, N))
            # the dense kernel draws the same mask
            dense = ops.linear_fwd_dropout(x, w, b, act, p=p, seed=SEED, salt=salt)
            assert bool((dense[~m] == 0).all()) and bool((dense[m] != 0).any())


# -------------------------------------------------------------------------------------------- the backward
def _act64(z, act):
    return {None: z, "tanh": torch.tanh(z), "sigmoid": torch.sigmoid(z)}[ACT_NAMES[act]]


def _dact64(y, act):
    return {None: torch.ones_like(y), "tanh": 1 - y * y, "sigmoid": y * (1 - y)}[ACT_NAMES[act]]


@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_TANH, ops.ACT_SIGMOID])
@pytest.mark.parametrize("kernel", ["ring", "staged"])
def test_input_gradient_and_fused_backward(gpu, kernel, act):
    lay = "v" if kernel == "ring" else "u"
    p, salt = 0.3, 4
    scale = float(scale_f32(p))
    g = torch.Generator().manual_seed(31 + act)
    for M in (65, 301):
        for N, K in ((32, 32), (97, 16), (187, 96)):
            y = _act64(torch.randn(M, K, generator=g, dtype=torch.float64), act).float()     # the previous layer's output
            m = _mask(M, K, p, SEED, salt, BIG)
            d = torch.where(m, y * scale, torch.zeros(()))                                  # ... as the forward stores it
            dz = torch.rand(M, N, generator=g) - 0.25
            w = (torch.rand(N, K, generator=g) - 0.5) * (2.0 / N ** 0.5)
            ref = (dz.double() @ w.double()) * m * float(scale) * _dact64(y.double(), act)
            (zb, zv), (wb, wv), (db_, dv) = frame_in(dz, lay, gpu), flat_in(w, lay, gpu), frame_in(d, lay, gpu)
            before = [t.clone() for t in (zb, wb, db_)]
            out, ov = frame_out(M, K, lay, gpu)
            ops.linear_bwd_input_dropout(zv, wv, dv, act, p=p, seed=SEED, salt=salt, row_offset=BIG, out=ov)
            e = _one(ops.gemm_last_plan())
            what = (kernel, act, M, N, K)
            assert e.kernel == kernel and e.epi == "dact" and e.dropout, (what, e)
            got = ov.clone().cpu()
            assert bool((got[~m] == 0).all()) and bool((got[m] != 0).any()), what
            check("dx", got, ref)
            for t, t0 in zip((zb, wb, db_), before):
                assert torch.equal(_bits(t), _bits(t0)), (what, "an input was written")
            check_out_frame(out, K, lay, kernel == "ring", what)
            # both gradients in one call: dw / db are the plain call's on the same operands, dx the separate call's
            # (db right behind dw for both, as the flat gradient arenas hold them: whether one reduction serves the two
            # depends on that, and two separate allocations may or may not come out adjacent)
            (dw0, db0), (dw1, db1) = (torch.empty(N * K + N, device=gpu).split([N * K, N]) for _ in range(2))
            dw0, dw1 = dw0.view(N, K), dw1.view(N, K)
            dx0, o0 = frame_out(M, K, lay, gpu)
            dx1, o1 = frame_out(M, K, lay, gpu)
            ops.linear_bwd(zv, dv, wv, dw0, db0, o0, yprev=dv, act_prev=act)
            plan0 = ops.gemm_last_plan()
            ops.linear_bwd_dropout(zv, dv, wv, dw1, db1, o1, yprev=dv, act_prev=act, p=p, seed=SEED, salt=salt,
                                   row_offset=BIG)
            plan1 = ops.gemm_last_plan()
            assert [getattr(e, "kernel", "reduce") for e in plan0] == [getattr(e, "kernel", "reduce") for e in plan1]
            assert [e.dropout for e in plan1 if hasattr(e, "dropout")].count(True) == 1, plan1
            assert torch.equal(dw0, dw1) and torch.equal(db0, db1), what
            assert torch.equal(_bits(o1), _bits(ov)), (what, "fused and separate input gradients differ")
            check_out_frame(dx1, K, lay, kernel == "ring", what)


def test_last_layer_gradient_through_dropout_and_activation(gpu):
    g = torch.Generator().manual_seed(5)
    M, N, p = 65, 97, 0.4
    y = torch.tanh(torch.randn(M, N, generator=g))
    m = _mask(M, N, p, 9, 2)
    d = torch.where(m, y * float(scale_f32(p)), torch.zeros(()))
    dy = torch.randn(M, N, generator=g)
    got = ops.dropout_act_bwd(dy.to(gpu), d.to(gpu), ops.ACT_TANH, p, 9, 2).cpu()
    ref = dy.double() * m * float(scale_f32(p)) * (1 - y.double() ** 2)
    assert bool((got[~m] == 0).all())
    check("dx", got, ref)


def test_p_zero_is_the_plain_entry_point(gpu):
    g = torch.Generator().manual_seed(6)
    M, N, K = 301, 97, 32
    x = (torch.rand(M, K, generator=g) * (torch.rand(M, K, generator=g) < 0.3)).to(gpu)
    w, b = (torch.rand(N, K, generator=g) - 0.5).to(gpu), (torch.rand(N, generator=g) - 0.5).to(gpu)
    dz = (torch.rand(M, N, generator=g) - 0.25).to(gpu)
    rule = dict(p=0.0, seed=SEED, salt=3, row_offset=7)
    y0 = ops.linear_fwd(x, w, b, ops.ACT_TANH)
    plan0 = ops.gemm_last_plan()
    y1 = ops.linear_fwd_dropout(x, w, b, ops.ACT_TANH, **rule)
    assert ops.gemm_last_plan() == plan0 and torch.equal(y0, y1)
    lists = ops.sparse_rows_build(x)
    assert torch.equal(ops.linear_fwd_sparse(lists, x, w, b, ops.ACT_TANH),
                       ops.linear_fwd_sparse_dropout(lists, x, w, b, ops.ACT_TANH, **rule))
    dx0 = ops.linear_bwd_input(dz, w, yprev=x, act_prev=ops.ACT_TANH)
    plan0 = ops.gemm_last_plan()
    dx1 = ops.linear_bwd_input_dropout(dz, w, x, ops.ACT_TANH, **rule)
    assert ops.gemm_last_plan() == plan0 and torch.equal(dx0, dx1)
    outs = []
    for fn, kw in ((ops.linear_bwd, {}), (ops.linear_bwd_dropout, rule)):
        dw, db, dx = torch.empty(N, K, device=gpu), torch.empty(N, device=gpu), torch.empty(M, K, device=gpu)
        fn(dz, x, w, dw, db, dx, yprev=x, act_prev=ops.ACT_TANH, **kw)
        outs.append((dw, db, dx, ops.gemm_last_plan()))
    assert outs[0][3] == outs[1][3] and all(torch.equal(a, b_) for a, b_ in zip(outs[0][:3], outs[1][:3]))
    # operands that cannot take the ring kernel: the separate weight and input gradient, for p == 0 as well
    Mu, Nu, Ku = 65, 97, 16
    (_, zu), (_, wu), (_, yu) = (frame_in(torch.rand(Mu, Nu, generator=g) - 0.25, "u", gpu),
                                 flat_in(torch.rand(Nu, Ku, generator=g) - 0.5, "u", gpu),
                                 frame_in(torch.tanh(torch.randn(Mu, Ku, generator=g)), "u", gpu))
    outs = []
    for fn_in, fn, kw in ((ops.linear_bwd_input, ops.linear_bwd, {}),
                          (ops.linear_bwd_input_dropout, ops.linear_bwd_dropout, rule)):
        _, dxi = frame_out(Mu, Ku, "u", gpu)
        fn_in(zu, wu, yu, ops.ACT_TANH, out=dxi, **kw)
        plan_in = ops.gemm_last_plan()
        dw, db, (_, dx) = torch.empty(Nu, Ku, device=gpu), torch.empty(Nu, device=gpu), frame_out(Mu, Ku, "u", gpu)
        fn(zu, yu, wu, dw, db, dx, yprev=yu, act_prev=ops.ACT_TANH, **kw)
        outs.append((dxi.clone(), dw, db, dx.clone(), plan_in, ops.gemm_last_plan()))
    kinds = [getattr(e, "kernel", "reduce") for e in outs[0][5]]
    assert _one(outs[0][4]).kernel == "staged" and kinds == ["staged", "reduce", "reduce", "staged"], outs[0][4:]
    assert outs[0][4:] == outs[1][4:] and all(torch.equal(_bits(a), _bits(b_)) for a, b_ in zip(outs[0][:4], outs[1][:4]))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[0][3])), "fused and separate input gradients differ"
    assert torch.equal(ops.dropout_apply(dz, 0.0, 1, 2), dz)
    assert torch.equal(ops.dropout_act_bwd(dz, y0, ops.ACT_TANH, 0.0, 1, 2), ops.act_bwd(dz, y0, ops.ACT_TANH))


# ------------------------------------------------------------------------------------------- the flat step
DIMS, M_FLAT = (13, 32, 32, 7), 301


def _flat_inputs():
    g = torch.Generator().manual_seed(41)
    x = (torch.rand(M_FLAT, DIMS[0], generator=g) < 0.25).float() * (1.0 - torch.rand(M_FLAT, DIMS[0], generator=g))
    target = torch.randn(M_FLAT, DIMS[-1], generator=g)
    valid = (torch.rand(M_FLAT, generator=g) > 0.2).to(torch.uint8)
    return x, target, valid


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("drops", [(0.2, 0.5, 0.0), (0.2, 0.2, 0.2)])
def test_flat_step_against_the_restatement(gpu, drops, sparse):
    x, target, valid = _flat_inputs()
    n_valid = float(valid.sum())
    model = FlatFFModel(DIMS, device=gpu, seed=3, dropouts=drops, sparse_input=sparse, sparse_wgrad=False)
    plain = FlatFFModel(DIMS, device=gpu, seed=3, sparse_input=sparse, sparse_wgrad=False)
    layers = [(w.cpu().numpy(), b.cpu().numpy()) for w, b in model.layers()]
    acts = ("tanh", "tanh", None)
    masks = [keep_mask(M_FLAT, N, p, SEED, i) if p > 0 else None for i, (N, p) in enumerate(zip(DIMS[1:], drops))]
    outs, _ = chain_forward(x.numpy(), layers, acts, masks, drops)
    loss_ref, g_ref = masked_mse(outs[-1], target.numpy(), valid.numpy(), n_valid)
    _, grads_ref = chain_backward(x.numpy(), layers, acts, masks, drops, g_ref)

    xd, td, vd = x.to(gpu), target.to(gpu), valid.to(gpu)
    loss = model.loss_and_backward(xd, td, vd, n_valid, seed=SEED)
    check("y", loss.cpu().reshape(1), torch.tensor([loss_ref]))
    first = model.grads.clone()
    for i, (dw, db) in enumerate(grads_ref):
        check("dx", model.weight(i, model.grads).cpu(), torch.from_numpy(dw))
        check("dx", model.bias(i, model.grads).cpu(), torch.from_numpy(db))
    # the training forward's outputs are the dropped ones
    hs = model.forward(xd, sparse=sparse, training=True, seed=SEED)
    for h, ref, mk in zip(hs, outs, masks):
        check("y", h.cpu(), torch.from_numpy(ref))
        if mk is not None:
            assert bool((h.cpu()[~torch.from_numpy(mk)] == 0).all())
    # one seed, one step; another seed, another step
    loss2 = model.loss_and_backward(xd, td, vd, n_valid, seed=SEED)
    assert torch.equal(loss, loss2) and torch.equal(first, model.grads)
    loss3 = model.loss_and_backward(xd, td, vd, n_valid, seed=SEED + 1)
    assert not torch.equal(loss, loss3) and not torch.equal(first, model.grads)
    # without a seed the step draws one from the package's stream: repeatable after reseeding it
    from idiaptts_amd.nn.functional import default_dropout_stream
    default_dropout_stream().reseed(77)
    la = model.loss_and_backward(xd, td, vd, n_valid)
    lb = model.loss_and_backward(xd, td, vd, n_valid)
    default_dropout_stream().reseed(77)
    assert torch.equal(la, model.loss_and_backward(xd, td, vd, n_valid)) and not torch.equal(la, lb)
    # validation and inference: the model without dropout, bit for bit
    for a, b in zip(model.forward(xd, sparse=sparse), plain.forward(xd, sparse=sparse)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        model.forward(xd, training=True)


# ----------------------------------------------------------------------------------------- the module path
def _rnn_dyn(model_type, in_dim, dropout, gpu):
    from idiaptts_amd.src.neural_networks.pytorch.models import rnn_dyn
    hp = types.SimpleNamespace(model_type=model_type, batch_first=False, dropout=dropout)
    return rnn_dyn.convert_legacy_to_config((in_dim,), hp).create_model().to(gpu)


def _linears(model):
    return [m for grp in model.layer_groups for m in grp.module if type(m).__name__ == "LinearAct"]


def _graph_nodes(t):
    seen, todo = [], [t.grad_fn]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.append(n)
        todo += [f for f, _ in n.next_functions]
    return [type(n).__name__ for n in seen]


def test_module_path_against_the_restatement(gpu):
    from idiaptts_amd.nn.functional import DropoutStream, default_dropout_stream
    torch.manual_seed(8)
    T, B, F, p = 23, 3, 13, 0.3
    model = _rnn_dyn("RNNDYN-2_TANH_32-1_FC_7", F, p, gpu).train()
    clean = _rnn_dyn("RNNDYN-2_TANH_32-1_FC_7", F, 0.0, gpu)
    for a, b in zip(_linears(clean), _linears(model)):
        a.load_state_dict(b.state_dict())
    lens = torch.tensor([23, 17, 9])
    x = torch.randn(T, B, F, device=gpu, requires_grad=True)
    dy = torch.randn(T, B, 7, device=gpu)
    default_dropout_stream().reseed(4321)
    y, _ = model(x, seq_lengths_input=lens, max_length_inputs=T)
    y.backward(dy)
    second = DropoutStream()
    second.reseed(4321)
    seeds = [second.next(), second.next()]                  # one per group and forward
    M = T * B
    layers = [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in _linears(model)]
    masks = [keep_mask(M, 32, p, seeds[0], 0), keep_mask(M, 32, p, seeds[0], 1), keep_mask(M, 7, p, seeds[1], 2)]
    acts, ps = ("tanh", "tanh", None), (p, p, p)
    x64 = x.detach().cpu().numpy().reshape(M, F)
    outs, _ = chain_forward(x64, layers, acts, masks, ps)
    dx_ref, grads_ref = chain_backward(x64, layers, acts, masks, ps, dy.cpu().numpy().reshape(M, 7))
    check("y", y.detach().cpu().reshape(M, 7), torch.from_numpy(outs[-1]))
    assert bool((y.detach().cpu().reshape(M, 7)[~torch.from_numpy(masks[2])] == 0).all())
    check("dx", x.grad.cpu().reshape(M, F), torch.from_numpy(dx_ref))
    for m, (dw, db) in zip(_linears(model), grads_ref):
        check("dx", m.weight.grad.cpu(), torch.from_numpy(dw))
        check("dx", m.bias.grad.cpu(), torch.from_numpy(db))
    # the group is one autograd node
    h, _ = model.layer_groups[0](x.detach().requires_grad_(), seq_lengths_input=lens, max_length_inputs=T)
    names = _graph_nodes(h)
    assert [n for n in names if n.endswith("FunctionBackward")] == ["LinearChainFunctionBackward"], names
    assert not [n for n in names if "Dropout" in n or "Mul" in n or "Addmm" in n], names
    # eval(): the model without dropout, bit for bit
    model.eval()
    clean.eval()
    with torch.no_grad():
        ye, _ = model(x, seq_lengths_input=lens, max_length_inputs=T)
        yc, _ = clean(x, seq_lengths_input=lens, max_length_inputs=T)
    assert torch.equal(ye, yc)


def test_layer_norm_group_uses_the_elementwise_kernel(gpu):
    from idiaptts_amd.nn.functional import DropoutStream, default_dropout_stream
    from idiaptts_amd.src.neural_networks.pytorch.models.rnn_dyn import Config, FFWrapper
    torch.manual_seed(9)
    T, B, F, p = 11, 3, 19, 0.3
    lc = Config.LayerConfig("LayerNorm", num_layers=1, nonlin="tanh", dropout=p, normalized_shape=F)
    group = FFWrapper(F, lc, batch_first=False).to(gpu)
    x = torch.randn(T, B, F, device=gpu)
    dy = torch.randn(T, B, F, device=gpu)
    group.eval()
    x0 = x.clone().requires_grad_()
    y0, _ = group(x0)
    group.train()
    default_dropout_stream().reseed(99)
    x1 = x.clone().requires_grad_()
    y1, _ = group(x1)
    second = DropoutStream()
    second.reseed(99)
    m = _mask(T * B, F, p, second.next(), 0, 0, gpu).view(T, B, F)
    scale = float(scale_f32(p))
    assert torch.equal(_bits(y1.detach()), _bits(torch.where(m, y0.detach() * scale, torch.zeros((), device=gpu))))
    assert "DropoutFunctionBackward" in _graph_nodes(y1)
    y1.backward(dy)
    y0.backward(torch.where(m, dy * scale, torch.zeros((), device=gpu)))
    assert torch.equal(x1.grad, x0.grad)
    for prm in group.parameters():
        assert prm.grad is not None


# --------------------------------------------------------------------------------------------- the trainer
def test_trainer_keeps_a_dropout_model_on_the_flat_step(gpu, golden_dir, tmp_path):
    from fixture_dirs import materialise
    from idiaptts_amd.src.model_trainers.AcousticModelTrainer import AcousticModelTrainer
    root = str(tmp_path)
    ids, wdir, qdir, _ = materialise(golden_dir, root)

    def run(name):
        hp = AcousticModelTrainer.create_hparams()
        hp.num_questions, hp.voice, hp.out_dir = 409, "full", os.path.join(root, name)
        hp.frame_size_ms, hp.num_coded_sps, hp.seed, hp.epochs = 5, 20, 1234, 3
        hp.use_gpu, hp.dataset_num_workers_gpu = True, 0
        hp.model_type, hp.dropout = "RNNDYN-1_RELU_32-1_FC_67", 0.2
        hp.batch_size_train, hp.batch_size_val = 2, 50
        hp.optimiser_args["lr"] = 0.001
        hp.model_name, hp.epochs_per_checkpoint = "test_model", 2
        hp.world_dir, hp.use_best_as_final_model, hp.resident_dataset = wdir, False, True
        trainer = AcousticModelTrainer(**AcousticModelTrainer.legacy_support_init(wdir, qdir, ids, hp.num_questions, hp))
        trainer.init(hp)
        val, train, handler = trainer.train(hp)
        return trainer, hp, handler, val["MSELoss_acoustic_features"], train["MSELoss_acoustic_features"]

    trainer, hp, handler, val, train = run("a")
    assert handler._resident is not None and handler._resident["flat"].dropouts == [0.2, 0.2]
    assert np.isfinite(val).all() and np.isfinite(train).all()
    _, _, handler_b, val_b, train_b = run("b")
    assert handler_b._resident is not None
    assert list(val) == list(val_b) and list(train) == list(train_b)
    # validation ran without dropout: the module path's eval() loss of the same weights
    handler._resident_sync_to_module()
    hp.resident_dataset = False
    handler.set_dataset(hp, trainer.dataset_train, trainer.dataset_val, trainer.batch_collate_fn)
    assert handler._resident is None
    loss = handler.test(hparams=hp, total_epoch=trainer.total_epoch, total_steps=trainer.total_steps,
                        current_epoch=hp.epochs)
    np.testing.assert_allclose(loss["MSELoss_acoustic_features"], val[-1], rtol=2e-5)
