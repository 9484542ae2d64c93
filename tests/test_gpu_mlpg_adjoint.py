"""The MLPG adjoint kernel, MlpgFunction and MLPGLayer on the GPU against the float64 restatement
(tests/mlpg_adjoint_spec.py).  Bounds: float64 gradients the forward's own (rmse 1e-10, largest element 1e-9, times
max(1, max|ref|)); float32 gradients the dense layers' (relative 2-norm 2e-6, per element 2e-5 max(1, max|ref|));
parameter gradients of the chain 1e-5 relative, as tests/test_gpu_lnorm_model.py."""
import numpy as np
import pytest
import torch

import mlpg_adjoint_spec as spec
from idiaptts_amd.src.neural_networks.pytorch.loss.NamedLoss import NamedLoss
from idiaptts_amd.src.neural_networks.pytorch.ModularModelHandlerPyTorch import ModularModelHandlerPyTorch as Handler
from idiaptts_amd.src.neural_networks.pytorch.models import enc_dec_dyn, rnn_dyn

pytestmark = pytest.mark.gpu


def _check(got, ref, f32, what=""):
    (spec.check_f32 if f32 else spec.check_f64)(got, ref, what)


# ---- the kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", spec.VARIANCE_SETS)
@pytest.mark.parametrize("dim", spec.DIMS)
def test_adjoint_shape_sweep(gpu, dim, kind, f32):
    from idiaptts_amd import ops
    offsets, var, gout, ref = spec.sweep_case(dim, kind, f32)
    got = ops.mlpg_adjoint(torch.tensor(gout).to(gpu), torch.tensor(var).to(gpu), dim, offsets)
    assert got.dtype == (torch.float32 if f32 else torch.float64) and got.shape == (offsets[-1], 3 * dim)
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    _check(got, ref, f32, "D %d %s" % (dim, kind))
    for a, b in zip(offsets[:-1], offsets[1:]):          # and utterance by utterance, each at its own scale
        if b > a:
            _check(got[a:b], ref[a:b], f32, "D %d %s T %d" % (dim, kind, b - a))


@pytest.mark.parametrize("gin32,out32", [(False, False), (True, True), (True, False), (False, True)],
                         ids=["f64-f64", "f32-f32", "f32-f64", "f64-f32"])
def test_adjoint_column_placement_and_untouched_memory(gpu, gin32, out32):
    """gcol0, col0 != 0 inside wider tensors of odd pitch, a row range inside a taller one: every element outside the
    written block keeps its bits, and 1e30 in the unread columns of the incoming gradient changes nothing."""
    from idiaptts_amd import ops
    dim, gcol0, col0, top, bottom = 15, 3, 5, 2, 3
    offsets, var, gout, ref = spec.sweep_case(dim, "loguniform", gin32)
    n = offsets[-1]
    gdt, odt = (torch.float32 if gin32 else torch.float64), (torch.float32 if out32 else torch.float64)
    gbuf = torch.full((n, 23), 1e30, dtype=gdt)
    gbuf[:, gcol0:gcol0 + dim] = torch.tensor(gout)
    sentinel = -12345.678
    obuf = torch.full((top + n + bottom, 55), sentinel, dtype=odt, device=gpu)
    out = obuf[top:top + n]
    res = ops.mlpg_adjoint(gbuf.to(gpu), torch.tensor(var).to(gpu), dim, offsets, gcol0=gcol0, out=out, col0=col0)
    assert res is out
    host = obuf.cpu()
    _check(host[top:top + n, col0:col0 + 3 * dim].numpy(), ref, out32, "placed")
    host[top:top + n, col0:col0 + 3 * dim] = sentinel
    assert torch.equal(host, torch.full_like(host, sentinel))
    # a plan, another pitch: the same bits
    plan = ops.MlpgPlan(offsets)
    again = ops.mlpg_adjoint(torch.tensor(gout).to(gpu), torch.tensor(var).to(gpu), dim, offsets, plan=plan,
                             out=torch.empty((n, 3 * dim), dtype=odt, device=gpu))
    assert torch.equal(again.cpu(), obuf[top:top + n, col0:col0 + 3 * dim].cpu())
    plan.close()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_adjoint_utterances_are_isolated_and_edges_carry_1e_minus_11(gpu, f32):
    from idiaptts_amd import ops
    dim = 17
    offsets, var, gout, ref = spec.sweep_case(dim, "typical", f32)
    lengths = np.diff(offsets)
    d_var = torch.tensor(var).to(gpu)
    base = ops.mlpg_adjoint(torch.tensor(gout).to(gpu), d_var, dim, offsets).cpu().numpy()
    for u in (int(np.argmax(lengths == 9)), int(np.argmax(lengths == 64))):
        loud = gout.copy()
        for v in (u - 1, u + 1):                            # both neighbours shout
            loud[offsets[v]:offsets[v + 1]] = 1e6
        got = ops.mlpg_adjoint(torch.tensor(loud).to(gpu), d_var, dim, offsets).cpu().numpy()
        a, b = offsets[u], offsets[u + 1]
        assert np.array_equal(got[a:b], base[a:b])
        _check(got[a:b], ref[a:b], f32, "isolated T %d" % (b - a))
        assert np.abs(got[offsets[u + 1]:offsets[u + 2]]).max() > 1e4
    for a, b in zip(offsets[:-1], offsets[1:]):
        if b > a:
            z = np.abs(base[a:b, :dim].astype(np.float64) * var[:dim]).max()
            assert z > 0
            assert np.abs(base[[a, b - 1], dim:]).max() <= 4.1e-11 * z, (b - a)


def test_adjoint_is_deterministic_and_the_planned_entry_gives_the_same_bits(gpu):
    from idiaptts_amd import ops
    for dim, f32 in ((60, True), (65, False)):
        offsets, var, gout, _ = spec.sweep_case(dim, "loguniform", f32)
        d_g, d_var = torch.tensor(gout).to(gpu), torch.tensor(var).to(gpu)
        first = ops.mlpg_adjoint(d_g, d_var, dim, offsets).cpu()
        assert torch.equal(ops.mlpg_adjoint(d_g, d_var, dim, offsets).cpu(), first)
        plan = ops.MlpgPlan(offsets)
        assert torch.equal(ops.mlpg_adjoint(d_g, d_var, dim, None, plan=plan).cpu(), first)
        assert torch.equal(ops.mlpg_adjoint(d_g, d_var, dim, None, plan=plan).cpu(), first)
        plan.close()


def test_adjoint_wrapper_refuses_wrong_shapes(gpu):
    from idiaptts_amd import ops
    var = torch.ones(6, dtype=torch.float64, device=gpu)
    g = torch.zeros(5, 2, dtype=torch.float64, device=gpu)
    with pytest.raises(ValueError, match="number of rows"):
        ops.mlpg_adjoint(g, var, 2, [0, 4])
    with pytest.raises(ValueError, match="columns"):
        ops.mlpg_adjoint(g, var, 2, [0, 5], gcol0=1)
    with pytest.raises(ValueError, match="out must hold"):
        ops.mlpg_adjoint(g, var, 2, [0, 5], out=torch.zeros(5, 5, dtype=torch.float64, device=gpu))
    with pytest.raises(ValueError, match="3 \\* dim"):
        ops.mlpg_adjoint(g, var[:5], 2, [0, 5])
    empty = ops.mlpg_adjoint(g[:0], var, 2, [0, 0])
    assert empty.shape == (0, 6)


# ---- MlpgFunction --------------------------------------------------------------------------------------------------
FN_STREAMS = [(1, 4), (13, 1), (17, 2)]          # (col0, dim); columns 0 and 16 belong to no stream
FN_WIDTH = 23
FN_LENGTHS = (5, 300, 1, 64, 0, 2, 193)


def _fn_case(f32):
    rng = np.random.RandomState(21)
    offsets = spec.offsets_of(FN_LENGTHS)
    rows = rng.standard_normal((offsets[-1], FN_WIDTH))
    weights = rng.standard_normal((offsets[-1], sum(d for _, d in FN_STREAMS)))
    if f32:
        rows, weights = rows.astype(np.float32), weights.astype(np.float32)
    streams = [(c0, d, spec.variances("loguniform" if d == 4 else "typical", d)) for c0, d in FN_STREAMS]
    return offsets, rows, weights, streams


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_mlpg_function_forward_and_gradient(gpu, f32):
    from idiaptts_amd.misc.mlpg import MLPG
    from idiaptts_amd.nn.functional import MlpgFunction
    offsets, rows, weights, streams = _fn_case(f32)
    d_rows = torch.tensor(rows).to(gpu).requires_grad_(True)
    d_streams = [(c0, d, torch.tensor(v).to(gpu)) for c0, d, v in streams]
    out = MlpgFunction.apply(d_rows, d_streams, offsets, None)
    assert out.dtype == d_rows.dtype and out.shape == weights.shape
    # the forward is ops.mlpg_generation unchanged: what MLPG().generation_streams returns for the same rows
    mats = [rows[a:b] for a, b in zip(offsets[:-1], offsets[1:])]
    trajs = MLPG().generation_streams(mats, [(c0, np.diag(v), d) for c0, d, v in streams])
    same = np.concatenate([np.concatenate(t, axis=0) for t in trajs], axis=1)
    if f32:
        assert np.array_equal(out.detach().cpu().numpy(), same.astype(np.float32))
    else:
        assert np.array_equal(out.detach().cpu().numpy(), same)
    ref_out = np.concatenate([spec.per_utterance(spec.trajectory, rows[:, c0:c0 + 3 * d].astype(np.float64), v, d, offsets)
                              for c0, d, v in streams], axis=1)
    _check(out.detach().cpu().numpy(), ref_out, f32, "forward")
    (out * torch.tensor(weights).to(gpu)).sum().backward()
    grad = d_rows.grad.cpu().numpy()
    ref = np.zeros((offsets[-1], FN_WIDTH))
    o0 = 0
    for c0, d, v in streams:
        ref[:, c0:c0 + 3 * d] = spec.per_utterance(spec.adjoint, weights[:, o0:o0 + d].astype(np.float64), v, d, offsets)
        o0 += d
    _check(grad, ref, f32, "gradient")
    assert not grad[:, 0].any() and not grad[:, 16].any()          # columns of no stream: exactly zero
    # a pitched view of wider rows is read in place and gives the same bits
    wide = torch.zeros((offsets[-1], FN_WIDTH + 6), dtype=d_rows.dtype, device=gpu)
    wide[:, :FN_WIDTH] = d_rows.detach()
    assert torch.equal(MlpgFunction.apply(wide[:, :FN_WIDTH], d_streams, offsets, None), out.detach())


def test_mlpg_function_refusals(gpu):
    from idiaptts_amd.nn.functional import MlpgFunction
    offsets, rows, weights, streams = _fn_case(False)
    d_rows = torch.tensor(rows).to(gpu).requires_grad_(True)
    d_streams = [(c0, d, torch.tensor(v).to(gpu)) for c0, d, v in streams]
    learnt = [(c0, d, v.clone().requires_grad_(True)) for c0, d, v in d_streams]
    with pytest.raises(ValueError, match="variances"):
        MlpgFunction.apply(d_rows, learnt, offsets, None)
    out = MlpgFunction.apply(d_rows, d_streams, offsets, None)
    weights = torch.ones_like(out).requires_grad_(True)          # (a gradient that itself asks for a gradient)
    (grad,) = torch.autograd.grad((out * weights).sum(), d_rows, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):
        grad.sum().backward()


def test_inference_runs_the_forward_only(gpu, monkeypatch):
    from idiaptts_amd import ops
    from idiaptts_amd.nn import MLPGLayer
    calls = {"adjoint": 0, "generation": 0}
    real_adjoint, real_generation = ops.mlpg_adjoint, ops.mlpg_generation

    def adjoint(*args, **kwargs):
        calls["adjoint"] += 1
        return real_adjoint(*args, **kwargs)

    def generation(*args, **kwargs):
        calls["generation"] += 1
        return real_generation(*args, **kwargs)

    monkeypatch.setattr(ops, "mlpg_adjoint", adjoint)
    monkeypatch.setattr(ops, "mlpg_generation", generation)
    layer = _layer(True, True).to(gpu)
    x = torch.randn(3, 13, C, device=gpu)
    for context in (torch.no_grad, torch.inference_mode):
        with context():
            out, _ = layer(x, seq_lengths_input=torch.tensor(LENS), max_length_inputs=13)
        assert not out.requires_grad
    assert calls == {"adjoint": 0, "generation": 6}
    out, _ = layer(x.requires_grad_(True), seq_lengths_input=torch.tensor(LENS), max_length_inputs=13)
    out.sum().backward()
    assert calls == {"adjoint": 3, "generation": 9}


# ---- MLPGLayer -----------------------------------------------------------------------------------------------------
STREAMS = [(0, 4), (12, 1), (16, 2)]          # C = 3 * 4 + 3 * 1 + 1 + 3 * 2, V/UV at column 15
VUV, C, WIDTH_OUT = 15, 22, 8
LENS = (13, 7, 10)


def _layer(batch_first, normalised, select_only=False):
    from idiaptts_amd.nn import MLPGLayer
    rng = np.random.RandomState(3)
    mean, std_dev = (rng.standard_normal(C), rng.uniform(0.5, 2.0, C)) if normalised else (None, None)
    streams = [(c0, d, spec.variances("loguniform" if d == 2 else "typical", d)) for c0, d in STREAMS]
    return MLPGLayer(streams, passthrough=[VUV], mean=mean, std_dev=std_dev, batch_first=batch_first,
                     select_only=select_only)


def _dense_close(got, ref, what):
    """the dense layers' bounds (tests/lnorm_cases.py)"""
    spec.check_f32(got.detach().double().cpu().numpy(), ref.detach().double().cpu().numpy(), what)


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "f64"])
@pytest.mark.parametrize("batch_first", [True, False], ids=["BTC", "TBC"])
def test_layer_against_its_cpu_path(gpu, batch_first, f32):
    B, T = len(LENS), max(LENS) + 1
    g = torch.Generator().manual_seed(8)
    dtype = torch.float32 if f32 else torch.float64
    x = torch.randn((B, T, C) if batch_first else (T, B, C), generator=g, dtype=dtype)
    w = torch.randn(x.shape[:2] + (WIDTH_OUT,), generator=g, dtype=dtype)
    lens = torch.tensor(LENS)
    cpu_layer = _layer(batch_first, True)
    x_ref = x.detach().clone().double().requires_grad_(True)
    ref, _ = cpu_layer(x_ref, seq_lengths_input=lens, max_length_inputs=T)
    (ref * w.double()).sum().backward()
    layer = _layer(batch_first, True).to(gpu)
    assert layer.variances_0.is_cuda and layer.mean.is_cuda and layer.variances_0.dtype == torch.float64
    x_gpu = x.to(gpu).requires_grad_(True)
    out, kwargs = layer(x_gpu, seq_lengths_input=lens, max_length_inputs=T)
    assert out.dtype == dtype and out.shape == ref.shape and kwargs["seq_lengths_input"] is lens
    (out * w.to(gpu)).sum().backward()
    _dense_close(out, ref, "layer output")
    _dense_close(x_gpu.grad, x_ref.grad, "layer input gradient")
    for u, n in enumerate(LENS):
        pad_out = out[u, n:] if batch_first else out[n:, u]
        pad_grad = x_gpu.grad[u, n:] if batch_first else x_gpu.grad[n:, u]
        assert not pad_out.any() and not pad_grad.any()
    # the same batch again takes the kept layout and plan: the same bits
    again, _ = layer(x_gpu.detach(), seq_lengths_input=lens, max_length_inputs=T)
    assert torch.equal(again, out.detach())


def test_layer_as_the_last_module_of_a_trajectory_training_chain(gpu):
    """questions -> Linear(9 -> C) -> pred_acoustic_features -> MLPGLayer -> pred_trajectory; acoustic_features ->
    MLPGLayer(select_only) -> acoustic_static; masked MSE between the two.  Loss and every parameter gradient against
    the same chain on the CPU in float64."""
    W, M = enc_dec_dyn.Config.WrapperConfig, enc_dec_dyn.Config.ModuleConfig
    full, select = _layer(True, True), _layer(True, True, select_only=True)

    def layer_config(layer, select_only):
        from idiaptts_amd.nn import MLPGLayer
        streams = [(c0, d, getattr(layer, "variances_%d" % i).numpy()) for i, (c0, d) in enumerate(STREAMS)]
        return MLPGLayer.Config(streams, passthrough=[VUV], mean=layer.mean.numpy(), std_dev=layer.std_dev.numpy(),
                                select_only=select_only)

    config = enc_dec_dyn.Config(modules=[
        M(name="acoustic", input_names=["questions"], process_group=0, output_names=["pred_acoustic_features"],
          config=rnn_dyn.Config(in_dim=9, batch_first=True,
                                layer_configs=[rnn_dyn.Config.LayerConfig("Linear", out_dim=C)])),
        W(layer_config(full, False), ["pred_acoustic_features"], name="trajectory", output_names=["pred_trajectory"],
          process_group=1),
        W(layer_config(select, True), ["acoustic_features"], name="static", output_names=["acoustic_static"],
          process_group=1)])
    torch.manual_seed(4)
    model = config.create_model().to(gpu)
    params = dict(model.named_parameters())
    assert len(params) == 2 and all(k.startswith("acoustic.") for k in params)
    loss_fn = NamedLoss(NamedLoss.Config("MSELoss_trajectory", "MSELoss", seq_mask="acoustic_features_mask",
                                         input_names=["acoustic_static", "pred_trajectory"], batch_first=True))
    B, T = len(LENS), max(LENS)
    lens = torch.tensor(LENS)
    g = torch.Generator().manual_seed(9)
    questions, target = torch.randn(B, T, 9, generator=g), torch.randn(B, T, C, generator=g)
    mask = Handler.sequence_mask(lens, T, batch_first=True)
    questions, target = questions * mask, target * mask
    data = {"questions": questions.to(gpu), "acoustic_features": target.to(gpu), "acoustic_features_mask": mask.to(gpu)}
    lengths = {k: lens for k in data}
    max_lengths = {k: T for k in data}
    model.init_hidden(B)
    model(data, lengths, max_lengths)
    assert data["pred_trajectory"].shape == data["acoustic_static"].shape == (B, T, WIDTH_OUT)
    loss = loss_fn(data, lengths, 0)["MSELoss_trajectory"]
    loss.backward()
    # the same chain on the CPU in float64
    weight, bias = [p.detach().double().cpu().requires_grad_(True)
                    for p in sorted(params.values(), key=lambda p: -p.dim())]
    pred = questions.double() @ weight.t() + bias
    traj, _ = full(pred, seq_lengths_input=lens, max_length_inputs=T)
    static, _ = select(target.double(), seq_lengths_input=lens, max_length_inputs=T)
    ref_loss = (((traj - static) ** 2) * mask.double()).sum() / (float(lens.sum()) * WIDTH_OUT)
    ref_loss.backward()
    _dense_close(data["pred_trajectory"], traj, "pred_trajectory")
    assert torch.equal(data["acoustic_static"].cpu(), static.float())
    loss, ref_loss = float(loss.detach()), float(ref_loss.detach())
    print("loss", loss, ref_loss)
    assert abs(loss - ref_loss) <= 2e-6 * abs(ref_loss)
    for key, prm in params.items():
        ref = (weight if prm.dim() == 2 else bias).grad.numpy()
        err = np.linalg.norm(prm.grad.double().cpu().numpy() - ref) / np.linalg.norm(ref)
        print(key, "relative gradient error", err)
        assert err < 1e-5, (key, err)
