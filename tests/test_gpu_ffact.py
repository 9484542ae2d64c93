"""Linear layers with the activations beyond Tanh / ReLU (Sigmoid, LogSigmoid, Softplus, Softsign, LeakyReLU, ELU,
CELU, SELU, Hardtanh, ReLU6, Hardsigmoid) on the GPU: the fused GEMM epilogues and act_bwd through ops against torch
in float64, torch's values at the branch points, the fused backward against the separate calls bit for bit, RNNDyn
against the reference's own CPU runs (tests/golden/ffact_fixture.npz, written by tests/golden/make_golden_ffact.py),
the valid-rows path against the padded one, the flat feed-forward step, and AcousticModelTrainer on the module path
and with hparams.resident_dataset."""
import os

import numpy as np
import pytest
import torch

from ffact_cases import CASES, case_config, case_inputs, masked_mse, trainer_model_config
from fixture_dirs import materialise
from idiaptts_amd import ops
from idiaptts_amd.native_ff import FlatFFModel
from idiaptts_amd.nn.functional import padding_rows_identical
from idiaptts_amd.src.neural_networks.pytorch.models import rnn_dyn
from idiaptts_amd.src.neural_networks.pytorch.models.rnn_dyn import Config, RNNDyn

pytestmark = pytest.mark.gpu

NEW_ACTS = sorted(c for c in ops.ACT_TORCH_NAME if c >= ops.ACT_SIGMOID)
IDS = [ops.ACT_TORCH_NAME[c] for c in NEW_ACTS]


def _rel(a, b):
    return (a - b).norm().item() / (b.norm().item() + 1e-30)


def _act64(code, z):
    """torch's activation (default arguments) on a float64 tensor"""
    return getattr(torch.nn, ops.ACT_TORCH_NAME[code])()(z)


def _dact64(code, z):
    """torch's derivative of the activation at z (float64 autograd, so torch's rule at every branch point)"""
    z = z.detach().double().requires_grad_(True)
    y = _act64(code, z)
    (g,) = torch.autograd.grad(y.sum(), z)
    return g


def _rows(M, N, device, fill=None):
    """[M, N] view of a zeroed [M, N rounded up to 4] buffer (16-byte rows)"""
    full = torch.zeros(M, (N + 3) // 4 * 4, device=device)
    v = full[:, :N]
    if fill is not None:
        v.copy_(fill)
    return v


FWD_SHAPES = [   # M, N, K, output rows padded to 16 bytes
    (5, 7, 3, False), (257, 512, 425, False), (1000, 512, 512, False), (333, 67, 412, True), (130, 187, 64, True),
    (64, 32, 36, False)]


@pytest.mark.parametrize("M,N,K,padded", FWD_SHAPES)
@pytest.mark.parametrize("act", NEW_ACTS, ids=IDS)
def test_linear_fwd(gpu, act, M, N, K, padded):
    g = torch.Generator().manual_seed(M * 31 + N + act)
    x = torch.randn(M, K, generator=g) * 4
    w = (torch.rand(N, K, generator=g) - 0.5) * (2.0 / K ** 0.5)
    b = torch.rand(N, generator=g) - 0.5
    ref = _act64(act, torch.nn.functional.linear(x.double(), w.double(), b.double()))
    out = _rows(M, N, gpu) if padded else None
    y = ops.linear_fwd(x.to(gpu), w.to(gpu), b.to(gpu), act, out=out).cpu().double()
    assert _rel(y, ref) < 2e-6
    assert (y - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    if padded:
        assert torch.equal(out.as_strided((M, out.stride(0)), (out.stride(0), 1))[:, N:].cpu(),
                           torch.zeros(M, out.stride(0) - N))


@pytest.mark.parametrize("act", NEW_ACTS, ids=IDS)
def test_act_bwd(gpu, act):
    g = torch.Generator().manual_seed(act)
    M, N = 300, 187
    z = torch.randn(M, N, generator=g) * 5
    y = _act64(act, z.double()).float()
    dy = torch.randn(M, N, generator=g)
    ref = dy.double() * _dact64(act, z)
    for padded in (False, True):
        dyg = _rows(M, N, gpu, dy) if padded else dy.to(gpu)
        yg = _rows(M, N, gpu, y) if padded else y.to(gpu)
        dz = ops.act_bwd(dyg, yg, act).cpu().double()
        assert _rel(dz, ref) < 2e-6
        assert (dz - ref).abs().max().item() < 2e-6 * max(1.0, ref.abs().max().item())


BWD_SHAPES = [(5, 7, 3), (300, 187, 512), (257, 512, 425), (129, 64, 68), (1000, 512, 512)]


@pytest.mark.parametrize("M,N,K", BWD_SHAPES)
@pytest.mark.parametrize("act", NEW_ACTS, ids=IDS)
def test_linear_bwd_input(gpu, act, M, N, K):
    g = torch.Generator().manual_seed(M + N + act)
    dz = torch.randn(M, N, generator=g)
    w = torch.randn(N, K, generator=g) / N ** 0.5
    zprev = torch.randn(M, K, generator=g) * 4
    yprev = _act64(act, zprev.double()).float()
    ref = (dz.double() @ w.double()) * _dact64(act, zprev)
    dx = ops.linear_bwd_input(dz.to(gpu), w.to(gpu), yprev.to(gpu), act).cpu().double()
    assert _rel(dx, ref) < 1e-5
    assert (dx - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("M,N,K", [(3001, 187, 512), (2500, 512, 512), (777, 64, 96), (65, 7, 3)])
@pytest.mark.parametrize("act", NEW_ACTS, ids=IDS)
def test_fused_backward_equals_the_separate_calls_bit_for_bit(gpu, act, M, N, K):
    """itts_linear_bwd (weight + bias + input gradient in one launch, the previous layer's activation derivative in
    its epilogue) against itts_linear_bwd_weight + itts_linear_bwd_input, and against torch in float64"""
    g = torch.Generator().manual_seed(M + N + act)
    Kp = (K + 3) // 4 * 4
    zprev = torch.randn(M, K, generator=g) * 4
    x = torch.zeros(M, Kp)
    x[:, :K] = _act64(act, zprev.double()).float()
    dz = torch.randn(M, N, generator=g)
    w = torch.zeros(N, Kp)
    w[:, :K] = torch.randn(N, K, generator=g) * 0.1
    xg, wg = x.to(gpu), w.to(gpu)
    Np = (N + 3) // 4 * 4
    dzg = _rows(M, N, gpu, dz)
    flat = torch.zeros(N * Kp + Np, device=gpu)
    dw, db = flat[:N * Kp].view(N, Kp), flat[N * Kp:N * Kp + N]
    dx = torch.zeros(M, Kp, device=gpu)
    ops.linear_bwd(dzg, xg, wg, dw, db, dx, yprev=xg, act_prev=act)
    flat2 = torch.zeros_like(flat)
    dw2, db2 = flat2[:N * Kp].view(N, Kp), flat2[N * Kp:N * Kp + N]
    ops.linear_bwd_weight(dzg, xg, dw=dw2, db=db2)
    dx2 = ops.linear_bwd_input(dzg, wg, yprev=xg, act_prev=act, out=torch.zeros(M, Kp, device=gpu))
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(dx, dx2)
    dw_ref = dz.double().t() @ x.double()
    dx_ref = (dz.double() @ w.double())[:, :K] * _dact64(act, zprev)
    assert (dw.cpu().double() - dw_ref).abs().max() < 2e-4 * max(1.0, dw_ref.abs().max().item())
    assert (db.cpu().double() - dz.double().sum(0)).abs().max() < 2e-4 * max(1.0, dz.double().sum(0).abs().max().item())
    assert (dx.cpu().double()[:, :K] - dx_ref).abs().max() < 1e-5 * max(1.0, dx_ref.abs().max().item())
    assert not dx.cpu()[:, K:].any()


# pre-activations at and around every branch point, and deep in saturation
BRANCH_Z = [0.0, -0.0, 1.0, -1.0, 6.0, -6.0, 3.0, -3.0, 20.0, -20.0, 20.5, 19.5, 0.5, -0.5, 1e-3, -1e-3, 2.0, -2.0,
            50.0, -50.0, 100.0, -100.0, 1e3, -1e3, 1e30, -1e30, 5.999, 6.001, 2.999, -2.999, 0.999, -0.999]


@pytest.mark.parametrize("act", NEW_ACTS, ids=IDS)
def test_branch_points_take_torch_values(gpu, act):
    """z placed exactly (x @ I, no bias): the forward equals torch in float64, and the derivative through the
    output (itts_linear_bwd_input with an identity weight and dz = 1, and itts_act_bwd) takes torch's value at the
    branch points -- LeakyReLU 0.01 and ELU / CELU 1 at z = 0, 0 at the clamps of Hardtanh / ReLU6 / Hardsigmoid"""
    n = len(BRANCH_Z)
    z = torch.tensor(BRANCH_Z, dtype=torch.float32).reshape(n // 8, 8)
    eye = torch.eye(8)
    y = ops.linear_fwd(z.to(gpu), eye.to(gpu), None, act)
    ref = _act64(act, z.double())
    np.testing.assert_allclose(y.cpu().double().numpy(), ref.numpy(), rtol=1e-6, atol=1e-7)
    dref = _dact64(act, z).numpy()
    d = ops.linear_bwd_input(torch.ones(n // 8, 8, device=gpu), eye.to(gpu), y, act)
    np.testing.assert_allclose(d.cpu().double().numpy(), dref, rtol=1e-6, atol=1e-7)
    d = ops.act_bwd(torch.ones(n // 8, 8, device=gpu), y, act)
    np.testing.assert_allclose(d.cpu().double().numpy(), dref, rtol=1e-6, atol=1e-7)


def test_unknown_codes_are_refused(gpu):
    from idiaptts_amd.lib import IttsError
    x = torch.zeros(4, 4, device=gpu)
    w = torch.zeros(4, 4, device=gpu)
    with pytest.raises(IttsError, match="unknown activation"):
        ops.linear_fwd(x, w, None, ops.ACT_HARDSIGMOID + 1)
    with pytest.raises(IttsError, match="unknown activation"):
        ops.act_bwd(x, x, ops.ACT_HARDSIGMOID + 1)
    with pytest.raises(IttsError, match="unknown activation"):     # the Conv1d kernels fuse Tanh / ReLU only
        ops.conv1d_fwd(torch.zeros(1, 4, 4, device=gpu), torch.zeros(4, 4, 3, device=gpu), None, 1, 1, True,
                       ops.ACT_SIGMOID)


@pytest.fixture(scope="module")
def ffact_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ffact_fixture.npz"))


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c[0] for c in CASES])
def test_reference_module_case(gpu, ffact_golden, index):
    """the reference's RNNDyn (same seed) on a zero-padded batch: output, masked MSE, every parameter gradient and
    the input gradient, at the Conv1d model tests' tolerances -- on the padded tensor and on the valid rows"""
    g = ffact_golden
    case = CASES[index]
    name, in_dim, bf, lens, scale = case[0], case[2], case[3], case[5], case[6]
    p = name + "/"
    sd = {k[len(p + "sd/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(p + "sd/")}
    for identical in (False, True):
        model = RNNDyn(case_config(Config, case)).to(gpu)
        assert list(model.state_dict().keys()) == list(sd.keys())
        model.load_state_dict(sd)
        x, tgt = case_inputs(torch, index, in_dim, bf, lens, g[p + "y"].shape, scale)
        x = x.to(gpu).requires_grad_(True)
        lens_t = torch.tensor(lens, device=gpu)
        with padding_rows_identical(identical):
            y, _ = model(x, seq_lengths_input=lens_t, max_length_inputs=torch.tensor(max(lens)))
        loss = masked_mse(torch, y, tgt.to(gpu), lens_t, bf)
        loss.backward()
        ref_y = g[p + "y"]
        np.testing.assert_allclose(y.detach().cpu().numpy(), ref_y, rtol=0, atol=2e-5 * max(1, np.abs(ref_y).max()))
        np.testing.assert_allclose(float(loss), float(g[p + "loss"]), rtol=2e-6)
        for k, prm in model.named_parameters():
            ref = g[p + "grad/" + k]
            err = np.linalg.norm(prm.grad.cpu().numpy() - ref) / (np.linalg.norm(ref) + 1e-30)
            assert err < 1e-5, (k, identical, err)
        ref = g[p + "grad_x"]
        mask = (torch.arange(max(lens))[None, :] < torch.tensor(lens)[:, None])
        mask = (mask if bf else mask.t()).numpy()
        got = x.grad.cpu().numpy()
        err = np.linalg.norm(got[mask] - ref[mask]) / np.linalg.norm(ref[mask])
        assert err < 1e-5, (identical, err)


@pytest.mark.parametrize("batch_first", [True, False])
def test_valid_rows_path_equals_the_padded_path(gpu, batch_first):
    """Linear groups of mixed activations, one of them ending in Sigmoid: inside padding_rows_identical() the groups
    run on the valid rows as one LinearChainFunction node (the fused backward with every activation's derivative in
    its epilogue); the output at every position, every parameter gradient and the input gradient of the valid frames
    equal the padded run"""
    L = Config.LayerConfig
    layers = [L("Linear", out_dim=36, nonlin="SELU"), L("Linear", out_dim=20, num_layers=2, nonlin="Softplus"),
              L("Linear", out_dim=24, nonlin="Hardtanh"), L("Linear", out_dim=16, nonlin="LogSigmoid"),
              L("Linear", out_dim=7, nonlin="Sigmoid")]
    cfg = Config(in_dim=13, batch_first=batch_first, layer_configs=layers)
    torch.manual_seed(5)
    model = RNNDyn(cfg).to(gpu)
    lens = torch.tensor([40, 17, 33, 9], device=gpu)
    B, T = len(lens), 40
    x = torch.randn((B, T, 13) if batch_first else (T, B, 13), device=gpu) * 3
    pos = torch.arange(T, device=gpu)
    pad = (pos[None, :] >= lens[:, None])
    pad = pad if batch_first else pad.t()
    x[pad] = 0
    results = []
    for identical in (False, True):
        model.zero_grad()
        xi = x.clone().requires_grad_(True)
        with padding_rows_identical(identical):
            y, _ = model(xi, seq_lengths_input=lens, max_length_inputs=T)
        y.backward(torch.ones_like(y))
        results.append([y.detach(), xi.grad[~pad]] + [p.grad.clone() for p in model.parameters()])
    # (the two paths run the GEMMs on different row counts, hence other split-K chunks of the weight gradients)
    for a, b in zip(*results):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)


def _ref_stack(layers, acts):
    mods = []
    for (w, b), a in zip(layers, acts):
        lin = torch.nn.Linear(w.shape[1], w.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(w.double())
            lin.bias.copy_(b.double())
        mods.append(lin)
        if a is not None:
            mods.append(getattr(torch.nn, a)().double())
    return torch.nn.Sequential(*mods)


# (a stack whose first layer is Hardsigmoid is left out: on these frames torch's own fp32 step departs from its fp64
# step by 2e-4 after 3 Adam steps -- tiny weight gradients, which Adam normalises, meet fp32 rounding)
@pytest.mark.parametrize("acts", [("ELU", "Sigmoid", None), ("LeakyReLU", "SELU", "Softplus"),
                                  ("ReLU6", "Softsign", "Hardsigmoid"), ("Softsign", "ReLU6", "Hardtanh"),
                                  ("CELU", "LogSigmoid", "Sigmoid"), ("Tanh", "ReLU", "Tanh")])
def test_flat_step_matches_a_float64_stack_and_is_deterministic(gpu, acts):
    """FlatFFModel.train_step with mixed activations (the output layer fused with the loss when it has none, a
    separate masked MSE and the output activation's derivative otherwise): 3 Adam steps against torch in float64 on
    the same frames, and bit-identical parameters when run again"""
    dims = (64, 96, 80, 67)
    runs = []
    for _ in range(2):
        model = FlatFFModel(dims, acts, device=gpu, seed=6)
        ref = _ref_stack(model.layers(), acts)
        opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
        losses = []
        for step in range(3):
            g = torch.Generator().manual_seed(300 + step)
            M = 500 + 37 * step
            x = torch.randn(M, dims[0], generator=g) * 2
            t = torch.randn(M, dims[-1], generator=g)
            valid = torch.ones(M, dtype=torch.uint8, device=gpu)
            valid[-5:] = 0                                   # frames outside the loss
            vmask = valid.cpu().double()[:, None]
            n_valid = float(vmask.sum())
            pred = ref(x.double())
            ref_loss = (((pred - t.double()) ** 2) * vmask).sum() / (n_valid * dims[-1])
            opt.zero_grad()
            ref_loss.backward()
            opt.step()
            loss = model.train_step(x.to(gpu), t.to(gpu), valid, n_valid)
            losses.append(float(loss))
            assert abs(float(loss) - ref_loss.item()) < 1e-5 * abs(ref_loss.item())
        lins = [m for m in ref if isinstance(m, torch.nn.Linear)]
        for i, lin in enumerate(lins):
            assert (model.weight(i).cpu().double() - lin.weight.detach()).abs().max().item() < 2e-6
            assert (model.bias(i).cpu().double() - lin.bias.detach()).abs().max().item() < 2e-6
        runs.append((losses, model.params.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("resident", [False, True])
def test_trainer_reproduces_reference_losses(gpu, ffact_golden, golden_dir, tmp_path, resident):
    """The reference AcousticModelTrainer run of make_golden_ffact.py (trainer data of trainer_fixture.npz, seed 1234,
    3 epochs, batch size 2, Adam 1e-3, batch_first) with a new-style model_config of ELU / Sigmoid / Softsign groups:
    same initial weights, per-epoch losses to rtol 2e-5 and final weights -- on the module path and with
    hparams.resident_dataset (the flat feed-forward step)"""
    from idiaptts_amd.src.model_trainers.AcousticModelTrainer import AcousticModelTrainer
    from idiaptts_amd.src.neural_networks.pytorch.models.NamedForwardWrapper import NamedForwardWrapper
    g = ffact_golden
    root = str(tmp_path)
    ids, wdir, qdir, _ = materialise(golden_dir, root)
    hp = AcousticModelTrainer.create_hparams()
    hp.num_questions = 409
    hp.voice = "full"
    hp.out_dir = os.path.join(root, "ffact_train")
    hp.frame_size_ms = 5
    hp.num_coded_sps = 20
    hp.seed = 1234
    hp.epochs = 3
    hp.use_gpu = True
    hp.dataset_num_workers_gpu = 0
    hp.batch_first = True
    hp.batch_size_train = 2
    hp.batch_size_val = 50
    hp.use_saved_learning_rate = True
    hp.optimiser_args["lr"] = 0.001
    hp.model_name = "test_model"
    hp.epochs_per_checkpoint = 2
    hp.world_dir = wdir
    hp.use_best_as_final_model = False
    hp.resident_dataset = resident
    trainer = AcousticModelTrainer(**AcousticModelTrainer.legacy_support_init(wdir, qdir, ids, hp.num_questions, hp))
    trainer.init(hp, model_config=trainer_model_config(rnn_dyn, NamedForwardWrapper))
    sd = trainer.model_handler.model.state_dict()
    init = {k[len("trainer/init/"):] for k in g.files if k.startswith("trainer/init/")}
    assert set(sd.keys()) == init
    for k in init:
        assert np.array_equal(sd[k].cpu().numpy(), g["trainer/init/" + k]), k
    all_loss, all_loss_train, handler = trainer.train(hp)
    if resident:
        assert handler._resident is not None and handler._resident["flat"] is not None
        assert handler._resident["flat"].acts == [ops.ACT_ELU, ops.ACT_SIGMOID, ops.ACT_SOFTSIGN, ops.ACT_NONE]
    key = "MSELoss_acoustic_features"
    np.testing.assert_allclose(all_loss[key], g["trainer/val_losses"], rtol=2e-5)
    np.testing.assert_allclose(all_loss_train[key], g["trainer/train_losses"], rtol=2e-5)
    sd = handler.model.state_dict()
    for k in sd:
        np.testing.assert_allclose(sd[k].cpu().numpy(), g["trainer/final/" + k], rtol=0, atol=2e-5)
