"""csrc/mol.hip's loss on the GPU, through `ops`, against the float64 restatement of mol_cases.py (pinned to the
reference's float64 fixture by tests/test_mol_cases.py): the sweep over K, T, shift, num_classes, log_scale_min and
hinge, weight-zero rows holding NaN / inf / out-of-range targets, absent outputs, repeated calls, a frame's bits under
another batch size and another position, every refusal; then the module, NamedLoss with every reduction, and one
backward pass with a non-unit incoming gradient against tests/golden/mol_fixture.npz.

The bound of every comparison is the larger of the dense layers' (xent_cases.REL_BOUND / ELEM_BOUND) and twice the
error of torch's own float32 flow on the same data (mol_cases.check); each case prints its error as a fraction of it."""
import itertools
import os

import numpy as np
import pytest
import torch

import mol_cases as mc
from idiaptts_amd import lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mol_fixture.npz")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _call(x, y, w, nc, lsm, shift, hinge, **kw):
    kw.setdefault("want_elem", True)
    return ops.mol_loss(torch.as_tensor(x).to(DEV), torch.as_tensor(y).to(DEV), torch.as_tensor(w).to(DEV), nc, lsm,
                        shift, hinge, **kw)


def _weights(B, Tn, seed):
    return (0.5 + np.random.default_rng(seed).random((B, Tn))).astype(np.float32)


def _check_all(got, x, y, w, nc, lsm, shift, hinge, what):
    loss, grad, elem = got
    ref = mc.reference64(x, y, w, nc, lsm, shift, hinge)
    t32 = mc.torch32(torch, x, y, w, nc, lsm, shift, hinge)
    fr = []
    for product, g in (("elem", elem), ("grad", grad), ("loss", loss)):
        fr.extend(mc.check(product, g.cpu().numpy(), ref[product], t32[product].numpy(), what))
    return max(fr)


def _sweep(K, T):
    B, worst = mc.SWEEP_B, 0.0
    for n, (shift, nc, lsm, hinge) in enumerate(itertools.product(mc.SWEEP_SHIFT, mc.NUM_CLASSES, mc.LOG_SCALE_MINS,
                                                                  (True, False))):
        if shift >= T:          # (refused: test_refusals)
            continue
        x, y = mc.inputs(B, K, T, nc, lsm, shift, seed=n)
        w = _weights(B, T - shift, 100 * K + n)
        got = _call(x, y, w, nc, lsm, shift, hinge)
        assert got[1].shape == (B, 3 * K, T) and got[2].shape == (B, T - shift)
        if shift:
            assert got[1][:, :, T - shift:].abs().max().item() == 0         # the frames without a loss: written, zeros
        worst = max(worst, _check_all(got, x, y, w, nc, lsm, shift, hinge,
                                      "K{} T{} s{} nc{} lsm{:.0f} h{}".format(K, T, shift, nc, lsm, int(hinge))))
    print("mol sweep K{} T{}: largest error {:.3f} of its bound".format(K, T, worst))


@pytest.mark.parametrize("T", mc.SWEEP_T)
@pytest.mark.parametrize("K", mc.SWEEP_K)
def test_sweep(K, T):
    _sweep(K, T)


@pytest.mark.parametrize("K", (16, 17, 32, 33))
def test_sweep_at_the_workgroup_sizes(K):
    """256 lanes a workgroup up to K = 16, 128 up to 32, 64 above: both sides of each threshold, at more than one
    workgroup of either size"""
    _sweep(K, 129)


def _base_case(B=3, K=10, T=130, nc=65536, lsm=-7.0, shift=1, seed=5):
    x, y = mc.inputs(B, K, T, nc, lsm, shift, seed=seed)
    return x, y, _weights(B, T - shift, 77), nc, lsm, shift


def test_weight_zero_rows_are_never_read():
    x, y, w, nc, lsm, shift = _base_case()
    B, _, T = x.shape
    w[0, 3] = w[1, 64] = w[2, T - shift - 1] = w[2, 0] = 0.0
    base = _call(x, y, w, nc, lsm, shift, True)
    _check_all(base, x, y, w, nc, lsm, shift, True, "weight-zero rows")
    xb, yb = x.copy(), y.copy()
    for (b, t), (vx, vy) in zip(((0, 3), (1, 64), (2, T - shift - 1), (2, 0)),
                                ((np.nan, 0.0), (np.inf, 5.0), (-np.inf, np.nan), (1e30, -7.0))):
        xb[b, :, t] = vx
        yb[b, 0, t + shift] = vy          # (read by frame t alone)
    got = _call(xb, yb, w, nc, lsm, shift, True)
    assert all(_same_bits(a, b) for a, b in zip(got, base))
    for b, t in ((0, 3), (1, 64), (2, T - shift - 1), (2, 0)):
        assert got[2][b, t].item() == 0 and got[1][b, :, t].abs().max().item() == 0
    assert torch.isfinite(got[0]).all()


def test_absent_outputs_and_repeated_calls():
    x, y, w, nc, lsm, shift = _base_case()
    base = _call(x, y, w, nc, lsm, shift, True)
    again = _call(x, y, w, nc, lsm, shift, True)
    assert all(_same_bits(a, b) for a, b in zip(again, base))
    l1, g1, e1 = _call(x, y, w, nc, lsm, shift, True, want_grad=False)
    assert g1 is None and _same_bits(l1, base[0]) and _same_bits(e1, base[2])
    l2, g2, e2 = _call(x, y, w, nc, lsm, shift, True, want_elem=False)
    assert e2 is None and _same_bits(l2, base[0]) and _same_bits(g2, base[1])


@pytest.mark.parametrize("K", (3, 20, 64))           # workgroups of 256, 128 and 64 lanes
def test_frame_bits_depend_on_the_frame_alone(K):
    x, y, w, nc, lsm, shift = _base_case(K=K, T=300)
    _, grad, elem = _call(x, y, w, nc, lsm, shift, True)
    # one batch entry alone
    _, g1, e1 = _call(x[1:2], y[1:2], w[1:2], nc, lsm, shift, True)
    assert _same_bits(g1[0], grad[1]) and _same_bits(e1[0], elem[1])
    # the same frames 37 positions earlier (another lane, another workgroup)
    _, g2, e2 = _call(x[:, :, 37:], y[:, :, 37:], w[:, 37:], nc, lsm, shift, True)
    assert _same_bits(g2, grad[:, :, 37:]) and _same_bits(e2, elem[:, 37:])


def test_refusals():
    x, y, w, nc, lsm, shift = _base_case(B=2, K=2, T=8)
    for bad, text in ((dict(nc=1), "num_classes = 1"), (dict(nc=0), "num_classes = 0")):
        with pytest.raises(lib.IttsError, match=text):
            _call(x, y, w, bad["nc"], lsm, shift, True)
    x65 = np.zeros((2, 3 * 65, 8), dtype=np.float32)
    with pytest.raises(lib.IttsError, match="K = 65"):
        _call(x65, y, w, nc, lsm, shift, True)
    with pytest.raises(ValueError, match="C = 7"):
        _call(np.zeros((2, 7, 8), dtype=np.float32), y, w, nc, lsm, shift, True)
    for s in (8, 9, -1):
        with pytest.raises(ValueError, match="shift = {}".format(s)):
            _call(x, y, np.ones((2, max(8 - s, 0)), dtype=np.float32), nc, lsm, s, True)
    with pytest.raises(ValueError, match="row_weight has"):
        _call(x, y, w[:, :-1], nc, lsm, shift, True)
    # the C entry point itself refuses the shift too, before any device work
    L = lib.load()
    assert L.itts_mol_loss(None, None, None, 2, 2, 8, 8, 256, -7.0, 1, None, None, None, None, None) == -1
    assert b"shift = 8" in L.itts_last_error()
    # B == 0: loss 0
    loss, grad, elem = _call(x[:0], y[:0], w[:0], nc, lsm, shift, True)
    assert loss.item() == 0 and grad.shape == (0, 6, 8) and elem.shape == (0, 7)


# ---- module and NamedLoss against the reference's float64 fixture ------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _golden_case(golden, case):
    p = mc.case_name(*case) + "/"
    return golden[p + "x"], golden[p + "y"], golden[p + "w"], golden[p + "elem"], golden[p + "grad"]


@pytest.mark.parametrize("case", mc.GOLDEN_CASES, ids=lambda c: mc.case_name(*c))
def test_module_matches_the_reference_fixture(golden, case):
    from idiaptts_amd.src.neural_networks.pytorch.loss.DiscretizedMixturelogisticLoss import \
        DiscretizedMixturelogisticLoss
    K, nc, lsm, shift, hinge = case
    x, y, w, elem, grad = _golden_case(golden, case)
    t32 = mc.torch32(torch, x, y, w, nc, lsm, shift, hinge)
    leaf = torch.from_numpy(x).to(DEV).requires_grad_(True)
    out = DiscretizedMixturelogisticLoss(nc, lsm, shift=shift, hinge_loss=hinge)(leaf, torch.from_numpy(y).to(DEV))
    assert out.shape == elem.shape
    # a non-unit incoming gradient: the fixture's gradient is that of sum(w elem)
    (out[..., 0] * torch.from_numpy(w).float().to(DEV)).sum().backward()
    name = mc.case_name(*case)
    mc.check("elem", out.detach().cpu().numpy()[..., 0] * w, elem[..., 0] * w, t32["elem"].numpy(), name)
    mc.check("grad", leaf.grad.cpu().numpy(), grad, t32["grad"].numpy(), name)
    # the CPU path of the module: the same values
    cpu = DiscretizedMixturelogisticLoss(nc, lsm, shift=shift, hinge_loss=hinge)(torch.from_numpy(x),
                                                                                 torch.from_numpy(y))
    mc.check("elem", cpu.numpy()[..., 0] * w, elem[..., 0] * w, t32["elem"].numpy(), name + " cpu")


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("reduction", mc.REDUCTIONS)
def test_named_loss_reductions(golden, reduction, masked):
    from idiaptts_amd.src.neural_networks.pytorch.loss.NamedLoss import NamedLoss
    case = (10, 65536, -7.0, 1, True)
    K, nc, lsm, shift, hinge = case
    x, y, _, elem, _ = _golden_case(golden, case)
    B, Tn = elem.shape[:2]
    lens = [Tn, Tn - 4]
    mask = (np.arange(Tn)[None, :] < np.array(lens)[:, None]).astype(np.float32) if masked else np.ones((B, Tn),
                                                                                                        np.float32)
    cfg = NamedLoss.Config(name="mol", type_="DiscretizedMixturelogisticLoss", input_names=["pred", "wave"],
                           seq_mask="mask" if masked else None, batch_first=True, reduction=reduction,
                           num_classes=nc, log_scale_min=lsm, shift=shift, hinge_loss=hinge)
    effective = "mean" if not masked and reduction in ("mean_per_frame", "mean_per_sample") else reduction
    assert cfg.reduction == effective
    wr = mc.reduction_weight(effective, mask, lens)
    leaf = torch.from_numpy(x).to(DEV).requires_grad_(True)
    data = {"pred": leaf, "wave": torch.from_numpy(y).to(DEV)}
    if masked:
        data["mask"] = torch.from_numpy(mask).to(DEV).unsqueeze(-1)
    out = cfg.create_loss()(data, {"mask": torch.tensor(lens)}, 0)["mol"]
    ref = mc.reference64(x, y, wr, nc, lsm, shift, hinge)
    t32 = mc.torch32(torch, x, y, wr.astype(np.float32), nc, lsm, shift, hinge)
    what = "NamedLoss {} {}".format(reduction, "masked" if masked else "no mask")
    if effective == "none":
        assert out.shape == (B, Tn, 1)
        np.testing.assert_allclose(ref["elem"], elem[..., 0] * wr, rtol=1e-8, atol=1e-8)   # restatement == fixture
        mc.check("elem", out.detach().cpu().numpy(), elem[..., 0] * wr, t32["elem"].numpy(), what)
        out.sum().backward()
    else:
        assert out.dim() == 0
        mc.check("loss", out.detach().cpu().numpy(), (elem[..., 0] * wr).sum(), t32["loss"].numpy(), what)
        out.backward()
    mc.check("grad", leaf.grad.cpu().numpy(), ref["grad"], t32["grad"].numpy(), what)
    # the CPU path gives the same value
    cpu = cfg.create_loss()({k: v.detach().cpu() for k, v in data.items()}, {"mask": torch.tensor(lens)}, 0)["mol"]
    if effective == "none":
        mc.check("elem", cpu.numpy(), elem[..., 0] * wr, t32["elem"].numpy(), what + " cpu")
    else:
        mc.check("loss", cpu.numpy(), (elem[..., 0] * wr).sum(), t32["loss"].numpy(), what + " cpu")
