"""GPU tests of the WaveNet vocoder network against the float64 spec (tests/wavenet_spec.py): the gate kernel pair,
the teacher-forced forward / loss / parameter gradients, generation (itts_wavenet_generate) and the wrapper.

Bounds.  Dense comparisons use the dense layers' bounds (xent_cases.REL_BOUND / ELEM_BOUND: relative 2-norm error and
largest element error over max(1, max |ref|)), or twice the error of torch's own float32 flow of the spec on the same
data where that is larger (the rule of mol_cases.check); every case prints its error as a fraction of its bound.
Generated class indices must EQUAL the spec's at every step: the spec moves a uniform that falls within 1e-3 of an edge
of its own float64 CDF to the middle of an interval (wavenet_spec.generate), the kernel is given those uniforms, and
float32 logits (errors ~1e-6) cannot cross 1e-3."""
import numpy as np
import pytest
import torch

import mol_cases as mc
import wavenet_spec as ws
from xent_cases import ELEM_BOUND, REL_BOUND

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MARGIN = 1e-3


def _errors(got, ref):
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return float(np.linalg.norm(d) / (np.linalg.norm(ref) + 1e-30)), float(d.max() / max(1.0, np.abs(ref).max()))


def _check(product, got, ref, t32=None, what=""):
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (what, "non-finite values")
    tol_rel, tol_el = REL_BOUND[product], ELEM_BOUND
    r32 = 0.0
    if t32 is not None:
        r32, e32 = _errors(np.asarray(t32, dtype=np.float64).reshape(-1), ref)
        tol_rel, tol_el = max(tol_rel, 2 * r32), max(tol_el, 2 * e32)
    rel, el = _errors(got, ref)
    print("wavenet {} {}: rel {:.3g} ({:.2f} of bound {:.3g}; torch32 {:.3g}), elem {:.3g} ({:.2f} of bound)".format(
        what, product, rel, rel / tol_rel, tol_rel, r32, el, el / tol_el))
    assert rel < tol_rel and el < tol_el, (product, what, rel, tol_rel, el, tol_el)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- gate ----------------------------------------------------------------------------------------------------------
def _gate64(x, c, dz):
    x = torch.from_numpy(x).double().requires_grad_(True)
    c = torch.from_numpy(c).double().requires_grad_(True) if c is not None else None
    a = x if c is None else x + c
    H = x.shape[1] // 2
    z = torch.tanh(a[:, :H]) * torch.sigmoid(a[:, H:])
    z.backward(torch.from_numpy(dz).double())
    return z.detach().numpy(), x.grad.numpy()


def _pitched(a, pad):
    """a [N, W] on the device as a view of rows `pad` floats wider, starting one float into the storage when pad is
    odd: an unaligned base and a pitch that is no multiple of four"""
    N, W = a.shape
    buf = torch.full((N * (W + pad) + 1,), 7.0, dtype=torch.float32, device=DEV)
    view = buf[pad % 2:pad % 2 + N * (W + pad)].view(N, W + pad)[:, :W]
    view.copy_(torch.from_numpy(a))
    return view


@pytest.mark.parametrize("with_c", [False, True], ids=["noc", "c"])
@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("G", [2, 32, 34, 512])
def test_gate_forward_and_backward(G, N, with_c):
    from idiaptts_amd import ops
    from idiaptts_amd.nn.functional import GluGateFunction
    rng = np.random.default_rng(1000 * G + N + int(with_c))
    x = (2.0 * rng.standard_normal((N, G))).astype(np.float32)
    c = rng.standard_normal((N, G)).astype(np.float32) if with_c else None
    dz = (0.5 + rng.random((N, G // 2))).astype(np.float32) * 3.0           # a non-unit incoming gradient
    z64, dx64 = _gate64(x, c, dz)
    for pad in (0, 4, 3):                                                   # contiguous, aligned pitch, unaligned
        xd, dzd = _pitched(x, pad), _pitched(dz, pad)
        cd = _pitched(c, pad) if with_c else None
        what = "gate G{} N{} c{} pad{}".format(G, N, int(with_c), pad)
        z = ops.glu_gate(xd, cd)
        _check("elem", z.cpu().numpy(), z64, what=what)
        dx = ops.glu_gate_bwd(dzd, xd, cd)
        assert dx.shape == (N, G)
        _check("grad", dx.cpu().numpy(), dx64, what=what)
        zout = _pitched(np.zeros((N, G // 2), np.float32), pad)
        ops.glu_gate(xd, cd, out=zout)
        assert torch.equal(_bits(zout), _bits(z))
        if pad:                                                             # nothing written between the rows
            assert (zout.as_strided((N, pad), (G // 2 + pad, 1), zout.storage_offset() + G // 2)[:-1] == 7.0).all()
    # through autograd: one buffer for both gradients
    xl = torch.from_numpy(x).to(DEV).requires_grad_(True)
    cl = torch.from_numpy(c).to(DEV).requires_grad_(True) if with_c else None
    GluGateFunction.apply(xl, cl).backward(torch.from_numpy(dz).to(DEV))
    _check("grad", xl.grad.cpu().numpy(), dx64, what="gate autograd G{} N{}".format(G, N))
    if with_c:
        assert torch.equal(_bits(cl.grad), _bits(xl.grad))


# ---- the small models ----------------------------------------------------------------------------------------------
def _wrapper(net, sd, weight_normalization=True, dropout=0.0):
    from idiaptts_amd.src.neural_networks.pytorch.models.WaveNetWrapper import WaveNetWrapper
    model = WaveNetWrapper.Config(layers=net.layers, stacks=net.stacks, residual_channels=net.R, gate_channels=net.G,
                                  skip_out_channels=net.S, kernel_size=net.k, cin_channels=net.cin,
                                  out_channels=net.C, scalar_input=net.scalar, dropout=dropout,
                                  weight_normalization=weight_normalization).create_model()
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)).float() for k, v in sd.items()})
    return model.to(DEV)


def _cond(net, B, T, seed):
    return np.random.default_rng(seed).standard_normal((B, net.cin, T)).astype(np.float32)


def _tensors(sd, dtype):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in sd.items()}


MODELS = [(2, False), (3, False), (2, True)]
MODEL_IDS = ["k2", "k3", "mol"]
TRAIN_LENGTHS, TRAIN_T = [70, 41, 9], 70
NUM_CLASSES_MOL = 256


def _train_data(net, seed):
    rng = np.random.default_rng(seed)
    B, T = len(TRAIN_LENGTHS), TRAIN_T
    if net.scalar:
        target = rng.uniform(-0.95, 0.95, size=(B, 1, T)).astype(np.float32)
    else:
        target = np.zeros((B, net.C, T), dtype=np.float32)
        idx = rng.integers(0, net.C, size=(B, T))
        for b in range(B):
            target[b, idx[b], np.arange(T)] = 1.0
    lens = [n - 1 for n in TRAIN_LENGTHS]                                   # frames with a loss (shift 1)
    mask = (np.arange(T - 1)[None, :] < np.array(lens)[:, None]).astype(np.float32)
    return target, _cond(net, B, T, seed + 1), lens, mask


def _spec_loss(net, sd, target, c, w, dtype):
    """(logits, loss, {key: gradient}) of the spec in `dtype` on the CPU; w [B, T - 1] row weights"""
    t = _tensors(sd, dtype)
    logits = ws.forward(torch, net, t, torch.from_numpy(target).to(dtype), torch.from_numpy(c).to(dtype))
    if net.scalar:
        f = mc.reference64 if dtype == torch.float64 else None
        x = logits.detach().numpy()
        if f is not None:
            assert not mc.offending(x.astype(np.float32), target, NUM_CLASSES_MOL, net.log_scale_min, 1).any()
            r = f(x, target, w, NUM_CLASSES_MOL, net.log_scale_min, 1, True)
            loss, grad = r["loss"], torch.from_numpy(r["grad"])
        else:
            r = mc.torch32(torch, x, target, w.astype(np.float32), NUM_CLASSES_MOL, net.log_scale_min, 1, True)
            loss, grad = r["loss"].item(), r["grad"]
        logits.backward(grad.to(dtype))
    else:
        idx = torch.from_numpy(target.argmax(axis=1))[:, 1:]
        lp = torch.log_softmax(logits[:, :, :-1], dim=1)
        elem = -lp.gather(1, idx.unsqueeze(1))[:, 0] * torch.from_numpy(w).to(dtype)
        total = elem.sum()
        total.backward()
        loss = total.item()
    # (the last layer's conv1x1_out feeds nothing: its parameters get no gradient, which stands for zeros)
    return logits.detach().numpy(), loss, {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy()
                                           for k, v in t.items()}


@pytest.mark.parametrize("k,mol", MODELS, ids=MODEL_IDS)
def test_training_forward_loss_and_parameter_gradients(k, mol):
    from idiaptts_amd.src.neural_networks.pytorch.loss.NamedLoss import NamedLoss
    net = ws.small(k=k, mol=mol)
    sd = ws.random_state(net, seed=11 + k)
    target, c, lens, mask = _train_data(net, seed=20 + k)
    w = mask.astype(np.float64) / float(sum(lens))                          # mean_per_frame
    ref_logits, ref_loss, ref_grads = _spec_loss(net, sd, target, c, w, torch.float64)
    t32_logits, t32_loss, t32_grads = _spec_loss(net, sd, target, c, w, torch.float32)

    model = _wrapper(net, sd).train()
    out, none = model(torch.from_numpy(c).to(DEV), torch.from_numpy(target).to(DEV), torch.tensor(TRAIN_LENGTHS))
    assert none is None and out.shape == (len(TRAIN_LENGTHS), net.C, TRAIN_T)
    what = "train k{}{}".format(k, " mol" if mol else "")
    _check("elem", out.detach().cpu().numpy(), ref_logits, t32_logits, what + " logits")
    if mol:
        cfg = NamedLoss.Config(name="loss", type_="DiscretizedMixturelogisticLoss", input_names=["pred", "wave"],
                               seq_mask="mask", batch_first=True, reduction="mean_per_frame",
                               num_classes=NUM_CLASSES_MOL, log_scale_min=net.log_scale_min, shift=1, hinge_loss=True)
    else:
        cfg = NamedLoss.Config(name="loss", type_="OneHotCrossEntropyLoss", input_names=["pred", "wave"],
                               seq_mask="mask", batch_first=True, reduction="mean_per_frame", shift=1)
    data = {"pred": out, "wave": torch.from_numpy(target).to(DEV), "mask": torch.from_numpy(mask).to(DEV).unsqueeze(-1)}
    loss = cfg.create_loss()(data, {"mask": torch.tensor(lens)}, 0)["loss"]
    _check("loss", loss.detach().cpu().numpy(), ref_loss, t32_loss, what + " loss")
    loss.backward()
    names = dict(model.named_parameters())
    assert set(names) == set(ref_grads)
    for key in sorted(ref_grads):
        assert key.rsplit(".", 1)[1] in ("weight_g", "weight_v", "bias")
        grad = names[key].grad if names[key].grad is not None else torch.zeros_like(names[key])
        if mol and key == "model.first_conv.weight_v":
            # one input channel: w = g v / |v| = g sign(v) does not depend on |v|, the exact gradient is zero (the
            # float64 flow leaves rounding noise), so there is no norm to be relative to: the element bound alone
            assert np.abs(ref_grads[key]).max() < 1e-14
            assert grad.abs().max().item() < ELEM_BOUND
            continue
        _check("grad", grad.cpu().numpy(), ref_grads[key], t32_grads[key], what + " d " + key)


# ---- generation ----------------------------------------------------------------------------------------------------
GEN_T = 70
GEN_LENGTHS = [70, 1, 33, 70, 5, 64, 70, 12, 70, 48, 3, 70, 69, 17, 70, 2, 70]     # 17 rows: two tiles


class _GenCase(object):
    """one model, the 17-row batch, the spec's generation of it (computed once, never changed)"""
    _cache = {}

    @classmethod
    def get(cls, k, mol):
        if (k, mol) not in cls._cache:
            cls._cache[(k, mol)] = cls(k, mol)
        return cls._cache[(k, mol)]

    def __init__(self, k, mol):
        self.net = ws.small(k=k, mol=mol)
        assert GEN_T > ws.receptive_field(self.net) and GEN_T > max((k - 1) * d + 1 for d in ws.dilations(self.net))
        self.sd = ws.random_state(self.net, seed=31 + k, scale=1.5)
        self.c = _cond(self.net, 17, GEN_T, seed=41)
        self.spec = ws.generate(self.net, self.sd, self.c.astype(np.float64), GEN_LENGTHS,
                                ws.draw_uniforms(self.net, 17, GEN_T, seed=51), margin=MARGIN)
        self.model = _wrapper(self.net, self.sd).eval()

    def run(self, rows):
        """the kernel on the rows `rows` of the batch: (out, logits) numpy"""
        lengths = [GEN_LENGTHS[r] for r in rows]
        T = max(lengths)
        u = torch.from_numpy(self.spec["uniforms"][rows][:, :T].copy()).to(DEV)
        c = torch.from_numpy(self.c[rows][:, :, :T].copy()).to(DEV)
        out, logits = self.model.model.generate(c, lengths, uniforms=u, return_logits=True)
        return out, logits, lengths


@pytest.mark.parametrize("rows", [[16], [0, 1, 2], list(range(17))], ids=["B1", "B3", "B17"])
@pytest.mark.parametrize("k,mol", MODELS, ids=MODEL_IDS)
def test_generation_equals_the_spec(k, mol, rows):
    case = _GenCase.get(k, mol)
    net, spec = case.net, case.spec
    out, logits, lengths = case.run(rows)
    T = max(lengths)
    assert out.shape == (len(rows), T) and logits.shape == (len(rows), T, net.C)
    assert out.dtype == (torch.float32 if mol else torch.int32)
    again, logits_again, _ = case.run(rows)
    assert torch.equal(_bits(out), _bits(again)) and torch.equal(_bits(logits), _bits(logits_again))
    o, lg = out.cpu().numpy(), logits.cpu().numpy()
    for i, n in enumerate(lengths):
        assert not o[i, n:].any() and not lg[i, n:].any()                    # zeros past the row's length
    if not mol:
        assert np.array_equal(o, spec["out"][rows][:, :T])                  # every step, no exemption
    # the logits against the teacher-forced spec over the kernel's own history, float64 and float32
    x = ws.teacher_input(net, o)
    c = case.c[rows][:, :, :T]
    sd64 = {k_: torch.from_numpy(np.asarray(v)) for k_, v in case.sd.items()}
    sd32 = {k_: v.float() for k_, v in sd64.items()}
    tf64 = ws.forward(torch, net, sd64, torch.from_numpy(x), torch.from_numpy(c).double()).transpose(1, 2).numpy()
    tf32 = ws.forward(torch, net, sd32, torch.from_numpy(x).float(), torch.from_numpy(c)).transpose(1, 2).numpy()
    live = np.arange(T)[None, :] < np.array(lengths)[:, None]
    what = "generate k{}{} B{}".format(k, " mol" if mol else "", len(rows))
    _check("elem", lg[live], tf64[live], tf32[live], what + " logits")
    if mol:
        u = spec["uniforms"][rows][:, :T].astype(np.float64)
        want = np.zeros_like(tf64[..., 0])
        want32 = np.zeros_like(want)
        for i, n in enumerate(lengths):
            for t in range(n):
                want[i, t], mix, _ = ws.draw_mol(tf64[i, t], u[i, t, 0], u[i, t, 1], net.log_scale_min)
                assert mix == spec["mixture"][rows[i], t]
                want32[i, t] = ws.draw_mol(tf32[i, t].astype(np.float64), u[i, t, 0], u[i, t, 1], net.log_scale_min)[0]
        _check("elem", o[live], want[live], want32[live], what + " samples")
        assert np.abs(o).max() <= 1.0


@pytest.mark.parametrize("k,mol", MODELS, ids=MODEL_IDS)
def test_a_row_has_the_same_bits_alone_and_at_position_16_of_17(k, mol):
    case = _GenCase.get(k, mol)
    alone, alone_logits, _ = case.run([16])
    batch, batch_logits, _ = case.run(list(range(17)))
    assert torch.equal(_bits(alone[0]), _bits(batch[16]))
    assert torch.equal(_bits(alone_logits[0]), _bits(batch_logits[16]))
    # and the first tile's rows do not change when the second tile is there
    three, three_logits, _ = case.run([0, 1, 2])
    assert torch.equal(_bits(three), _bits(batch[:3])) and torch.equal(_bits(three_logits), _bits(batch_logits[:3]))


def test_initial_class_feeds_step_zero():
    case = _GenCase.get(2, False)
    net = case.net
    u = torch.from_numpy(case.spec["uniforms"][:1, :4].copy()).to(DEV)
    c = torch.from_numpy(case.c[:1, :, :4].copy()).to(DEV)
    _, logits = case.model.model.generate(c, [4], uniforms=u, return_logits=True, initial_class=5)
    spec = ws.generate(net, case.sd, case.c[:1].astype(np.float64), [1], case.spec["uniforms"][:1, :1], initial_class=5)
    x = np.zeros((1, net.C, 1), dtype=np.float32)
    x[0, 5, 0] = 1.0
    sd32 = {k_: torch.from_numpy(np.asarray(v)).float() for k_, v in case.sd.items()}
    tf32 = ws.forward(torch, net, sd32, torch.from_numpy(x), torch.from_numpy(case.c[:1, :, :1]))[0, :, 0].numpy()
    _check("elem", logits[0, 0].cpu().numpy(), spec["logits"][0, 0], tf32, what="initial_class")
    assert np.abs(spec["logits"][0, 0] - case.spec["logits"][0, 0]).max() > 1e-3


def test_generation_at_the_default_config_widths():
    """R 512, G 512, S 256, cin 80, 256 classes, 24 layers / 4 stacks, kernel 3: the deepest ring buffer (2 * 32 + 1
    slots) wraps twice in 140 steps"""
    net = ws.DEFAULT
    lengths, T = [140, 97], 140
    assert T > 2 * (2 * 32 + 1)
    sd = ws.random_state(net, seed=7)
    c = _cond(net, 2, T, seed=8)
    spec = ws.generate(net, sd, c.astype(np.float64), lengths, ws.draw_uniforms(net, 2, T, seed=9), margin=MARGIN)
    model = _wrapper(net, sd).eval()
    out = model.model.generate(torch.from_numpy(c).to(DEV), lengths,
                               uniforms=torch.from_numpy(spec["uniforms"]).to(DEV)).cpu().numpy()
    wrong = np.argwhere(out != spec["out"])
    assert wrong.size == 0, ("first differing (row, step)", wrong[:4].tolist())
    assert len(np.unique(out[0])) > 16


# ---- the wrapper ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mol", [False, True], ids=["mulaw", "mol"])
def test_wrapper_inference_shapes_and_checkpoint_round_trip(mol):
    case = _GenCase.get(2, mol)
    net, model = case.net, case.model
    lengths = [33, 70, 5]
    rows = [2, 3, 4]
    c = torch.from_numpy(case.c[rows].copy()).to(DEV)
    u = torch.from_numpy(case.spec["uniforms"][rows].copy()).to(DEV)
    out, none = model(c, None, torch.tensor(lengths), uniforms=u)
    assert none is None and out.shape == (3, 1 if mol else net.C, 70) and out.dtype == torch.float32
    o = out.cpu().numpy()
    for i, n in enumerate(lengths):
        assert not o[i, :, n:].any()
        if not mol:
            assert np.array_equal(o[i, :, :n].sum(axis=0), np.ones(n))
            assert np.array_equal(o[i, :, :n].argmax(axis=0), case.spec["out"][rows[i], :n])
    assert model.has_weight_norm
    # len_in_out_multiplier scales the lengths
    model.len_in_out_multiplier = 2
    try:
        assert model(c, None, [16, 35, 2], uniforms=u)[0].shape[-1] == 70
    finally:
        model.len_in_out_multiplier = 1
    # a second model built from the checkpoint generates the same bits
    other = _wrapper(net, {k: v.cpu().numpy() for k, v in model.state_dict().items()})
    assert torch.equal(_bits(other(c, None, lengths, uniforms=u)[0]), _bits(out))
    # waveforms: the classes decoded / the samples, one tensor per row
    waves = model.generate_waveform(c, lengths, uniforms=u)
    assert [w.shape[0] for w in waves] == lengths and all(w.dtype == torch.float64 for w in waves)
    if mol:
        assert torch.equal(waves[1].float(), out[1, 0])
    else:
        from idiaptts_amd import ops
        idx = torch.from_numpy(case.spec["out"][3]).to(DEV)
        assert torch.equal(waves[1], ops.mulaw_decode(idx, [0, 70], mu=net.C - 1))
    # draws of its own: reproducible with a seeded generator
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    a = model(c, None, lengths, generator=g)[0]
    g.manual_seed(3)
    assert torch.equal(_bits(a), _bits(model(c, None, lengths, generator=g)[0]))


def test_five_adam_steps_lower_the_loss_and_generation_still_works():
    from idiaptts_amd.src.neural_networks.pytorch.loss.NamedLoss import NamedLoss
    from idiaptts_amd.src.neural_networks.pytorch.ModularModelHandlerPyTorch import HipAdam
    net = ws.small(k=3)
    model = _wrapper(net, ws.random_state(net, seed=61), dropout=0.05).train()
    target, c, lens, mask = _train_data(net, seed=62)
    cfg = NamedLoss.Config(name="loss", type_="OneHotCrossEntropyLoss", input_names=["pred", "wave"],
                           seq_mask="mask", batch_first=True, reduction="mean_per_frame", shift=1)
    loss_fn = cfg.create_loss()
    data = {"wave": torch.from_numpy(target).to(DEV), "mask": torch.from_numpy(mask).to(DEV).unsqueeze(-1)}
    cd = torch.from_numpy(c).to(DEV)
    opt = HipAdam(model.parameters(), lr=1e-2)
    losses = []
    torch.manual_seed(0)
    for _ in range(6):
        opt.zero_grad()
        data["pred"] = model(cd, data["wave"], torch.tensor(TRAIN_LENGTHS))[0]
        loss = loss_fn(data, {"mask": torch.tensor(lens)}, 0)["loss"]
        losses.append(loss.item())
        loss.backward()
        opt.step()
    print("wavenet adam losses", ["{:.4f}".format(v) for v in losses])
    assert losses[5] < losses[0]
    model.eval()
    out, _ = model(cd, None, TRAIN_LENGTHS, generator=torch.Generator(device=DEV))
    assert out.shape == (3, net.C, 70) and model.has_weight_norm
    assert all(k_.rsplit(".", 1)[1] in ("weight_g", "weight_v", "bias") for k_ in model.state_dict())
    # training goes on after generation
    model.train()
    opt.zero_grad()
    data["pred"] = model(cd, data["wave"], torch.tensor(TRAIN_LENGTHS))[0]
    loss_fn(data, {"mask": torch.tensor(lens)}, 0)["loss"].backward()
    opt.step()
