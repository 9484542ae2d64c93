"""Plain-torch restatement of the fixed attention and of both passes of the decoder, for the models of
tests/golden/decoder_fixture.npz (written by tests/golden/make_golden_decoder.py against the reference).  Every
function takes the dtype it computes in: float64 is the reference of the GPU tests (tests/test_encdec_spec.py holds it
to the fixture at 1e-12 relative), float32 on the CPU gives the error a float32 flow has anyway (check)."""
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_fixture.npz")
N_STEP = 5                                   # n_frames_per_step of cases 2 - 4
REL_BOUND, ELEM_BOUND = 2e-6, 2e-5           # the dense layers' bounds (tests/latent_cases.py)


def load_fixture():
    return np.load(FIXTURE)


def sub(fix, prefix):
    """{key without the prefix: array} of the fixture entries under `prefix`"""
    return {k[len(prefix):]: fix[k] for k in fix.files if k.startswith(prefix)}


def tensors(arrays, dtype):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in arrays.items()}


def errors(got, ref):
    d = (got.double().cpu() - ref.double().cpu()).abs()
    rel = d.norm().item() / (ref.double().norm().item() + 1e-30)
    el = d.max().item() / max(1.0, ref.abs().max().item()) if d.numel() else 0.0
    return rel, el


def check(what, got, ref, ref32=None):
    """asserts `got` against the float64 `ref`.  The bound is the larger of the dense layers' (2e-6 relative in the
    2-norm, 2e-5 * max(1, max|ref|) per element) and twice the error of `ref32`, the same flow in torch float32 on the
    CPU.  Prints and returns the larger fraction of tolerance used."""
    rel, el = errors(got, ref)
    rel_tol, el_tol = REL_BOUND, ELEM_BOUND
    if ref32 is not None:
        rel32, el32 = errors(ref32, ref)
        rel_tol, el_tol = max(rel_tol, 2 * rel32), max(el_tol, 2 * el32)
    used = max(rel / rel_tol, el / el_tol)
    print("encdec {}: rel {:.3g} (tol {:.3g}), elem {:.3g} (tol {:.3g}): {:.2f} of tolerance".format(
        what, rel, rel_tol, el, el_tol, used))
    assert rel < rel_tol and el < el_tol, (what, rel, rel_tol, el, el_tol)
    return used


# ---- the attention ---------------------------------------------------------------------------------------------------
def attention(A, enc, n, partial_last=False):
    """A [B, T, P], enc [B, P, C] -> (ctx [B, K, C], Abar [B, K, P]) as a dense product in the dtype of the operands"""
    B, T, P = A.shape
    if not partial_last:
        assert T % n == 0
        abar = A.reshape(B, T // n, n, P).mean(dim=2)
    else:
        abar = torch.stack([A[:, t:t + n].mean(dim=1) for t in range(0, T, n)], dim=1) if T else A.new_zeros(B, 0, P)
    return torch.bmm(abar, enc), abar


def attention_bwd(abar, dctx):
    """d_enc [B, P, C]"""
    return torch.bmm(abar.transpose(1, 2), dctx)


# ---- layers ------------------------------------------------------------------------------------------------------------
def linear(sd, key, x, act=None):
    y = x @ sd[key + ".weight"].T + sd[key + ".bias"]
    return {None: y, "tanh": torch.tanh(y), "relu": torch.relu(y)}[act]


def lstm_step(sd, key, x, h, c):
    """one frame x [B, F] of torch.nn.LSTM's layer 0 (gate order i, f, g, o)"""
    g = x @ sd[key + ".weight_ih_l0"].T + sd[key + ".bias_ih_l0"] + h @ sd[key + ".weight_hh_l0"].T \
        + sd[key + ".bias_hh_l0"]
    i, f, gg, o = g.chunk(4, dim=1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c), c


def lstm(sd, group, x, lens):
    """x [B, T, F] from the group's initial state; frames at or behind a row's length are zero and leave its state"""
    B, T, _ = x.shape
    h = sd[group + ".h_0"][0].expand(B, -1)
    c = sd[group + ".c_0"][0].expand(B, -1)
    ys = []
    for t in range(T):
        h1, c1 = lstm_step(sd, group + ".module", x[:, t], h, c)
        live = (lens > t).to(x.dtype)[:, None]
        h, c = live * h1 + (1 - live) * h, live * c1 + (1 - live) * c
        ys.append(live * h1)
    return torch.stack(ys, dim=1), (h, c)


def encoder(sd, phonemes):
    return linear(sd, "Encoder.model.1.module.0", phonemes, "tanh")


# ---- case 1: attention, then a parallel decoder ---------------------------------------------------------------------
def case1(sd, inputs, frame_lens):
    enc = encoder(sd, inputs["phonemes"])
    ctx, abar = attention(inputs["attention_matrix"], enc, 1)
    hidden = linear(sd, "ParallelDecoder.model.1.module.0", ctx, "relu")
    pred, _ = lstm(sd, "ParallelDecoder.model.2", hidden, frame_lens)
    return {"phoneme_embeddings": enc, "attention": abar, "upsampled_phoneme_embeddings": ctx,
            "pred_acoustic_features": pred}


# ---- cases 2 - 4: the autoregressive decoder ------------------------------------------------------------------------
def pre_net(sd, x):
    return linear(sd, "Decoder.pre_net.1.module.2", linear(sd, "Decoder.pre_net.1.module.0", x, "relu"), "relu")


def project(sd, y, n=N_STEP):
    out = linear(sd, "Decoder.Decoder_AcousticFeaturesProjector.model.1.module.0", y)
    return out.reshape(out.shape[0], out.shape[1] * n, -1)


def decoder_batched(sd, inputs, frame_lens, n=N_STEP):
    enc = encoder(sd, inputs["phonemes"])
    target = inputs["acoustic_features"]
    ctx, abar = attention(inputs["attention_matrix"], enc, n)
    go = target.new_zeros(target.shape[0], 1, target.shape[2])
    fed = torch.cat((go, target[:, n - 1::n][:, :-1]), dim=1)
    x = torch.cat((ctx, pre_net(sd, fed)), dim=2)
    y, _ = lstm(sd, "Decoder.model.2", linear(sd, "Decoder.model.1.module.0", x, "relu"), frame_lens // n)
    return {"phoneme_embeddings": enc, "attention": abar, "pred_acoustic_features": project(sd, y, n)}


def mse(pred, target, mask):
    return (((pred - target) ** 2) * mask).sum() / (mask.sum() * pred.shape[2])


def decoder_iterative(sd, inputs, with_target, p_teacher_forcing=1.0, draws=(), n=N_STEP):
    """the loop of the reference; `draws`: what np.random.uniform returns, in order.  Every row runs every step."""
    enc = encoder(sd, inputs["phonemes"])
    A = inputs["attention_matrix"]
    target = inputs["acoustic_features"] if with_target else None
    B, T = A.shape[:2]
    steps = -(-(target.shape[1] if with_target else T) // n)
    ctx, abar = attention(A, enc, n, partial_last=True)
    h = sd["Decoder.model.2.h_0"][0].expand(B, -1)
    c = sd["Decoder.model.2.c_0"][0].expand(B, -1)
    frame = enc.new_zeros(B, 1, inputs["acoustic_features"].shape[2])
    draws, outs, last = list(draws), [], None
    for i in range(steps):
        if i > 0:
            if with_target and draws.pop(0) <= p_teacher_forcing:
                frame = target[:, i * n - 1:i * n]
            else:
                frame = last[:, -1:]
        x = torch.cat((ctx[:, i:i + 1], pre_net(sd, frame)), dim=-1)
        h, c = lstm_step(sd, "Decoder.model.2.module", linear(sd, "Decoder.model.1.module.0", x, "relu")[:, 0], h, c)
        last = project(sd, h[:, None], n)
        outs.append(last)
    assert not draws
    return {"phoneme_embeddings": enc, "attention": abar[:, :steps], "pred_acoustic_features": torch.cat(outs, dim=1)}
