"""Float64 restatements of multi-head self-attention over a padded batch (csrc/attention.hip) and of a whole
torch.nn.TransformerEncoderLayer block, with closed-form gradients of the core; the cases, bounds and input draws of
tests/test_gpu_attention.py and tests/test_gpu_attention_model.py.  tests/test_attention_spec.py anchors all of it to
torch's own float64 modules and to autograd, without a GPU.

Layout: qkv [B, T, 3 D] (batch-major here; the tests transpose for the time-major layout), q | k | v per row, head h
in columns h dh .. (h + 1) dh of each third.  Query t of utterance b attends keys 0 .. klen[b] - 1 for EVERY t < T.
A keep mask is bool [B, H, T, T]; element (b, h, t, key) is row (b H + h) T + t, column key, of dropout_spec.keep_mask."""
import math

import numpy as np
import torch

import dropout_spec

# the dense layers' bounds (tests/lnorm_cases.py): relative error in the 2-norm, and the largest element error as a
# multiple of max(1, max |ref|)
REL_BOUND = 2e-6
REL_BOUND_REDUCED = 3e-6      # sums over rows: bias gradients, norm weights
ELEM_BOUND = 2e-5
# the only cases that may use twice torch's own float32 error instead (scores near +-60: the rounding of a score of
# 60 is 4e-6 absolute, which the exponential turns into as much relative error of a probability)
HAZARDS = ("spike_last_tile", "spike_first_tile")
# the envelope of the kernel (ops.ATTENTION_*)
MIN_DH, MAX_DH, DH_STEP, MAX_D, MAX_T, MAX_BH = 4, 128, 4, 1024, 32768, 65535


def check_envelope(B, T, H, dh):
    """ValueError naming the value outside the kernel's envelope"""
    if dh % DH_STEP or not MIN_DH <= dh <= MAX_DH:
        raise ValueError("dh = {} is not a multiple of {} in {} .. {}".format(dh, DH_STEP, MIN_DH, MAX_DH))
    if H * dh > MAX_D:
        raise ValueError("D = {} is beyond {}".format(H * dh, MAX_D))
    if not 1 <= T <= MAX_T:
        raise ValueError("T = {} is outside 1 .. {}".format(T, MAX_T))
    if B * H > MAX_BH:
        raise ValueError("B * H = {} is beyond {}".format(B * H, MAX_BH))


def split_heads(qkv, H):
    """q, k, v [B, H, T, dh] (float64) of qkv [B, T, 3 D]"""
    B, T, D3 = qkv.shape
    D = D3 // 3
    parts = qkv.double().reshape(B, T, 3, H, D // H).permute(2, 0, 3, 1, 4)
    return parts[0], parts[1], parts[2]


def key_mask(klen, T):
    """bool [B, 1, 1, T]: True where the key is attended"""
    return (torch.arange(T)[None, :] < torch.as_tensor(klen)[:, None])[:, None, None, :]


def drop_factor(keep, p):
    """float64 [B, H, T, T]: keep mask times the float32 scale 1 / (1 - p) of the kernels, or None"""
    if keep is None:
        return None
    return torch.as_tensor(np.asarray(keep)).double() * float(dropout_spec.scale_f32(p))


def attention_keep_mask(B, H, T, p, seed, salt):
    """the kernel's mask restated in numpy: bool [B, H, T, T]"""
    return dropout_spec.keep_mask(B * H * T, T, p, seed, salt).reshape(B, H, T, T)


def core_forward(qkv, H, klen, keep=None, p=0.0):
    """(o [B, T, D], lse [B, H, T], P [B, H, T, T] before dropout) with explicit scores"""
    B, T, D3 = qkv.shape
    dh = D3 // 3 // H
    check_envelope(B, T, H, dh)
    q, k, v = split_heads(qkv, H)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    s = s.masked_fill(~key_mask(klen, T), -math.inf)
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse[..., None])
    f = drop_factor(keep, p)
    Pd = P if f is None else P * f
    o = (Pd @ v.masked_fill(~key_mask(klen, T).transpose(-1, -2), 0.0)).permute(0, 2, 1, 3).reshape(B, T, D3 // 3)
    return o, lse, P


def core_backward(do, qkv, H, klen, keep=None, p=0.0):
    """dqkv [B, T, 3 D] in closed form: dV = Pd^T dO, dP = m (dO V^T), dS = P (dP - rowsum(dO * O)),
    dQ = dS K / sqrt(dh), dK = dS^T Q / sqrt(dh); rows of dk / dv at and beyond klen are zero"""
    B, T, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    o, _, P = core_forward(qkv, H, klen, keep, p)
    q, k, v = split_heads(qkv, H)
    valid = key_mask(klen, T).transpose(-1, -2)          # [B, 1, T, 1] over key rows
    k, v = k.masked_fill(~valid, 0.0), v.masked_fill(~valid, 0.0)
    f = drop_factor(keep, p)
    dO = do.double().reshape(B, T, H, dh).permute(0, 2, 1, 3)
    O = o.reshape(B, T, H, dh).permute(0, 2, 1, 3)
    Pd = P if f is None else P * f
    dV = Pd.transpose(-1, -2) @ dO
    dP = dO @ v.transpose(-1, -2)
    if f is not None:
        dP = dP * f
    delta = (dO * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dQ = dS @ k / math.sqrt(dh)
    dK = dS.transpose(-1, -2) @ q / math.sqrt(dh)
    parts = [t.permute(0, 2, 1, 3).reshape(B, T, D) for t in (dQ, dK, dV)]
    return torch.cat(parts, dim=2)


def layer_norm(x, w, b, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w + b


def block_forward(x, sd, H, klen, norm_first=False, eps=1e-5, prefix=""):
    """torch.nn.TransformerEncoderLayer (ReLU, no dropout) on x [B, T, D] in float64 from its state dict `sd`
    (keys `<prefix>self_attn.in_proj_weight` ...); differentiable, so autograd gives the block's gradients"""
    g = lambda name: sd[prefix + name].double()        # noqa: E731

    def attention(h):
        qkv = h @ g("self_attn.in_proj_weight").t() + g("self_attn.in_proj_bias")
        q, k, v = split_heads(qkv, H)
        s = (q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
        s = s.masked_fill(~key_mask(klen, h.shape[1]), -math.inf)
        a = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(h.shape)
        return a @ g("self_attn.out_proj.weight").t() + g("self_attn.out_proj.bias")

    def feed_forward(h):
        h = torch.relu(h @ g("linear1.weight").t() + g("linear1.bias"))
        return h @ g("linear2.weight").t() + g("linear2.bias")

    def norm(i, h):
        return layer_norm(h, g("norm{}.weight".format(i)), g("norm{}.bias".format(i)), eps)

    x = x.double()
    if norm_first:
        x = x + attention(norm(1, x))
        return x + feed_forward(norm(2, x))
    x = norm(1, x + attention(x))
    return norm(2, x + feed_forward(x))


def errors(got, ref):
    """(relative error in the 2-norm, largest element error over max(1, max|ref|)) against a float64 reference"""
    d = (got.double().cpu() - ref).abs()
    return d.norm().item() / (ref.norm().item() + 1e-30), d.max().item() / max(1.0, ref.abs().max().item())


def check(product, got, ref, case=None, torch32=None, reduced=False):
    """asserts `got` against the float64 `ref` at the dense layers' bounds; a HAZARDS case passes its name and torch's
    own float32 result on the same data, and the bound becomes the larger of the dense one and twice torch's error
    (the pattern of lnorm_cases.check).  Prints and returns the errors."""
    tol_rel, tol_el = (REL_BOUND_REDUCED if reduced else REL_BOUND), ELEM_BOUND
    if torch32 is not None:
        assert case in HAZARDS, "only the named hazards may use the relaxed bound"
        r32, e32 = errors(torch32, ref)
        tol_rel, tol_el = max(tol_rel, 2 * r32), max(tol_el, 2 * e32)
    rel, el = errors(got, ref)
    print("attention {} {}: rel {:.3g} ({:.2f} of tol), elem {:.3g} ({:.2f} of tol)".format(
        case or tuple(ref.shape), product, rel, rel / tol_rel, el, el / tol_el))
    assert rel < tol_rel and el < tol_el, (product, case, rel, tol_rel, el, tol_el)
    return rel, el


def check_dqkv(got, ref, D, **kw):
    for i, name in enumerate(("dq", "dk", "dv")):
        check(name, got[..., i * D:(i + 1) * D], ref[..., i * D:(i + 1) * D], **kw)


# ---- the model cases of tests/golden/attention_fixture.npz (written by tests/golden/make_golden_attention.py against
# the reference, read by tests/test_gpu_attention_model.py) ------------------------------------------------------------
# Linear(16, Tanh) -> TransformerEncoderLayer x 2 (d_model 16, nhead 2, dim_feedforward 32) -> Linear(5) on 6 inputs
MODEL_IN, MODEL_D, MODEL_H, MODEL_F, MODEL_OUT = 6, 16, 2, 32, 5
MODEL_LENS = (7, 4, 1)
MODEL_CASES = [("bf", True, False, 61), ("tm", False, False, 62), ("bf_norm_first", True, True, 63)]   # name, batch_first, norm_first, seed


def model_config(Config, batch_first, norm_first=False, **extra):
    """the rnn_dyn Config of a model case (the reference's package or this one: same names); `extra` goes into the
    attention group's kwargs (this package's mask_padding / layer_dropout)"""
    kwargs = dict(d_model=MODEL_D, nhead=MODEL_H, dim_feedforward=MODEL_F, batch_first=batch_first)
    if norm_first:
        kwargs["norm_first"] = True
    kwargs.update(extra)
    LC = Config.LayerConfig
    return Config(in_dim=MODEL_IN, batch_first=batch_first, layer_configs=[
        LC("Linear", out_dim=MODEL_D, nonlin="Tanh"), LC("TransformerEncoderLayer", num_layers=2, **kwargs),
        LC("Linear", out_dim=MODEL_OUT)])


def model_inputs(seed, batch_first, lens=MODEL_LENS):
    """(x zero-padded, w) float32 in the model's layout: the loss of a case is sum(y * w) over EVERY position"""
    g = torch.Generator().manual_seed(700 + seed)
    B, T = len(lens), max(lens)
    x = torch.randn(B, T, MODEL_IN, generator=g)
    for b, n in enumerate(lens):
        x[b, n:] = 0
    w = torch.randn(B, T, MODEL_OUT, generator=g)
    return (x, w) if batch_first else (x.transpose(0, 1).contiguous(), w.transpose(0, 1).contiguous())


# ---- the cases of tests/test_gpu_attention.py -------------------------------------------------------------------------
TILE = 32          # AT_TILE: keys per tile
BLOCK = 128        # AT_BLOCK: queries (keys) per workgroup
SWEEP_T = (1, 2, 31, 32, 33, 63, 64, 65, 129, 200)
SWEEP_DH = (16, 48, 64, 128)
SWEEP_DH_NARROW = (4, 8, 24, 100)     # head widths that are no multiple of 16 (the fixture's model has 8)
SWEEP_H = (1, 3)
SWEEP_B = (1, 3, 17)


def ragged_klen(B, T, seed=0):
    """lengths that include 1, T and every tile / workgroup edge +- 1 that fits, then seeded draws"""
    edges = [T, 1] + [e + d for e in (TILE, 2 * TILE, BLOCK) for d in (-1, 0, 1)]
    edges = [e for e in edges if 1 <= e <= T]
    rng = np.random.RandomState(100 + seed + 7 * T + B)
    klen = [edges[i] if i < len(edges) else int(rng.randint(1, T + 1)) for i in range(B)]
    return klen


def sweep_cases():
    """(B, T, H, dh, batch_first): every T with a rotating choice of the other axes, then every value of every other
    axis at T = 65 and T = 200, both layouts throughout"""
    cases = []
    for i, T in enumerate(SWEEP_T):
        cases.append((SWEEP_B[i % 3], T, SWEEP_H[i % 2], SWEEP_DH[i % 4], i % 2 == 0))
    for T in (65, 200):
        for dh in SWEEP_DH:
            for bf in (True, False):
                cases.append((3, T, 3 if dh < 128 else 1, dh, bf))
        for B in SWEEP_B:
            cases.append((B, T, 3, 16, B != 3))
    for i, dh in enumerate(SWEEP_DH_NARROW):
        cases.append((3, 65, 2 + i % 2, dh, i % 2 == 0))
    return sorted(set(cases))


def draw_qkv(B, T, H, dh, seed=0, scale=1.0):
    """(qkv [B, T, 3 D], do [B, T, D]) float32 from a seeded CPU generator; q and k of unit variance per element give
    scores of unit variance"""
    g = torch.Generator().manual_seed(9000 + 131 * seed + 17 * T + 3 * B + H + dh)
    return torch.randn(B, T, 3 * H * dh, generator=g) * scale, torch.randn(B, T, H * dh, generator=g)


def hazard_inputs(name, T=200, H=1, dh=64):
    """One key row spiked against one query row so that this query's row maximum (a score near +60) sits in the last
    key tile, or in the first; the opposite key gives a score near -60 against the same query."""
    qkv, do = draw_qkv(2, T, H, dh, seed=40 + HAZARDS.index(name))
    D = H * dh
    key = T - 3 if name == "spike_last_tile" else 2
    other = 5 if name == "spike_last_tile" else T - 7
    for b in range(2):
        qrow = 70
        q = qkv[b, qrow, :dh]
        unit = q / q.norm()
        target = 60.0 * math.sqrt(dh) / q.norm()
        qkv[b, key, D:D + dh] = unit * target
        qkv[b, other, D:D + dh] = -unit * target
    return qkv, do


def torch32_core(qkv, do, H, klen):
    """torch's own float32 attention (explicit softmax) and autograd on the CPU: (o, dqkv)"""
    B, T, D3 = qkv.shape
    D = D3 // 3
    leaf = qkv.clone().requires_grad_(True)
    parts = leaf.reshape(B, T, 3, H, D // H).permute(2, 0, 3, 1, 4)
    s = (parts[0] @ parts[1].transpose(-1, -2)) / math.sqrt(D // H)
    s = s.masked_fill(~key_mask(klen, T), -math.inf)
    o = (torch.softmax(s, dim=-1) @ parts[2]).permute(0, 2, 1, 3).reshape(B, T, D)
    o.backward(do)
    return o.detach(), leaf.grad
