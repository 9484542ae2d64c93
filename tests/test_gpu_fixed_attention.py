"""csrc/fixed_attention.hip through ops against the float64 restatement of tests/encdec_spec.py at the dense layers'
bounds (2e-6 relative in the 2-norm, 2e-5 * max(1, max|ref|) per element): hard matrices of ragged utterances with
all-zero padding rows, soft matrices, a zero row in the middle, a partial last chunk, K = 1, P on both sides of the
tile of 256 per wave's lane quads (1, 13, 67, 130 with a non-zero at p = 129), C on both sides of the channel tile (12,
67, 256, 260, 516), n 1 / 2 / 5; exact selection for n = 1; pitches and bases off the 16-byte grid inside NaN frames;
identical bits alone and inside a batch; the autograd node; every refusal by name."""
import pytest
import torch

import encdec_spec as spec
from idiaptts_amd import lib, ops
from idiaptts_amd.nn import functional as F

pytestmark = pytest.mark.gpu

# (B, T, P, C, n, soft, partial_last)
CASES = [
    (1, 1, 1, 12, 1, False, False),        # K = 1, P = 1
    (3, 20, 13, 67, 1, False, False),
    (3, 20, 13, 67, 2, False, False),
    (3, 20, 67, 256, 5, False, False),
    (3, 22, 67, 260, 5, False, True),      # 22 = 4 * 5 + 2: the last chunk has two rows
    (3, 24, 130, 516, 2, False, False),    # phoneme 129 is attended
    (1, 5, 130, 12, 5, False, False),      # K = 1 with n = 5
    (3, 21, 13, 260, 2, True, True),
    (3, 20, 67, 67, 5, True, False),
    (1, 7, 130, 516, 1, True, False),
]
IDS = ["B{}T{}P{}C{}n{}{}{}".format(b, t, p, c, n, "soft" if s else "hard", "part" if pl else "")
       for b, t, p, c, n, s, pl in CASES]


def make_inputs(B, T, P, C, soft, seed=0):
    """A [B, T, P]: utterance 0 has T frames and P phonemes (its last frame attends phoneme P - 1), the others fewer
    of both; rows behind an utterance's frames and columns behind its phonemes are zero; utterance 0 has an all-zero
    row in the middle when it has more than two frames.  enc [B, P, C], dctx weights come from the caller."""
    g = torch.Generator().manual_seed(1000 * B + 100 * T + 10 * P + C + seed)
    A = torch.zeros(B, T, P)
    for b in range(B):
        frames = T if b == 0 else max(1, T - 3 * b - 1)
        phonemes = P if b == 0 else max(1, P - 2 * b)
        if soft:
            A[b, :frames, :phonemes] = torch.rand(frames, phonemes, generator=g) + 0.05
            A[b, :frames] /= A[b, :frames].sum(dim=1, keepdim=True)
        else:
            idx = torch.randint(0, phonemes, (frames,), generator=g).sort().values
            if b == 0:
                idx[-1] = phonemes - 1
            A[b, torch.arange(frames), idx] = 1.0
        if b == 0 and frames > 2:
            A[b, frames // 2] = 0.0
    enc = torch.randn(B, P, C, generator=g) + 0.3
    return A, enc, g


def check(what, got, ref):
    return spec.check(what, got, ref)


@pytest.mark.parametrize("B,T,P,C,n,soft,partial", CASES, ids=IDS)
def test_forward_and_backward_against_float64(gpu, B, T, P, C, n, soft, partial):
    A, enc, g = make_inputs(B, T, P, C, soft)
    ctx64, abar64 = spec.attention(A.double(), enc.double(), n, partial)
    K = ctx64.shape[1]
    plan = ops.fixed_attention_plan(B, T, P, C, n, partial)
    assert plan["K"] == K and plan["fwd_grid"] == B * -(-K // 4) and plan["fwd_lds_bytes"] == 4 * P * 8
    assert plan["bwd_grid"] == (B * -(-P // 16), -(-C // 256))
    assert (plan["vec_p"], plan["vec_c"]) == (P % 4 == 0, C % 4 == 0)
    Ad, ed = A.to(gpu), enc.to(gpu)
    ctx = torch.full((B, K, C), float("nan"), device=gpu)
    abar = torch.full((B, K, P), float("nan"), device=gpu)
    ops.fixed_attention(Ad, ed, n, partial, abar=abar, ctx=ctx)
    check("abar", abar, abar64)
    check("ctx", ctx, ctx64)
    zero_rows = (abar64.abs().sum(dim=2) == 0)
    assert zero_rows.any() or B == 1                       # the padded frames (and the zero row with n = 1)
    assert (ctx.cpu()[zero_rows] == 0).all()               # .. give zero context rows
    ctx2, abar2 = ops.fixed_attention(Ad, ed, n, partial)  # identical bits on a second call
    assert torch.equal(ctx, ctx2) and torch.equal(abar, abar2)
    dctx = torch.randn(B, K, C, generator=g)
    denc = torch.full((B, P, C), float("nan"), device=gpu)          # every position must be written
    ops.fixed_attention_bwd(abar, dctx.to(gpu), out=denc)
    check("d_enc", denc, spec.attention_bwd(abar64, dctx.double()))
    assert torch.equal(denc, ops.fixed_attention_bwd(abar, dctx.to(gpu)))
    # the autograd node: the gradient of enc is that kernel's, A gets none, "attention" is not differentiable
    e = ed.clone().requires_grad_(True)
    c, a = F.fixed_attention(Ad, e, n, partial)
    assert torch.equal(c, ctx) and torch.equal(a, abar) and not a.requires_grad
    (c * dctx.to(gpu)).sum().backward()
    assert torch.equal(e.grad, denc)


@pytest.mark.parametrize("B,T,P,C", [(3, 20, 13, 67), (3, 24, 130, 516), (1, 9, 67, 260)])
def test_hard_attention_with_one_frame_per_step_selects_rows_exactly(gpu, B, T, P, C):
    A, enc, _ = make_inputs(B, T, P, C, soft=False, seed=2)
    ctx, abar = ops.fixed_attention(A.to(gpu), enc.to(gpu), 1)
    assert torch.equal(abar.cpu(), A)
    expect = torch.zeros(B, T, C)
    live = A.sum(dim=2) > 0
    expect[live] = enc[torch.nonzero(live)[:, 0], A.argmax(dim=2)[live]]
    assert torch.equal(ctx.cpu(), expect)                  # one term of weight 1.0: bit for bit
    if P == 130:
        assert A[0, -1, 129] == 1.0 and torch.equal(ctx[0, -1].cpu(), enc[0, 129])


def _framed(shape, pitch, base, gpu, fill=None):
    """a [B, R, W] view with row pitch `pitch` starting `base` floats into a NaN-filled buffer, 5 floats behind its
    last row still inside; -> (buffer, view, mask of the view's own floats)"""
    B, R, W = shape
    utt = R * pitch + 3
    size = base + B * utt + 5
    buf = torch.full((size,), float("nan"), device=gpu)
    view = buf.as_strided(shape, (utt, pitch, 1), base)
    own = torch.zeros(size, dtype=torch.bool, device=gpu)
    own.as_strided(shape, (utt, pitch, 1), base).fill_(True)
    if fill is not None:
        view.copy_(fill)
    return buf, view, own


@pytest.mark.parametrize("base,extra", [(0, 0), (1, 1), (3, 2), (4, 4), (2, 3)])
def test_pitches_and_bases_off_the_16_byte_grid_inside_nan_frames(gpu, base, extra):
    """widths 68 / 260 (16-byte accesses when pitch, utterance step and base allow: base 4, extra 4 is the one framed
    case that does) and every other combination on plain accesses: the same bits as the dense call, and not one float
    outside the views is touched"""
    B, T, P, C, n = 3, 21, 68, 260, 2
    A, enc, g = make_inputs(B, T, P, C, soft=True, seed=3)
    dctx = torch.randn(B, 11, C, generator=g)
    ref_ctx, ref_abar = ops.fixed_attention(A.to(gpu), enc.to(gpu), n, True)
    ref_denc = ops.fixed_attention_bwd(ref_abar, dctx.to(gpu))
    _, Av, _ = _framed((B, T, P), P + extra, base, gpu, A.to(gpu))
    _, ev, _ = _framed((B, P, C), C + extra, base, gpu, enc.to(gpu))
    abuf, av, aown = _framed((B, 11, P), P + extra, base, gpu)
    cbuf, cv, cown = _framed((B, 11, C), C + extra, base, gpu)
    ops.fixed_attention(Av, ev, n, True, abar=av, ctx=cv)
    assert torch.equal(av, ref_abar) and torch.equal(cv, ref_ctx)
    assert torch.isnan(abuf[~aown]).all() and torch.isnan(cbuf[~cown]).all()
    _, dv, _ = _framed((B, 11, C), C + extra, base, gpu, dctx.to(gpu))
    dbuf, dev_, down = _framed((B, P, C), C + extra, base, gpu)
    ops.fixed_attention_bwd(av, dv, out=dev_)
    assert torch.equal(dev_, ref_denc)
    assert torch.isnan(dbuf[~down]).all()


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_an_utterance_does_not_depend_on_its_batch(gpu, soft):
    T, P, C, n = 23, 67, 260, 5
    A, enc, g = make_inputs(3, T, P, C, soft, seed=4)
    A[2], enc[2] = A[0], enc[0]                 # utterance 0 again, at index 2 of 3
    dctx = torch.randn(3, 5, C, generator=g)
    dctx[2] = dctx[0]
    ctx3, abar3 = ops.fixed_attention(A.to(gpu), enc.to(gpu), n, True)
    ctx1, abar1 = ops.fixed_attention(A[:1].to(gpu), enc[:1].to(gpu), n, True)
    assert torch.equal(ctx3[2], ctx1[0]) and torch.equal(abar3[2], abar1[0]) and torch.equal(ctx3[0], ctx3[2])
    d3 = ops.fixed_attention_bwd(abar3, dctx.to(gpu))
    d1 = ops.fixed_attention_bwd(abar1, dctx[:1].to(gpu))
    assert torch.equal(d3[2], d1[0])


def test_inf_and_nan_at_a_zero_weight_do_not_reach_the_context(gpu):
    """the one place where skipping zeros differs from bmm"""
    A, enc, _ = make_inputs(1, 6, 5, 12, soft=False, seed=5)
    unattended = [p for p in range(5) if A[0, :, p].sum() == 0]
    if not unattended:
        A[0, :, 4] = 0.0
        unattended = [4]
    enc[0, unattended[0], 0], enc[0, unattended[0], 1] = float("inf"), float("nan")
    ctx, _ = ops.fixed_attention(A.to(gpu), enc.to(gpu), 2)
    assert torch.isfinite(ctx).all()
    assert not torch.isfinite(torch.bmm(A.reshape(1, 3, 2, 5).mean(2), enc)).all()


def test_refusals_by_name(gpu):
    def call(B=1, T=4, P=4, C=4, n=1, partial=False):
        return ops.fixed_attention(torch.zeros(B, T, P, device=gpu), torch.zeros(B, P, C, device=gpu), n, partial)
    with pytest.raises(lib.IttsError, match=r"P = 2049 is outside 1 \.\. 2048"):
        call(P=2049)
    with pytest.raises(lib.IttsError, match=r"C = 4097 is outside 1 \.\. 4096"):
        call(C=4097)
    with pytest.raises(ValueError, match=r"n_frames_per_step = 65 is outside 1 \.\. 64"):
        call(T=65, n=65)
    with pytest.raises(ValueError, match="T = 7 is not a multiple of n_frames_per_step = 2"):
        call(T=7, n=2)
    assert call(T=7, n=2, partial=True)[0].shape == (1, 4, 4)
    assert call(P=2048, C=4, T=2)[0].shape == (1, 2, 4) and call(C=4096, T=2)[0].shape == (1, 2, 4096)
    with pytest.raises(lib.IttsError, match=r"P = 2049"):
        ops.fixed_attention_bwd(torch.zeros(1, 2, 2049, device=gpu), torch.zeros(1, 2, 4, device=gpu))
    for bad in (dict(P=2049), dict(C=4097), dict(n=65), dict(T=7, n=2)):
        with pytest.raises(ValueError, match="no fixed-attention plan"):
            ops.fixed_attention_plan(**{**dict(B=1, T=4, P=4, C=4, n=1), **bad})
    A = torch.zeros(1, 4, 4, device=gpu, requires_grad=True)
    for fn in (ops.fixed_attention, F.fixed_attention):
        with pytest.raises(ValueError, match="A.requires_grad"):
            fn(A, torch.zeros(1, 4, 4, device=gpu), 1)
    with pytest.raises(lib.IttsError, match="must live on the GPU"):
        ops.fixed_attention(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), 1)
    with pytest.raises(ValueError, match=r"enc must be \[B, P, C\]"):
        ops.fixed_attention(torch.zeros(1, 4, 4, device=gpu), torch.zeros(1, 5, 4, device=gpu), 1)
