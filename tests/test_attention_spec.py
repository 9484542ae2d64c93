"""tests/attention_spec.py against torch's own float64 modules and autograd (no GPU): the block restatement equals
torch.nn.TransformerEncoderLayer under src_key_padding_mask to 1e-12 for both norm orders, the closed-form gradients
of the core equal autograd with and without a keep mask, the mask is dropout_spec.keep_mask's, masked keys carry
nothing (NaN in their rows changes no output), and a shape outside the kernel's envelope is refused by name."""
import numpy as np
import pytest
import torch

import attention_spec as spec
import dropout_spec


def _block(D, H, F, norm_first, seed):
    torch.manual_seed(seed)
    block = torch.nn.TransformerEncoderLayer(d_model=D, nhead=H, dim_feedforward=F, dropout=0.0, batch_first=True,
                                             norm_first=norm_first).double()
    with torch.no_grad():               # (biases and norms away from their zeros and ones)
        for prm in block.parameters():
            if prm.dim() == 1:
                prm.add_(0.3 * torch.randn_like(prm))
    return block.train()


@pytest.mark.parametrize("norm_first", [False, True])
def test_block_equals_torch_float64(norm_first):
    D, H, F, lens = 32, 2, 48, [9, 5, 1]
    block = _block(D, H, F, norm_first, 3)
    B, T = len(lens), max(lens)
    x = torch.randn(B, T, D, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    pad = ~(torch.arange(T)[None, :] < torch.tensor(lens)[:, None])
    x1 = x.clone().requires_grad_(True)
    y_ref = block(x1, src_key_padding_mask=pad)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in block.state_dict().items()}
    x2 = x.clone().requires_grad_(True)
    y = spec.block_forward(x2, sd, H, lens, norm_first=norm_first)
    assert (y - y_ref).abs().max().item() < 1e-12           # every position, padded queries included
    w = torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    (y_ref * w).sum().backward()
    (y * w).sum().backward()
    assert (x1.grad - x2.grad).abs().max().item() < 1e-12
    for k, prm in block.named_parameters():
        assert (prm.grad - sd[k].grad).abs().max().item() < 1e-12, k
    # no mask: every padded position is a key
    y_all = spec.block_forward(x, sd, H, [T] * B, norm_first=norm_first)
    assert (y_all - block(x)).abs().max().item() < 1e-12
    assert (y_all - y).abs().max().item() > 1e-3


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_core_gradients_equal_autograd(p):
    B, T, H, dh = 3, 37, 2, 16
    klen = [37, 1, 20]
    qkv, do = spec.draw_qkv(B, T, H, dh, seed=1)
    keep = spec.attention_keep_mask(B, H, T, p, seed=1234, salt=3) if p > 0 else None
    if keep is not None:
        assert abs(keep.mean() - (1 - p)) < 0.02
        flat = dropout_spec.keep_mask(B * H * T, T, p, 1234, 3)
        assert np.array_equal(keep[1, 1, 5], flat[(1 * H + 1) * T + 5])
    leaf = qkv.double().requires_grad_(True)
    o, lse, P = spec.core_forward(leaf, H, klen, keep, p)
    assert torch.allclose(P.sum(-1), torch.ones(B, H, T, dtype=torch.float64), atol=1e-13)
    assert (P[1, :, :, 1:] == 0).all() and (P[2, :, :, 20:] == 0).all()
    o.backward(do.double())
    dqkv = spec.core_backward(do, qkv, H, klen, keep, p)
    assert (dqkv - leaf.grad).abs().max().item() < 1e-12
    D = H * dh
    assert (dqkv[1, 1:, D:] == 0).all() and (dqkv[2, 20:, D:] == 0).all()       # dk, dv of masked keys
    assert dqkv[2, 20:, :D].abs().max() > 1e-3                                  # dq of padded queries is computed
    if p == 0:
        o32, dqkv32 = spec.torch32_core(qkv, do, H, klen)
        spec.check("o", o32, o.detach())
        spec.check_dqkv(dqkv32, dqkv, D)


def test_masked_keys_carry_nothing():
    B, T, H, dh = 2, 40, 1, 16
    klen = [33, 7]
    qkv, do = spec.draw_qkv(B, T, H, dh, seed=2)
    o, lse, _ = spec.core_forward(qkv, H, klen)
    dqkv = spec.core_backward(do, qkv, H, klen)
    bad = qkv.clone()
    for b, n in enumerate(klen):
        bad[b, n:, H * dh:] = float("nan")
    o2, lse2, _ = spec.core_forward(bad, H, klen)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    assert torch.equal(dqkv, spec.core_backward(do, bad, H, klen))


@pytest.mark.parametrize("shape,needle", [
    ((1, 4, 1, 6), "dh = 6"), ((1, 4, 1, 136), "dh = 136"), ((1, 4, 1, 2), "dh = 2"), ((1, 4, 65, 16), "D = 1040"),
    ((1, 0, 1, 16), "T = 0"), ((1, 32769, 1, 16), "T = 32769"), ((65536, 4, 1, 16), "B * H = 65536"),
])
def test_envelope_is_refused_by_name(shape, needle):
    with pytest.raises(ValueError, match=needle.replace("*", r"\*")):
        spec.check_envelope(*shape)
    B, T, H, dh = shape
    if 0 < B * T * H * dh < 1 << 16:            # the restatement itself refuses it
        with pytest.raises(ValueError, match=needle.replace("*", r"\*")):
            spec.core_forward(torch.zeros(B, T, 3 * H * dh), H, [T] * B)


def test_sweep_covers_the_axes():
    cases = spec.sweep_cases()
    assert {c[1] for c in cases} == set(spec.SWEEP_T)
    assert {c[3] for c in cases} == set(spec.SWEEP_DH) | set(spec.SWEEP_DH_NARROW)
    assert {c[2] for c in cases} >= set(spec.SWEEP_H) and {c[0] for c in cases} == set(spec.SWEEP_B)
    assert {c[4] for c in cases} == {True, False}
    klen = spec.ragged_klen(17, 200)
    for edge in (1, 200, 31, 32, 33, 63, 64, 65, 127, 128, 129):
        assert edge in klen
    assert all(1 <= n <= 200 for n in klen)
    for name in spec.HAZARDS:
        qkv, _ = spec.hazard_inputs(name)
        _, _, P = spec.core_forward(qkv, 1, [200, 200])
        s = (qkv[0, 70, :64].double() @ qkv[0, :, 64:128].double().t()) / 8.0
        assert 59 < s.max() < 61 and -61 < s.min() < -59
        assert int(s.argmax()) // spec.TILE == (6 if name == "spike_last_tile" else 0)
