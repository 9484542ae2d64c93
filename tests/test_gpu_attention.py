"""The attention kernels of csrc/attention.hip on the GPU against the float64 restatement of tests/attention_spec.py:
the shape sweep in both layouts (forward, log-sum-exp and all three gradients), the two hazards of the running
maximum, independence of whatever lies in masked key rows, bit-identity of an utterance alone and inside a batch,
run-to-run reproducibility, dropout against the numpy mask, sentinel frames around every output, and the memory the
calls take."""
import ctypes

import pytest
import torch

import attention_spec as spec
from idiaptts_amd import lib, ops

pytestmark = pytest.mark.gpu


def to_layout(t, batch_first):
    """a batch-major CPU tensor in the layout the kernel is called with, on the GPU"""
    return (t if batch_first else t.transpose(0, 1)).contiguous().cuda()


def from_layout(t, batch_first):
    return (t if batch_first else t.transpose(0, 1)).cpu()


def run(qkv, do, H, klen, batch_first=True, p=0.0, seed=0, salt=0):
    """(o, lse, dqkv) on the GPU for batch-major CPU operands, returned batch-major on the CPU"""
    q = to_layout(qkv, batch_first)
    kl = None if klen is None else torch.tensor(klen, dtype=torch.int32, device="cuda")
    o, lse = ops.attention_forward(q, H, kl, batch_first, p, seed, salt)
    dqkv = ops.attention_backward(to_layout(do, batch_first), q, o, lse, H, kl, batch_first, p, seed, salt)
    return from_layout(o, batch_first), lse.cpu(), from_layout(dqkv, batch_first)


@pytest.mark.parametrize("B,T,H,dh,batch_first", spec.sweep_cases())
def test_sweep(gpu, B, T, H, dh, batch_first):
    klen = spec.ragged_klen(B, T)
    qkv, do = spec.draw_qkv(B, T, H, dh)
    o, lse, dqkv = run(qkv, do, H, klen, batch_first)
    ref_o, ref_lse, _ = spec.core_forward(qkv, H, klen)
    spec.check("o", o, ref_o)
    spec.check("lse", lse, ref_lse)
    spec.check_dqkv(dqkv, spec.core_backward(do, qkv, H, klen), H * dh)
    if T == 65 and dh == 16 and B == 3:
        # no lengths: every position is a key
        o_all, _, dqkv_all = run(qkv, do, H, None, batch_first)
        spec.check("o", o_all, spec.core_forward(qkv, H, [T] * B)[0])
        spec.check_dqkv(dqkv_all, spec.core_backward(do, qkv, H, [T] * B), H * dh)


@pytest.mark.parametrize("name", spec.HAZARDS)
def test_running_maximum_hazards(gpu, name):
    """a query whose row maximum (a score near +60, next to one near -60) sits in the last key tile, so that every
    earlier tile is rescaled by almost nothing, and in the first, so that every later tile adds almost nothing"""
    qkv, do = spec.hazard_inputs(name)
    klen = [qkv.shape[1]] * 2
    o, lse, dqkv = run(qkv, do, 1, klen)
    o32, dqkv32 = spec.torch32_core(qkv, do, 1, klen)
    ref_o, ref_lse, _ = spec.core_forward(qkv, 1, klen)
    spec.check("o", o, ref_o, case=name, torch32=o32)
    spec.check("lse", lse, ref_lse)
    ref = spec.core_backward(do, qkv, 1, klen)
    D = 64
    for i, product in enumerate(("dq", "dk", "dv")):
        sl = slice(i * D, (i + 1) * D)
        spec.check(product, dqkv[..., sl], ref[..., sl], case=name, torch32=dqkv32[..., sl])


@pytest.mark.parametrize("batch_first", [True, False])
def test_masked_rows_are_never_used(gpu, batch_first):
    B, T, H, dh = 3, 70, 2, 48
    klen = [33, 70, 1]
    qkv, do = spec.draw_qkv(B, T, H, dh, seed=3)
    clean = run(qkv, do, H, klen, batch_first)
    bad = qkv.clone()
    for b, n in enumerate(klen):
        bad[b, n:, H * dh:] = float("nan")
    got = run(bad, do, H, klen, batch_first)
    for a, b in zip(clean, got):
        assert torch.equal(a, b)
        assert torch.isfinite(b).all()
    D = H * dh
    assert not got[2][0, 33:, D:].any() and not got[2][2, 1:, D:].any()        # dk, dv of masked keys: zeros
    assert got[2][0, 33:, :D].abs().max() > 0                                  # dq of padded queries: computed


@pytest.mark.parametrize("n,dh", [(77, 64), (129, 16), (32, 128)])
def test_utterance_alone_and_as_row_16_of_17(gpu, n, dh):
    B, T, H = 17, 200, 2
    klen = spec.ragged_klen(B, T)
    klen[16] = n
    qkv, do = spec.draw_qkv(B, T, H, dh, seed=4)
    do[16, n:] = 0              # (alone, the padded queries do not exist: their gradient must add nothing)
    o, lse, dqkv = run(qkv, do, H, klen)
    o1, lse1, dqkv1 = run(qkv[16:, :n].contiguous(), do[16:, :n].contiguous(), H, [n])
    assert torch.equal(o[16, :n], o1[0]) and torch.equal(lse[16, :, :n], lse1[0])
    assert torch.equal(dqkv[16, :n], dqkv1[0])
    # and in the other layout, at another position
    o2, lse2, dqkv2 = run(qkv[14:], do[14:], H, klen[14:], batch_first=False)
    assert torch.equal(o2[2, :n], o1[0]) and torch.equal(dqkv2[2, :n], dqkv1[0])


def test_two_runs_give_identical_bits(gpu):
    B, T, H, dh = 5, 200, 3, 48
    klen = spec.ragged_klen(B, T)
    qkv, do = spec.draw_qkv(B, T, H, dh, seed=5)
    first = run(qkv, do, H, klen, p=0.1, seed=77, salt=2)
    second = run(qkv, do, H, klen, p=0.1, seed=77, salt=2)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    third = run(qkv, do, H, klen, p=0.1, seed=78, salt=2)
    assert not torch.equal(first[0], third[0])


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("batch_first", [True, False])
def test_dropout_equals_the_spec_with_the_numpy_mask(gpu, p, batch_first):
    B, T, H, dh = 3, 70, 2, 16
    klen = [70, 33, 1]
    seed, salt = 0x1234567887654321, 5
    qkv, do = spec.draw_qkv(B, T, H, dh, seed=6)
    keep = spec.attention_keep_mask(B, H, T, p, seed, salt)
    o, lse, dqkv = run(qkv, do, H, klen, batch_first, p, seed, salt)
    ref_o, ref_lse, _ = spec.core_forward(qkv, H, klen, keep, p)
    spec.check("o", o, ref_o)
    spec.check("lse", lse, ref_lse)             # (the log-sum-exp is that of the probabilities before dropout)
    spec.check_dqkv(dqkv, spec.core_backward(do, qkv, H, klen, keep, p), H * dh)
    # the mask matters: the undropped result is far away
    assert (o - spec.core_forward(qkv, H, klen)[0]).abs().max() > 1e-2


def test_p_zero_is_the_path_without_dropout(gpu):
    B, T, H, dh = 2, 65, 1, 64
    klen = [65, 40]
    qkv, do = spec.draw_qkv(B, T, H, dh, seed=7)
    plain = run(qkv, do, H, klen)
    zero = run(qkv, do, H, klen, p=0.0, seed=99, salt=9)
    for a, b in zip(plain, zero):
        assert torch.equal(a, b)


@pytest.mark.parametrize("batch_first", [True, False])
def test_sentinel_frames_stay_intact(gpu, batch_first):
    """every output buffer framed by NaN on both sides, through the C entry points"""
    L = lib.load()
    B, T, H, dh, F = 3, 45, 2, 16, 64
    D = H * dh
    klen = torch.tensor([45, 20, 1], dtype=torch.int32, device="cuda")
    qkv, do = spec.draw_qkv(B, T, H, dh, seed=8)
    qkv, do = to_layout(qkv, batch_first), to_layout(do, batch_first)
    sb, st = (T, 1) if batch_first else (1, B)

    def framed(n):
        buf = torch.full((n + 2 * F,), float("nan"), dtype=torch.float32, device="cuda")
        return buf, buf[F:F + n]

    def intact(buf, n):
        return bool(torch.isnan(buf[:F]).all() and torch.isnan(buf[F + n:]).all() and torch.isfinite(buf[F:F + n]).all())

    ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_o, n_lse, n_dqkv = B * T * D, B * H * T, B * T * 3 * D
    (bo, o), (bl, lse), (bd, dqkv) = framed(n_o), framed(n_lse), framed(n_dqkv)
    for p in (0.0, 0.25):
        lib.check(L.itts_attention_fwd(ptr(qkv), ptr(o), ptr(klen), ptr(lse), B, T, H, dh, sb, st, p, 5, 1, stream),
                  "itts_attention_fwd")
        lib.check(L.itts_attention_bwd(ptr(do), ptr(qkv), ptr(o), ptr(klen), ptr(lse), ptr(dqkv), B, T, H, dh, sb, st,
                                       p, 5, 1, stream), "itts_attention_bwd")
        torch.cuda.synchronize()
        assert intact(bo, n_o) and intact(bl, n_lse) and intact(bd, n_dqkv)
    got, _ = ops.attention_forward(qkv, H, klen, batch_first, 0.25, 5, 1)
    assert torch.equal(got.reshape(-1), o)


def test_memory_stays_far_below_a_score_tensor(gpu):
    """B 2, H 4, T 4096, dh 64: a [B, H, T, T] float32 tensor would take 537 MB; forward and backward together may
    grow the allocation by less than a quarter of it (torch's allocator and the library's own scratch)"""
    B, T, H, dh = 2, 4096, 4, 64
    scores = B * H * T * T * 4
    assert scores == 536870912
    g = torch.Generator(device="cuda").manual_seed(1)
    qkv = torch.randn(B, T, 3 * H * dh, device="cuda", generator=g)
    do = torch.randn(B, T, H * dh, device="cuda", generator=g)
    klen = torch.tensor([T, 3000], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    free_before = torch.cuda.mem_get_info()[0]
    o, lse = ops.attention_forward(qkv, H, klen, True, 0.1, 3, 0)
    dqkv = ops.attention_backward(do, qkv, o, lse, H, klen, True, 0.1, 3, 0)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    taken = free_before - torch.cuda.mem_get_info()[0]
    print("attention memory: torch peak growth {} bytes, device memory taken {} bytes, scores {}".format(
        growth, taken, scores))
    # (the device-wide figure is printed only: other processes share the device.  The library's scratch is delta,
    # one float per (b, h, t): 131 KB here)
    assert growth < scores // 4
    assert torch.isfinite(o).all() and torch.isfinite(dqkv).all()
    # outputs only: o, lse and dqkv
    assert growth <= (o.numel() + lse.numel() + dqkv.numel()) * 4 + (1 << 20)
