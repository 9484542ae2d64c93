"""The C boundary of csrc/latent.hip (time pooling, VAE reparameterisation, KL term) without a GPU: header, ctypes
binding and exports agree; every refusal comes back as ITTS_E_INVALID with a message naming the offending value
before any device work (the pointers handed in are null or bogus: a call that got as far as a launch would not
return -1); empty calls succeed; the plan query matches expectations written out by hand."""
import ctypes
import os
import re

import pytest

from idiaptts_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("itts_time_pool_plan", "itts_time_pool_fwd", "itts_time_pool_bwd", "itts_vae_reparam_fwd",
           "itts_vae_reparam_bwd", "itts_vae_kld_workspace_bytes", "itts_vae_kld")
P = ctypes.c_void_p(64)       # never dereferenced: every call below is refused or empty
LAST, MEAN = 0, 1


def _pool_fwd(L, x=P, ldx=None, lens=P, B=3, T=5, D=7, bf=1, mode=MEAN, y=P, ldy=None, ws=P):
    return L.itts_time_pool_fwd(x, D if ldx is None else ldx, lens, B, T, D, bf, mode, y, D if ldy is None else ldy,
                                ws, None)


def _pool_bwd(L, dy=P, lddy=None, lens=P, B=3, T=5, D=7, bf=1, mode=MEAN, dx=P, lddx=None):
    return L.itts_time_pool_bwd(dy, D if lddy is None else lddy, lens, B, T, D, bf, mode, dx,
                                D if lddx is None else lddx, None)


def _rep_fwd(L, h=P, ldh=None, eps=P, lde=None, z=P, ldz=None, M=4, lat=3):
    return L.itts_vae_reparam_fwd(h, 2 * lat if ldh is None else ldh, eps, lat if lde is None else lde, z,
                                  lat if ldz is None else ldz, M, lat, None)


def _rep_bwd(L, dz=P, dmu=P, dlv=P, h=P, eps=P, dh=P, lddh=None, lddz=None, M=4, lat=3):
    return L.itts_vae_reparam_bwd(dz, lat if lddz is None else lddz, dmu, lat, dlv, lat, h, 2 * lat, eps, lat, dh,
                                  2 * lat if lddh is None else lddh, M, lat, None)


def _kld(L, mu=P, ldmu=None, lv=P, w=P, M=4, lat=3, loss=P, dmu=P, dlv=P, lddlv=None, elem=None, ws=P):
    return L.itts_vae_kld(mu, lat if ldmu is None else ldmu, lv, lat, w, M, lat, loss, dmu, lat, dlv,
                          lat if lddlv is None else lddlv, elem, ws, None)


def test_header_binding_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "idiaptts_amd.h")).read()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in SYMBOLS:
        proto = re.search(r"\b(int|int64_t) " + name + r"\s*\(([^)]*)\)", text)
        assert proto, name + " is not declared in the header"
        assert hasattr(cdll, name), "missing export " + name
        restype, argtypes = lib._SIGNATURES[name]
        assert restype is (ctypes.c_int if proto.group(1) == "int" else ctypes.c_int64)
        assert len(argtypes) == len(proto.group(2).split(",")), name + ": binding and header differ in arity"
    # each cites its reference call site
    for cite in ("rnn_dyn/Pooling.py:30-44", ":52-65", "rnn_dyn/Pooling.py:42-44", "rnn_dyn/VAE.py:23-27",
                 "rnn_dyn/VAE.py:19-27", "loss/VAEKLDLoss.py:56-58"):
        assert cite in text, cite
    from idiaptts_amd import ops
    assert (ops.POOL_LAST, ops.POOL_MEAN) == (LAST, MEAN)
    assert re.search(r"#define ITTS_POOL_LAST 0\b", text) and re.search(r"#define ITTS_POOL_MEAN 1\b", text)


@pytest.mark.parametrize("call,kwargs,needle", [
    (_pool_fwd, dict(D=0), "width = 0"),
    (_pool_bwd, dict(D=0), "width = 0"),
    (_pool_fwd, dict(T=0), "t_max = 0"),
    (_pool_bwd, dict(T=0), "t_max = 0"),
    (_pool_fwd, dict(T=128 * 65535 + 1), "t_max = 8388481"),
    (_pool_fwd, dict(mode=2), "mode = 2"),
    (_pool_bwd, dict(mode=2), "mode = 2"),
    (_pool_fwd, dict(mode=-1), "mode = -1"),
    (_pool_fwd, dict(B=-2), "n_utts = -2"),
    (_pool_fwd, dict(ldx=6), "ldx = 6"),
    (_pool_fwd, dict(ldy=5), "ldy = 5"),
    (_pool_bwd, dict(lddy=6), "lddy = 6"),
    (_pool_bwd, dict(lddx=4), "lddx = 4"),
    (_pool_fwd, dict(lens=None), "d_lens is NULL"),
    (_pool_bwd, dict(lens=None), "d_lens is NULL"),
    (_pool_fwd, dict(x=None), "null pointer (d_x / d_y) with n_utts = 3"),
    (_pool_fwd, dict(y=None, mode=LAST), "null pointer (d_x / d_y) with n_utts = 3"),
    (_pool_bwd, dict(dy=None), "null pointer (d_dy / d_dx) with n_utts = 3"),
    (_pool_bwd, dict(dx=None, mode=LAST, lens=None), "null pointer (d_dy / d_dx) with n_utts = 3"),
    # 1 utterance x 1 column tile and 3 segments: the time-split form needs its workspace
    (_pool_fwd, dict(B=1, T=300, ws=None), "null workspace"),
    (_rep_fwd, dict(lat=0), "L = 0"),
    (_rep_bwd, dict(lat=0), "L = 0"),
    (_kld, dict(lat=0), "L = 0"),
    (_rep_fwd, dict(M=-1), "M = -1"),
    (_rep_fwd, dict(ldh=5), "ldh = 5"),
    (_rep_fwd, dict(lde=2), "lde = 2"),
    (_rep_fwd, dict(ldz=2), "ldz = 2"),
    (_rep_bwd, dict(lddh=5), "lddh = 5"),
    (_rep_bwd, dict(lddz=2), "lddz = 2"),
    (_kld, dict(ldmu=2), "ldmu = 2"),
    (_kld, dict(lddlv=1), "lddlv = 1"),
    (_rep_fwd, dict(h=None), "null pointer (d_h / d_eps / d_z) with M = 4"),
    (_rep_fwd, dict(z=None), "null pointer (d_h / d_eps / d_z) with M = 4"),
    (_rep_bwd, dict(dh=None), "null pointer (d_dh) with M = 4"),
    (_rep_bwd, dict(eps=None), "null pointer (d_h / d_eps)"),
    (_kld, dict(loss=None), "null pointer (d_loss)"),
    (_kld, dict(mu=None), "with M = 4"),
    (_kld, dict(w=None), "with M = 4"),
    (_kld, dict(ws=None), "with M = 4"),
])
def test_refusals_name_the_value(call, kwargs, needle):
    L = lib.load()
    assert call(L, **kwargs) == -1
    msg = L.itts_last_error().decode()
    assert msg.startswith({_pool_fwd: "itts_time_pool_fwd", _pool_bwd: "itts_time_pool_bwd",
                           _rep_fwd: "itts_vae_reparam_fwd", _rep_bwd: "itts_vae_reparam_bwd",
                           _kld: "itts_vae_kld"}[call]), msg
    assert needle in msg, msg


def test_empty_calls_succeed_and_sizes_are_still_checked():
    L = lib.load()
    assert _pool_fwd(L, B=0, x=None, lens=None, y=None, ws=None) == 0
    assert _pool_fwd(L, B=0, mode=LAST, x=None, lens=None, y=None, ws=None) == 0
    assert _pool_bwd(L, B=0, dy=None, lens=None, dx=None) == 0
    assert _pool_fwd(L, B=0, D=0) == -1
    # the frame limit belongs to the time-split MEAN forward alone: LAST and the backward take any t_max
    assert _pool_fwd(L, B=0, mode=LAST, T=128 * 65535 + 1) == 0 and _pool_bwd(L, B=0, T=128 * 65535 + 1) == 0
    assert _pool_bwd(L, B=0, mode=LAST, T=1 << 40) == 0
    assert _rep_fwd(L, M=0, h=None, eps=None, z=None) == 0
    assert _rep_bwd(L, M=0, dz=None, dmu=None, dlv=None, h=None, eps=None, dh=None) == 0
    assert _rep_fwd(L, M=0, lat=0) == -1
    assert L.itts_vae_kld_workspace_bytes(0, 4) == 0 and L.itts_vae_kld_workspace_bytes(4, 0) == 0


def test_kld_workspace_is_one_double_per_block():
    L = lib.load()
    # four rows (one per wave) a block up to 1024 blocks, then more rows per block
    assert L.itts_vae_kld_workspace_bytes(1, 4) == 8
    assert L.itts_vae_kld_workspace_bytes(4, 4) == 8
    assert L.itts_vae_kld_workspace_bytes(5, 257) == 16
    assert L.itts_vae_kld_workspace_bytes(4096, 4) == 8 * 1024
    assert L.itts_vae_kld_workspace_bytes(4097, 4) == 8 * 513        # 8 rows a block


@pytest.mark.parametrize("B,T,D,segments,split,nbytes", [
    (1, 1, 1, 1, False, 0),                    # one segment: nothing to split
    (64, 40, 512, 1, False, 0),
    (64, 128, 512, 1, False, 0),               # a full segment
    (64, 129, 512, 2, True, 64 * 2 * 512 * 4),  # 64 utterances x 2 column tiles = 128 pairs < 512
    (5, 257, 67, 3, True, 5 * 3 * 67 * 4),
    (4, 1600, 130, 13, True, 4 * 13 * 130 * 4),
    (1, 2049, 64, 17, True, 17 * 64 * 4),
    (511, 130, 5, 2, True, 511 * 2 * 5 * 4),   # the threshold: 512 (utterance, tile) pairs fill the GPU
    (512, 130, 5, 2, False, 0),
    (256, 130, 257, 2, False, 0),              # 257 columns are two tiles
    (256, 130, 256, 2, True, 256 * 2 * 256 * 4),
])
def test_plan_query(B, T, D, segments, split, nbytes):
    from idiaptts_amd import ops
    assert ops.time_pool_plan(B, T, D) == (segments, split, nbytes)


def test_plan_query_refuses_what_the_entry_points_refuse():
    L = lib.load()
    for B, T, D in ((-1, 5, 7), (3, 0, 7), (3, 5, 0), (3, 128 * 65535 + 1, 7)):
        assert L.itts_time_pool_plan(B, T, D, None, None, None) == -1
    assert L.itts_time_pool_plan(3, 128 * 65535, 7, None, None, None) == 0
    assert L.itts_time_pool_plan(512, 128 * 65535 + 1, 7, None, None, None) == 0       # not split: no such limit
    from idiaptts_amd import ops
    with pytest.raises(ValueError, match="t_max=0"):
        ops.time_pool_plan(3, 0, 7)


def test_python_side_checks_host_lengths():
    import torch
    from idiaptts_amd import ops
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match=r"1 \.\. t_max = 5, got 0 \.\. 3"):
        ops._pool_lens(torch.tensor([3, 0]), 2, 5, ops.POOL_LAST, dev)
    with pytest.raises(ValueError, match=r"got 2 \.\. 6"):
        ops._pool_lens([2, 6], 2, 5, ops.POOL_MEAN, dev)
    with pytest.raises(ValueError, match="3 lengths for 2 utterances"):
        ops._pool_lens([1, 2, 3], 2, 5, ops.POOL_MEAN, dev)
    with pytest.raises(ValueError, match="lens is None"):
        ops._pool_lens(None, 2, 5, ops.POOL_MEAN, dev)
    assert ops._pool_lens(None, 2, 5, ops.POOL_LAST, dev) is None
    assert ops._pool_lens([1, 5], 2, 5, ops.POOL_MEAN, dev).dtype == torch.int64
