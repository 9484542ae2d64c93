"""One dense-GEMM case (a row of tests/gemm_cases.py, or a drawn one of scripts/gemm_fuzz.py) on the GPU: operands and
results framed in wider buffers, the call, what ops.gemm_last_plan() recorded in the table's terms, and every check
that needs no knowledge of the variant.

Frames.  An input slice lies in a buffer of NaN: a read outside the slice spreads into the result.  The one place a
kernel may read outside is the 1-3 floats between the width and the next multiple of 4 of a 16-byte row ("v"; the
pitch rule of include/idiaptts_amd.h): those hold zeros.  An output slice lies in a buffer of SENTINEL (the slice
itself too: every element must be written).  Afterwards the frame still holds SENTINEL, except that the ring
kernel's epilogue writes zeros into the 1-3 pad floats of a 16-byte row; the register-staged kernel leaves them.

Bounds (those of tests/test_gpu_nn.py for the same entry points): ||got - ref|| / ||ref|| < 2e-6 and |got - ref| <
2e-5 for the forward product, the input gradient and the fused loss's gradient, < 3e-6 for dw and db, 1e-6 relative
for the loss; ref is torch float64 on the CPU.  Inputs as there and in test_gpu_sparse_wgrad.py: x and yprev in
(0, 1], dz uniform in (-0.25, 0.75) (a single output, N = K = 1, is then no cancelling sum), w zero-mean and scaled by
the reduction length.  The same operation in float32 torch on the CPU is held to the same bounds first, so that a
bound a case cannot meet shows as the inputs' fault, not the kernel's."""
import collections
import zlib

import torch

from gemm_cases import Pair, Reduce, Ring, Staged, pad4, pitch

SENTINEL = 7.0
REL = {"y": 2e-6, "dx": 2e-6, "g": 2e-6, "dw": 3e-6, "db": 3e-6, "loss": 1e-6}
ABS = {"y": 2e-5, "dx": 2e-5, "g": 2e-5}
Result = collections.namedtuple("Result", "plan figures outputs")     # figures: {key: (kernel / bound, float32 torch / bound)}


def normalise(plan):
    """ops.gemm_last_plan() in the terms of tests/gemm_cases.py"""
    out, i = [], 0
    while i < len(plan):
        e = plan[i]
        if hasattr(e, "slabs"):
            out.append(Reduce(int(e.vec), int(e.merged), int(e.deferred), e.slabs))
        elif e.kernel == "staged":
            out.append(Staged(int(e.a_row), int(e.b_row), e.epi, e.tn, e.stages, int(e.vec_a), int(e.vec_b), int(e.wide),
                              e.splitk, e.family))
        elif e.kernel == "ring":
            out.append(Ring(int(e.a_row), int(e.b_row), e.epi, e.wm, int(e.grouped), e.splitk, e.family,
                            int(e.tiles > e.grid)))
        else:
            x = plan[i + 1]
            assert x.kernel == "ring_pair" and (e.a_row, e.b_row, e.epi) == (False, False, "store"), plan
            assert (x.a_row, x.b_row, x.wm, x.splitk) == (True, False, 2, 1) and e.grid == x.grid, plan
            out.append(Pair(e.wm, e.splitk, x.epi, x.family, int(e.tiles + x.tiles > e.grid)))
            i += 1
        i += 1
    return out


def _off(lay):
    return 1 if lay == "u" else 4


def frame_in(data, lay, dev):
    """data [rows, W] as a slice of a NaN buffer (zeros in the pad floats of a 16-byte row); (buffer, view)"""
    rows, W = data.shape
    buf = torch.full((rows, pitch(W, lay)), float("nan"))
    o = _off(lay)
    if lay == "v":
        buf[:, o:o + pad4(W)] = 0.0
    buf[:, o:o + W] = data
    buf = buf.to(dev)
    return buf, buf[:, o:o + W]


def frame_out(rows, W, lay, dev):
    buf = torch.full((rows, pitch(W, lay)), SENTINEL, device=dev)
    o = _off(lay)
    return buf, buf[:, o:o + W]


def flat_in(data, lay, dev):
    buf = torch.full((data.numel() + 8,), float("nan"))
    o = _off(lay)
    buf[o:o + data.numel()] = data.reshape(-1)
    buf = buf.to(dev)
    return buf, buf[o:o + data.numel()].view(data.shape)


def check_out_frame(buf, W, lay, zero_pads, what):
    o = _off(lay)
    host = buf.cpu()
    assert bool((host[:, :o] == SENTINEL).all()), (what, "columns in front of the slice were written")
    behind = o + W
    if zero_pads and lay == "v" and W % 4:
        assert bool((host[:, o + W:o + pad4(W)] == 0).all()), (what, "pad floats of the 16-byte row are not zero")
        behind = o + pad4(W)
    bad = (host[:, behind:] != SENTINEL).nonzero()
    assert bad.numel() == 0, (what, "columns behind the slice were written", bad[:4].tolist(),
                              host[:, behind:][host[:, behind:] != SENTINEL][:4].tolist())


def _act(z, act):
    if act == 1:
        return torch.tanh(z)
    if act == 2:
        return torch.relu(z)
    if act == 3:
        return torch.sigmoid(z)
    if act == 6:
        return z / (1 + z.abs())
    if act == 7:
        return torch.where(z > 0, z, 0.01 * z)
    assert act == 0, act
    return z


def _dact(y, act):
    if act == 1:
        return 1 - y * y
    if act == 2:
        return (y > 0).to(y.dtype)
    if act == 3:
        return y * (1 - y)
    if act == 6:
        return (1 - y.abs()) ** 2
    if act == 7:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.01))
    assert act == 0, act
    return torch.ones_like(y)


def _inputs(c):
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()) + 7 * c.M)
    M, N, K = c.M, c.N, c.K
    d = {"x": 1.0 - torch.rand(M, K, generator=g), "b": torch.rand(N, generator=g) - 0.5,
         "dz": torch.rand(M, N, generator=g) - 0.25, "t": torch.randn(M, N, generator=g)}
    red = K if c.entry in ("fwd", "mse") else N
    d["w"] = (torch.rand(N, K, generator=g) - 0.5) * (2.0 / red ** 0.5)
    d["yp"] = 1.0 - torch.rand(M, K, generator=g)
    valid = (torch.rand(M, generator=g) > 0.2).to(torch.uint8)
    valid[M // 2] = 1
    d["valid"] = valid
    return d


def reference(c, d, dtype):
    """the row's operation in plain torch on the CPU, in `dtype`"""
    f = {k: v.to(dtype) for k, v in d.items() if k != "valid"}
    lay, out = c.lay, {}
    if c.entry in ("fwd", "mse"):
        z = f["x"] @ f["w"].t()
        if lay["b"] is not None:
            z = z + f["b"]
        if c.entry == "fwd":
            out["y"] = _act(z, c.act)
        else:
            v = d["valid"].to(dtype)[:, None]
            nv = float(d["valid"].sum())
            diff = (z - f["t"]) * v
            out["loss"] = (diff * diff).sum().reshape(1) / (nv * c.N)
            out["g"] = diff * (2.0 / (nv * c.N))
    if c.entry in ("bwd_input", "bwd"):
        dx = f["dz"] @ f["w"]
        out["dx"] = dx * _dact(f["yp"], c.act) if lay["yp"] is not None else dx
    if c.entry in ("bwd_weight", "bwd"):
        out["dw"] = f["dz"].t() @ f["x"]
        if lay["db"] is not None:
            out["db"] = f["dz"].sum(0)
    return out


def errors(key, got, ref):
    """(error / bound) of a result against the float64 reference: the larger of the relative-L2 and the absolute one"""
    got, ref = got.double(), ref.double()
    if key == "loss":
        return float((got - ref).abs() / ref.abs().clamp_min(1e-300)) / REL[key]
    r = float((got - ref).norm()) / (float(ref.norm()) + 1e-30) / REL[key]
    if key in ABS:
        r = max(r, float((got - ref).abs().max()) / ABS[key])
    return r if r == r else float("inf")


class _Buffers(object):
    """the framed operands of one call"""

    def __init__(self, c, d, dev):
        self.c, lay = c, c.lay
        self.ins, self.outs = {}, {}
        for k in ("x", "dz", "t", "yp"):
            if lay.get(k) is not None:
                self.ins[k] = frame_in(d[k], lay[k], dev)
        for k in ("w", "b"):
            if lay.get(k) is not None:
                self.ins[k] = flat_in(d[k], lay[k], dev)
        self.before = {k: v[0].clone() for k, v in self.ins.items()}
        M, N, K = c.M, c.N, c.K
        for k, W in (("y", N), ("g", N), ("dx", K)):
            if k in lay:
                self.outs[k] = frame_out(M, W, lay[k], dev)
        if "dw" in lay:
            n, o = N * K, _off(lay["dw"])
            flat = torch.full((n + N + 8,), SENTINEL, device=dev)
            self.flat_dw, self.dw = flat, flat[o:o + n].view(N, K)
            self.db, self.flat_db = None, None
            if lay["db"] == "behind":
                self.db = flat[o + n:o + n + N]
            elif lay["db"] is not None:
                self.flat_db = torch.full((N + 8,), SENTINEL, device=dev)
                self.db = self.flat_db[4:4 + N]

    def view(self, k):
        return self.ins[k][1] if k in self.ins else None

    def call(self, ops, valid, accumulate=False):
        c, v = self.c, self.view
        if c.entry == "fwd":
            ops.linear_fwd(v("x"), v("w"), v("b"), c.act, out=self.outs["y"][1])
        elif c.entry == "mse":
            self.loss, _ = ops.linear_fwd_mse(v("x"), v("w"), v("b"), v("t"), valid, float(valid.sum()),
                                              grad=self.outs["g"][1])
        elif c.entry == "bwd_input":
            ops.linear_bwd_input(v("dz"), v("w"), yprev=v("yp"), act_prev=c.act, out=self.outs["dx"][1])
        elif c.entry == "bwd_weight":
            ops.linear_bwd_weight(v("dz"), v("x"), dw=self.dw, db=self.db, accumulate=accumulate,
                                  want_bias=self.db is not None)
        else:
            ops.linear_bwd(v("dz"), v("x"), v("w"), self.dw, self.db, self.outs["dx"][1], yprev=v("yp"),
                           act_prev=c.act, accumulate=accumulate)
        return normalise(ops.gemm_last_plan())

    def results(self):
        out = {k: view for k, (_, view) in self.outs.items()}
        if self.c.entry == "mse":
            out["loss"] = self.loss
        if "dw" in self.c.lay:
            out["dw"] = self.dw
            if self.db is not None:
                out["db"] = self.db
        return out

    def check_frames(self, plan):
        c = self.c
        for k, buf in self.before.items():        # (bit patterns: NaN != NaN)
            assert torch.equal(buf.view(torch.int32), self.ins[k][0].view(torch.int32)), (c.name, k, "an input was written")
        for k, (buf, _) in self.outs.items():
            # the ring kernel's epilogue zeroes the pad floats of a 16-byte row; nothing else may
            ring = any(isinstance(e, Pair) or (isinstance(e, Ring) and e.a_row) for e in plan)
            check_out_frame(buf, c.N if k in ("y", "g") else c.K, c.lay[k], ring, (c.name, k))
        if "dw" in c.lay:
            n, N, o = c.N * c.K, c.N, _off(c.lay["dw"])
            host = self.flat_dw.cpu()
            used = n + (N if c.lay["db"] == "behind" else 0)
            assert bool((host[:o] == SENTINEL).all()) and bool((host[o + used:] == SENTINEL).all()), (c.name, "around dw")
            if self.flat_db is not None:
                host = self.flat_db.cpu()
                assert bool((host[:4] == SENTINEL).all()) and bool((host[4 + N:] == SENTINEL).all()), (c.name, "around db")


def _run(ops, bufs, valid, deferred, accumulate=False):
    if deferred:
        with ops.deferred_reductions():
            plan = bufs.call(ops, valid, accumulate)
    else:
        plan = bufs.call(ops, valid, accumulate)
    torch.cuda.synchronize()
    return plan


def run_case(c, dev, ops):
    """Runs a case; asserts everything but the plan and the bounds, which the caller judges from the Result."""
    d = _inputs(c)
    valid = d["valid"].to(dev)
    ref = reference(c, d, torch.float64)
    ref32 = reference(c, d, torch.float32)
    bufs = _Buffers(c, d, dev)
    plan = _run(ops, bufs, valid, c.deferred)
    got = {k: v.clone() for k, v in bufs.results().items()}
    assert set(got) == set(ref), (c.name, sorted(got), sorted(ref))
    figures = {k: (errors(k, got[k].cpu(), ref[k]), errors(k, ref32[k], ref[k])) for k in sorted(ref)}
    bufs.check_frames(plan)
    if c.entry == "mse":
        assert bool((got["g"][valid == 0] == 0).all()), (c.name, "gradient in a masked row")
    # a second run into fresh frames: the same plan, the same bits
    again = _Buffers(c, d, dev)
    plan2 = _run(ops, again, valid, c.deferred)
    assert plan2 == plan, (c.name, plan, plan2)
    for k, v in again.results().items():
        assert torch.equal(v, got[k]), (c.name, k, "differs between two runs")
    if "dw" in c.lay:
        # accumulate onto the result itself: exactly twice (the same sum added to itself)
        plan3 = _run(ops, again, valid, c.deferred, accumulate=True)
        assert plan3 == plan, (c.name, plan, plan3)
        res = again.results()
        assert torch.equal(res["dw"], 2 * got["dw"]), (c.name, "accumulate: dw is not twice the result")
        if "db" in res:
            assert torch.equal(res["db"], 2 * got["db"]), (c.name, "accumulate: db is not twice the result")
        if "dx" in res:
            assert torch.equal(res["dx"], got["dx"]), (c.name, "accumulate changed dx")
        again.check_frames(plan3)
    return Result(plan, figures, got)
