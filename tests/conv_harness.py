"""What tests/test_gpu_conv1d.py (fixed CASES) and scripts/conv_fuzz.py (random cases) share: operands with a chosen
row pitch, outputs as column slices of sentinel-filled buffers, one run of the three Conv1d products with the checks
that need no tolerance (sentinels, finite garbage in the pad floats), the float64 reference (tests/conv_ref.py) and the
yardstick of scripts/bench_conv1d.py.  The callers compare `Results.items()` with the reference under their own
assertion of the project's bounds."""
import collections

import torch

from conv_ref import conv_ref, im2col, out_len, same_pad, weight_matrix
from idiaptts_amd import ops

SENTINEL = -7.25      # what the columns around an output slice hold before and must hold after
GARBAGE = 1e30        # finite, in the 1-3 pad floats of a row whose pitch is a multiple of 4 and whose width is not
PRODUCTS = ["fwd", "bwd_input", "bwd_weight"]

# pad: an int; pitch: tight (C), pad4 (the next multiple of 4: 16-byte rows, what the model path allocates), odd (no
# multiple of 4), unaligned (16-byte pitch, base 4 bytes off); act / act_prev: "none" / "tanh" / "relu" / None
Geometry = collections.namedtuple("Geometry", "B T Cin Cout Kw dil pad bf pitch bias act act_prev accumulate want_bias")

Case = collections.namedtuple("Case", "name geo plan yardstick")


def _case(name, shape, plan, bf=True, pitch="pad4", bias=True, act="none", act_prev=None, accumulate=False,
          want_bias=True, yardstick=False):
    B, T, Cin, Cout, Kw, dil, pad = shape
    return Case(name, Geometry(B, T, Cin, Cout, Kw, dil, same_pad(pad, Kw, dil), bf, pitch, bias, act, act_prev,
                               accumulate, want_bias), plan, yardstick)


BENCH_512 = (32, 1600, 512, 512, 5, 1, "same")      # the shapes scripts/bench_conv1d.py times
BENCH_425 = (32, 1600, 425, 512, 5, 1, "same")
BENCH_409 = (32, 1600, 409, 16, 3, 1, "same")
TN2_TAILS = (11, 1500, 130, 130, 3, 1, "same")      # 16 500 = 128 * 128 + 116 rows; column tile 2 holds 2 columns
SHORT_SLAB = (9, 1000, 130, 200, 3, 2, "same")      # 9 000 rows in 36 slabs of 256, the last 40
NARROW_SLABS = (4, 300, 20, 16, 5, 1, "same")       # 1 200 rows in 5 slabs of 256 (the last 176) on the 64-wide tile
# plan: (tile_cols, slabs, kchunk) of the forward, the input gradient and the weight gradient, worked out from the
# sizes by hand (M x N over K as in conv1d.hip: 128-wide when N > 64 and ceil(M / 128) ceil(N / 128) slabs >= 256;
# slabs: min(512 / tiles, ceil(rows / 256), 128) rounded to whole 32-row K steps) and asserted against the library
# (tests/test_conv_plan.py without a GPU, test_production_size_paths before it runs a case)
CASES = [
    _case("bench-512x512-k5", BENCH_512, ((128, 1, 2560), (128, 1, 2560), (128, 6, 8544)), yardstick=True),
    _case("bench-425x512-k5", BENCH_425, ((128, 1, 2144), (128, 1, 2560), (128, 7, 7328)), yardstick=True),
    # 50 slabs where the workspace is sized for 51: rounding 1004 rows up to 1024 leaves one fewer
    _case("bench-409x16-k3", BENCH_409, ((64, 1, 1248), (128, 1, 64), (128, 50, 1024)), yardstick=True),
    _case("bench-425x512-k5-time-major", BENCH_425, ((128, 1, 2144), (128, 1, 2560), (128, 7, 7328)), bf=False),
    _case("tn2-tails", TN2_TAILS, ((128, 1, 416), (128, 1, 416), (128, 58, 288)), yardstick=True),
    _case("tn2-tails-tanh-time-major", TN2_TAILS, ((128, 1, 416), (128, 1, 416), (128, 58, 288)), bf=False,
          act="tanh", act_prev="tanh"),
    _case("tn2-tails-relu-no-bias-odd-pitch", TN2_TAILS, ((128, 1, 416), (128, 1, 416), (128, 58, 288)),
          pitch="odd", bias=False, act="relu", act_prev="relu"),
    _case("tn2-tails-unaligned-base", TN2_TAILS, ((128, 1, 416), (128, 1, 416), (128, 58, 288)), pitch="unaligned",
          act="tanh"),
    _case("short-last-slab", SHORT_SLAB, ((64, 1, 416), (64, 1, 608), (128, 36, 256)), yardstick=True),
    _case("short-last-slab-accumulate-odd-pitch", SHORT_SLAB, ((64, 1, 416), (64, 1, 608), (128, 36, 256)),
          pitch="odd", accumulate=True),
    _case("short-last-slab-no-db-unaligned", SHORT_SLAB, ((64, 1, 416), (64, 1, 608), (128, 36, 256)),
          pitch="unaligned", want_bias=False, bf=False),
    _case("slabs-on-64-wide-tile", NARROW_SLABS, ((64, 1, 128), (64, 1, 96), (64, 5, 256))),
    _case("slabs-on-64-wide-tile-accumulate-odd-pitch", NARROW_SLABS, ((64, 1, 128), (64, 1, 96), (64, 5, 256)),
          accumulate=True, pitch="odd"),
    # T_out = 1: every row its own utterance (division by 1); 2 slabs of 160 rows, the last 140
    _case("t-out-1", (300, 5, 70, 70, 5, 1, 0), ((64, 1, 384), (64, 1, 384), (64, 2, 160))),
    # tiles of 128 rows straddle utterances of 256 (a power of two) and 257 (a prime) steps
    _case("t-out-256", (70, 256, 130, 130, 3, 1, "same"), ((128, 1, 416), (128, 1, 416), (128, 63, 288))),
    _case("t-out-257-time-major", (70, 257, 130, 130, 3, 1, "same"), ((128, 1, 416), (128, 1, 416), (128, 63, 288)),
          bf=False, pitch="odd"),
]


def rows16(g, C):
    """whether rows of C floats with the pitch of `g` are 16-byte rows"""
    return g.pitch == "pad4" or (g.pitch == "tight" and C % 4 == 0)


def expected_vec(g):
    """16-byte operand loads per product: x for the forward, dz for the input gradient, both for the weight gradient"""
    return rows16(g, g.Cin), rows16(g, g.Cout), rows16(g, g.Cin) and rows16(g, g.Cout)


def rows(dev, shape, pitch, gen):
    """a random [d0, d1, C] view of rows with the pitch asked for, and the view of the pad floats that 16-byte loads
    read and must mask (pad4 with C no multiple of 4; None otherwise: the other loads never touch them)"""
    d0, d1, C = shape
    C4 = (C + 3) // 4 * 4
    ld = {"tight": C, "pad4": C4, "odd": C4 + 1, "unaligned": C4 + 4}[pitch]
    off = 1 if pitch == "unaligned" else 0
    buf = torch.zeros(off + d0 * d1 * ld + 4, device=dev)
    full = buf[off:off + d0 * d1 * ld].view(d0, d1, ld)
    full[..., :C] = torch.randn(shape, device=dev, generator=gen)
    return full[..., :C], (full[..., C:] if pitch == "pad4" and ld > C else None)


def rows_vec(*views):
    """Whether the entry points take 16-byte loads from these operands.  A restatement, for counting only, of their
    rule `pitch % 4 == 0 && 16-byte aligned base` (conv1d.hip: rows16) on the pitch and pointer that ops.conv1d_*
    pass on; the plan does not depend on it today, and the library does not report it."""
    for t in views:
        kept, ld = ops._conv_rows(t, "operand")
        assert kept is t, "the operand would be copied: not the pitch the case asked for"
        if ld % 4 or t.data_ptr() % 16:
            return False
    return True


def sliced_out(dev, shape, col0):
    wide = torch.full(tuple(shape[:2]) + (shape[2] + col0 + 3,), SENTINEL, device=dev)
    return wide, wide[..., col0:col0 + shape[2]]


def yardstick(product, g, x, w, b, dz, yprev):
    """scripts/bench_conv1d.py's yardstick for one product: the dense-layer kernels on an explicit fp32 im2col of the
    same values (same arithmetic and reduction length as the conv kernel; batch-first copies, the layout does not
    enter its arithmetic) -> y, dx or (dw, db) in the layout of the case"""
    xb, dzb = (t.contiguous() if g.bf else t.permute(1, 0, 2).contiguous() for t in (x, dz))
    (B, T, Cin), (T_out, Cout), Kw = xb.shape, dzb.shape[1:], g.Kw
    if product == 1:
        # dx[t] = sum_k' dz[t + k' dil + pad - dil (Kw - 1)] w[:, :, Kw - 1 - k']: the same correlation on dz
        dzcol = im2col(dzb, Kw, g.pad - g.dil * (Kw - 1), g.dil, T).reshape(B * T, Kw * Cout)
        yp = None if yprev is None else (yprev if g.bf else yprev.permute(1, 0, 2)).reshape(B * T, Cin).contiguous()
        out = ops.linear_bwd_input(dzcol, w.flip(2).permute(2, 0, 1).reshape(Kw * Cout, Cin).contiguous(), yp,
                                   ops.ACT_BY_NAME[g.act_prev]).reshape(B, T, Cin)
        return out if g.bf else out.permute(1, 0, 2)
    xcol = im2col(xb, Kw, -g.pad, g.dil, T_out).reshape(B * T_out, Kw * Cin)
    if product == 0:
        out = ops.linear_fwd(xcol, weight_matrix(w).contiguous(), b, ops.ACT_BY_NAME[g.act]).reshape(B, T_out, Cout)
        return out if g.bf else out.permute(1, 0, 2)
    dw, db = ops.linear_bwd_weight(dzb.reshape(B * T_out, Cout), xcol)
    return dw.reshape(Cout, Kw, Cin).permute(0, 2, 1), db


class Results(object):
    """got / ref per key ("fwd", "bwd_input", "bwd_weight", "bwd_weight(db)") of one case, and its yardstick"""

    def __init__(self, g, got, ref, operands, added):
        self.g, self.got, self.ref, self._operands, self._added = g, got, ref, operands, added

    def items(self):
        """(key, got, float64 reference, relative bound of the project) per result"""
        for key in self.got:
            yield key, self.got[key], self.ref[key], (3e-6 if key.startswith("bwd_weight") else 2e-6)

    def yardstick(self, key):
        """the yardstick's result for `key` on the same data (what accumulate added is added here too)"""
        product = PRODUCTS.index(key.split("(")[0])
        out = yardstick(product, self.g, *self._operands)
        if product == 2:
            out = out[1 if key.endswith("(db)") else 0]
            if self.g.accumulate:
                out = out + self._added[1 if key.endswith("(db)") else 0]
        return out


def run_case(dev, g, gen, note=""):
    """All three products of geometry `g` on random data: outputs written into column slices of sentinel-filled
    buffers (the columns around them must stay bit-unchanged); where an operand has pad floats (pad4 pitch, channels
    no multiple of 4), 1e30 in them must change no bit of any result.  Asserts that the operands give the 16-byte /
    plain loads their pitch stands for.  Returns the Results for the caller's comparison."""
    B, T, Cin, Cout, Kw, dil, pad, bf = g[:8]
    T_out = out_len(T, Kw, pad, dil)
    x, x_pads = rows(dev, (B, T, Cin) if bf else (T, B, Cin), g.pitch, gen)
    dz, dz_pads = rows(dev, (B, T_out, Cout) if bf else (T_out, B, Cout), g.pitch, gen)
    w = torch.randn((Cout, Cin, Kw), device=dev, generator=gen) / (Cin * Kw) ** 0.5
    b = torch.randn((Cout,), device=dev, generator=gen) if g.bias else None
    yprev = None
    if g.act_prev is not None:
        yprev = (torch.tanh if g.act_prev == "tanh" else torch.relu)(x).contiguous()
    dw0 = torch.randn((Cout, Cin, Kw), device=dev, generator=gen)
    db0 = torch.randn((Cout,), device=dev, generator=gen)
    if B * T > 1 and B * T_out > 1:      # (a single row has no pitch: ops passes its width on)
        assert (rows_vec(x), rows_vec(dz), rows_vec(dz, x)) == expected_vec(g), (note, g)
    act, act_prev = ops.ACT_BY_NAME[g.act], ops.ACT_BY_NAME[g.act_prev]

    def run():
        ywide, y = sliced_out(dev, dz.shape, 2)
        dxwide, dx = sliced_out(dev, x.shape, 3)
        ops.conv1d_fwd(x, w, b, pad, dil, bf, act, out=y)
        ops.conv1d_bwd_input(dz, w, T, pad, dil, bf, yprev=yprev, act_prev=act_prev, out=dx)
        if g.accumulate:
            dw, db = ops.conv1d_bwd_weight(dz, x, Kw, pad, dil, bf, dw=dw0.clone(),
                                           db=db0.clone() if g.want_bias else None, accumulate=True,
                                           want_bias=g.want_bias)
        else:
            dw, db = ops.conv1d_bwd_weight(dz, x, Kw, pad, dil, bf, want_bias=g.want_bias)
        return ywide, dxwide, dw, db

    ywide, dxwide, dw, db = run()
    for wide, col0, C, what in ((ywide, 2, Cout, "y"), (dxwide, 3, Cin, "dx")):
        assert bool((wide[..., :col0] == SENTINEL).all()) and bool((wide[..., col0 + C:] == SENTINEL).all()), \
            (what, "columns outside the output slice were written", note, g)
    assert g.want_bias or db is None
    if x_pads is not None or dz_pads is not None:
        for pads in (x_pads, dz_pads):
            if pads is not None:
                pads.fill_(GARBAGE)
        for clean, dirty, what in zip((ywide, dxwide, dw, db), run(), ("y", "dx", "dw", "db")):
            assert clean is None or torch.equal(clean, dirty), (what, "changed with garbage in the pad floats", note, g)
    ry, rdx, rdw, rdb = conv_ref(x, w, b, pad, dil, bf, act=g.act, dz=dz, yprev=yprev, act_prev=g.act_prev or "none")
    if g.accumulate:
        rdw, rdb = rdw + dw0.double(), rdb + db0.double()
    got = collections.OrderedDict([("fwd", ywide[..., 2:2 + Cout]), ("bwd_input", dxwide[..., 3:3 + Cin]),
                                   ("bwd_weight", dw)])
    ref = {"fwd": ry, "bwd_input": rdx, "bwd_weight": rdw}
    if g.want_bias:
        got["bwd_weight(db)"], ref["bwd_weight(db)"] = db, rdb
    return Results(g, got, ref, (x, w, b, dz, yprev), (dw0, db0))
