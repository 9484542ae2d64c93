"""Random shapes and buffer layouts through the fp32 GEMM entry points against torch in float64.  A case calls each of
linear_fwd, linear_fwd_mse, linear_bwd_input, linear_bwd_weight and linear_bwd once, with shapes and layouts of its
own per call (tests/gemm_harness.py runs a call): operands in NaN frames,
results in sentinel frames, the bounds of tests/test_gpu_nn.py (relative L2 2e-6 and 2e-5 absolute for the forward
product, the input gradient and the fused loss's gradient, 3e-6 for dw and db, 1e-6 for the loss), the same bits
from a second run, exactly twice the gradient under accumulate.  Drawn per case: every operand's pitch and alignment,
bias or none, yprev or none, db separate / behind dw / none, reductions deferred or not, activations of both families.

The sampler is stratified, not long: the strata below are the pitch / alignment / size classes that the dispatch rules
of csrc/nn.hip tell apart, each drawn twice with random sizes inside its class, then at random.  Where a call lands is not
taken from the stratum but from what the call recorded (ops.gemm_last_plan), counted in the cells of
tests/gemm_cases.py; the script fails with "coverage too thin" unless every reachable cell was hit at least twice.

A result outside its bound fails the run unless float32 torch on the CPU misses the same bound on the same inputs and
the case is pinned by name in PINNED with its figure (none so far).

usage (GPU box): python scripts/gemm_fuzz.py [cases] [seed]"""
import collections
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gemm_cases as gc  # noqa: E402
from gemm_harness import run_case  # noqa: E402
from idiaptts_amd import ops  # noqa: E402

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 9
rng = np.random.default_rng(seed)
dev = torch.device("cuda", 0)
PINNED = {}          # case name -> {result: error / bound it is held to}; only where float32 torch misses the bound too
BASE, EXT = (gc.ACT_NONE, gc.ACT_TANH, gc.ACT_RELU), (gc.ACT_SIGMOID, gc.ACT_SOFTSIGN, gc.ACT_LEAKY_RELU)


def pick(*values):
    return values[int(rng.integers(0, len(values)))]


def between(lo, hi):
    return int(rng.integers(lo, hi + 1))


def any_size(hi=200):
    return pick(1, 3, 5, 31, 33, 63, 64, 65, 127, 128, 129, between(1, hi))


def mult4(lo=4, hi=200):
    return 4 * between((lo + 3) // 4, hi // 4)


def not_mult4(hi=200):
    return 4 * between(0, hi // 4 - 1) + between(1, 3)


def rows_operand(vec):
    """a layout that allows 16-byte accesses, or one that does not"""
    return "v" if vec else pick("o", "u")


def weight(vec):
    """(K, layout of w) with 16-byte rows of w or without"""
    if vec:
        return mult4(), "v"
    return (not_mult4(), pick("v", "u")) if rng.random() < 0.6 else (mult4(), "u")


def acts(family):
    return pick(*(EXT if family else BASE))


def tile_shape(wm):
    """(rows, columns) of an output that the ring kernel covers with 64 x 128 tiles (wm 1) or 128 x 64 tiles (wm 2)"""
    return (between(1, 64), mult4(68, 128)) if wm == 1 else (between(65, 128), mult4(4, 64))


def gradient_outputs():
    """(layout of dw, db) over the reduction forms"""
    return pick("v", "v", "u"), pick("sep", "behind", "behind", None)


STRATA = collections.defaultdict(list)       # entry point -> its strata


def stratum(entry):
    def register(fn):
        STRATA[entry].append(fn)
        return fn
    return register


def row_form_strata(entry):
    """the register-staged row-form kernel: 16-byte loads of either operand or not, wide stores or not, per epilogue"""
    for va in (0, 1):
        for vb in (0, 1):
            for wide in (0, 1):
                if va and vb and wide:
                    continue          # (the ring kernel's)
                for kind in ((0, 1) if entry == "fwd" else (None, 0, 1)):
                    def draw(va=va, vb=vb, wide=wide, kind=kind):
                        K, wl = weight(vb)
                        if entry == "fwd":
                            out = "v" if wide or (not (va and vb) and rng.random() < 0.3) else pick("o", "u")
                            b = pick("v", None) if wide else ("u" if out == "v" else pick("v", "u", None))
                            return dict(entry="fwd", M=any_size(300), N=any_size(), K=K, act=acts(kind),
                                        lay=dict(x=rows_operand(va), w=wl, b=b, y=out))
                        out = "v" if wide else pick("o", "u")
                        yp = None if kind is None else ("v" if wide else pick("o", "u", out))
                        if not wide and kind is not None and not (va and vb) and rng.random() < 0.3:
                            out, yp = "v", pick("o", "u")          # a 16-byte dx, yprev not
                        return dict(entry="bwd_input", M=any_size(300), N=any_size(), K=K, act=acts(kind or 0),
                                    lay=dict(dz=rows_operand(va), w=wl, yp=yp, dx=out))
                    STRATA[entry].append(draw)


row_form_strata("fwd")
row_form_strata("bwd_input")

for wm in (1, 2):
    for family in (0, 1):
        @stratum("fwd")
        def fwd_ring(wm=wm, family=family):
            M, N = tile_shape(wm)
            return dict(entry="fwd", M=M, N=N - between(0, 3), K=mult4(), act=acts(family), lay=dict(b=pick("v", "u", None)))

        @stratum("fwd")
        def fwd_ring_grouped(wm=wm, family=family):         # more than 4 MB of weights, a narrower last group
            return dict(entry="fwd", M=between(1, 64) if wm == 1 else between(65, 128), N=between(1025, 1088), K=1024,
                        act=acts(family), lay=dict(b=pick("v", None)))

    for kind in (None, 0, 1):
        @stratum("bwd_input")
        def bwd_input_ring(wm=wm, kind=kind):
            M, K = tile_shape(wm)
            return dict(entry="bwd_input", M=M, N=any_size(), K=K, act=acts(kind or 0),
                        lay=dict(yp=None if kind is None else "v"))

        for slabs in (0, 1):
            @stratum("bwd")
            def bwd_pair(wm=wm, kind=kind, slabs=slabs):
                N, K = tile_shape(wm)
                dw, db = gradient_outputs()
                return dict(entry="bwd", M=between(600, 3000) if slabs else between(1, 256), N=N, K=K,
                            act=acts(kind or 0), deferred=rng.random() < 0.3,
                            lay=dict(yp=None if kind is None else "v", dw=dw, db=db))

    for slabs in (0, 1):
        @stratum("bwd_weight")
        def bwd_weight_ring(wm=wm, slabs=slabs):
            N, K = tile_shape(wm)
            dw, db = gradient_outputs()
            return dict(entry="bwd_weight", M=between(600, 3000) if slabs else between(1, 256), N=N, K=K,
                        deferred=rng.random() < 0.3, lay=dict(dw=dw, db=db))

for va in (0, 1):
    for vb in (0, 1):
        for tn in (1, 2):
            for slabs in (0, 1):
                @stratum("bwd_weight")
                def bwd_weight_staged(va=va, vb=vb, tn=tn, slabs=slabs):
                    # 128 x 128 tiles (tn 2) take more than 512 tiles of 128 x 64: 17 x 17 x 2 in one slab, or 4 x 8 in
                    # 17 slabs of 512 rows; both operands with 16-byte rows reach this kernel when K % 4 != 0
                    if tn == 1:
                        M, N, K = (between(600, 3000) if slabs else between(1, 400)), any_size(), any_size()
                    elif slabs:
                        M, N, K = between(8193, 8704), between(385, 512), between(452, 512)   # (8 whole 64-column tiles)
                    else:
                        M, N, K = between(1, 100), between(2049, 2100), between(2049, 2100)
                    if va and vb and K % 4 == 0:
                        K -= between(1, 3)
                    if K < 1:
                        K = 1
                    dw, db = gradient_outputs()
                    return dict(entry="bwd_weight", M=M, N=N, K=K, deferred=rng.random() < 0.3,
                                lay=dict(dz=rows_operand(va), x=rows_operand(vb), dw=dw, db=db))

for entry in ("bwd_weight", "bwd"):
    for vec in (0, 1):
        for merged in (0, 1):
            for deferred in (0, 1):
                @stratum(entry)
                def reductions(entry=entry, vec=vec, merged=merged, deferred=deferred):
                    N, K = (mult4(4, 128), mult4(4, 128)) if merged else (any_size(), mult4(4, 128))
                    return dict(entry=entry, M=pick(between(1, 32), between(300, 1500), between(1500, 4000)), N=N, K=K,
                                deferred=bool(deferred),
                                lay=dict(dw="v" if vec else "u", db="behind" if merged else pick("sep", None)))


@stratum("bwd")
def one_workgroup_per_tile_pair():
    return dict(entry="bwd", M=between(1, 128), N=mult4(4, 64), K=mult4(4, 64), act=gc.ACT_TANH, lay=dict(yp="v"))


@stratum("bwd")
def separate_products():          # what the pair launch refuses runs as the two separate calls
    lay = pick(dict(dx=pick("o", "u")), dict(w="u"), dict(yp=pick("o", "u")), dict(dz=pick("o", "u")), dict(x=pick("o", "u")))
    return dict(entry="bwd", M=any_size(600), N=any_size(), K=mult4(), act=acts(pick(0, 1)), lay=lay)


@stratum("mse")
def mse_small():
    return dict(entry="mse", M=any_size(600), N=any_size(), K=mult4(), lay=dict(b=pick("v", "u", None), t=pick("v", "o", "u")))


# more than 512 tiles: a workgroup of the ring kernel walks on to a second one
SECOND_TILE = {
    "fwd": [lambda: dict(entry="fwd", M=between(8193, 8300), N=512, K=mult4(4, 16), act=acts(0))],
    "mse": [lambda: dict(entry="mse", M=between(22017, 22100), N=187, K=4)],
    "bwd_input": [lambda: dict(entry="bwd_input", M=between(8193, 8300), N=any_size(8), K=512, act=gc.ACT_RELU, lay=dict(yp="v")),
                  lambda: dict(entry="bwd_input", M=between(8193, 8300), N=any_size(8), K=512)],
    "bwd_weight": [lambda: dict(entry="bwd_weight", M=between(1, 64), N=2112, K=2048, lay=dict(db=None))],
    "bwd": [lambda: dict(entry="bwd", M=between(8193, 8300), N=any_size(8), K=512, lay=dict(db=None))],
}
for entry, draws in SECOND_TILE.items():
    for k, fn in enumerate(draws):
        fn.__name__ = "second_tile" + ("_%d" % k if k else "")
        STRATA[entry].append(fn)

# A case calls every entry point once, each from the next stratum of its own queue: every stratum twice, then random
# ones again.  (Fewer cases than twice the longest list of strata leave cells empty, and the run says so.)
queues = {}
for entry in gc.ENTRIES:
    q = STRATA[entry] * 2
    while len(q) < n_cases:
        q.append(STRATA[entry][int(rng.integers(0, len(STRATA[entry])))])
    queues[entry] = q

worst = collections.defaultdict(float)
cells = collections.Counter()
calls = 0
for case_no in range(n_cases):
    for entry in gc.ENTRIES:
        draw = queues[entry][case_no]
        spec = draw()
        name = "seed{}_case{:03d}_{}_{}".format(seed, case_no, entry, draw.__name__)
        case = gc.C(name, entry, spec["M"], spec["N"], spec["K"], [], act=spec.get("act", gc.ACT_NONE),
                    deferred=bool(spec.get("deferred", False)), **spec.get("lay", {}))
        calls += 1
        res = run_case(case, dev, ops)
        cells.update(gc.cells(res.plan))
        for key, (kernel, cpu) in res.figures.items():
            bound = 1.0
            if kernel >= 1.0 and cpu >= 1.0 and key in PINNED.get(name, {}):
                bound = PINNED[name][key]
                print("held to the pinned bound: {} {}: error / bound {:.3f} (float32 torch {:.3f}, pinned {:.3f})".format(
                    name, key, kernel, cpu, bound))
            else:
                worst[entry + " " + key] = max(worst[entry + " " + key], kernel)
            if not kernel < bound:
                print("FAILED {} {}: error / bound {:.3f} (float32 torch on the CPU: {:.3f}); M {} N {} K {} act {} {} plan {}"
                      .format(name, key, kernel, cpu, case.M, case.N, case.K, case.act, case.lay, res.plan))
                sys.exit(1)
torch.cuda.synchronize()
want = [cell for cell in gc.universe() if gc.unreachable(cell) is None]
print("coverage (calls per cell of tests/gemm_cases.py):")
for cell in want:
    print("  {:>4}  {}".format(cells[cell], cell))
stray = [cell for cell in cells if cell not in want]
print("cases", n_cases, "calls", calls, "strata", {e: len(STRATA[e]) for e in gc.ENTRIES})
print("worst error as a fraction of its bound:", {k: round(v, 3) for k, v in sorted(worst.items())})
thin = [cell for cell in want if cells[cell] < 2]
if thin or stray:
    print("coverage too thin:", thin, "cells outside the table:", stray)
    sys.exit(1)

