"""The dense fp32 GEMM variants (csrc/nn.hip, gemm_staged.h, gemm_ring.h) as a table: every row names an entry point,
the smallest shape and buffer layout that lands on one variant, and -- as literal values, worked out by hand from
the rules in nn.hip, not computed here -- what ops.gemm_last_plan() must report for it.  tests/test_gemm_cases.py
checks the table against the list of variants the dispatch code can produce (no GPU); tests/test_gpu_gemm_variants.py
runs every row; scripts/gemm_fuzz.py tallies its random cases in the same cells.  No torch in this file.

Layouts.  A row-major operand [rows, W] is the column slice [:, off:off + W] of a wider buffer (tests/gemm_harness.py):
  "v"  pitch pad4(W) + 8 floats, off 4: a 16-byte pitch on a 16-byte base -> 16-byte loads / stores allowed
  "o"  pitch pad4(W) + 5 floats, off 4: the pitch is no multiple of 4 floats
  "u"  pitch pad4(W) + 8 floats, off 1: the base is 4 bytes off the 16-byte grid
Flat operands (w [N, K] contiguous, b [N], dw [N, K], db [N]) start 4 floats ("v") or 1 float ("u") into their
buffer.  db: "sep" a buffer of its own, "behind" right behind dw in dw's buffer (merged with dw's reduction where N
and N K are multiples of 4), None no bias gradient.  b / yp None: no bias / no previous activation."""
import collections

ACT_NONE, ACT_TANH, ACT_RELU, ACT_SIGMOID, ACT_SOFTSIGN, ACT_LEAKY_RELU = 0, 1, 2, 3, 6, 7

Staged = collections.namedtuple("Staged", "a_row b_row epi tn stages vec_a vec_b wide splitk family")
Ring = collections.namedtuple("Ring", "a_row b_row epi wm grouped splitk family second_tile")
Pair = collections.namedtuple("Pair", "wm_w splitk epi_x family_x second_tile")
Reduce = collections.namedtuple("Reduce", "vec merged deferred slabs")

Case = collections.namedtuple("Case", "name entry M N K lay act deferred expect")

ENTRIES = ("fwd", "mse", "bwd_input", "bwd_weight", "bwd")
_DEFAULT_LAY = {
    "fwd": dict(x="v", w="v", b="v", y="v"),
    "mse": dict(x="v", w="v", b="v", t="v", g="v"),
    "bwd_input": dict(dz="v", w="v", yp=None, dx="v"),
    "bwd_weight": dict(dz="v", x="v", dw="v", db="sep"),
    "bwd": dict(dz="v", x="v", w="v", yp=None, dx="v", dw="v", db="sep"),
}


def C(name, entry, M, N, K, expect, act=ACT_NONE, deferred=False, **lay):
    full = dict(_DEFAULT_LAY[entry])
    assert set(lay) <= set(full), (name, lay)
    full.update(lay)
    return Case(name, entry, M, N, K, full, act, deferred, list(expect))


def _slab_class(s):
    return "1" if s == 1 else ("2-4" if s <= 4 else ">4")


def cells(plan):
    """The cells a normalised plan (a list of Staged / Ring / Pair / Reduce) falls into"""
    out = []
    for e in plan:
        if isinstance(e, Staged):
            out.append(("staged", e.a_row, e.b_row, e.epi, e.tn, e.stages, e.vec_a, e.vec_b, e.wide, int(e.splitk > 1),
                        e.family))
        elif isinstance(e, Ring):
            out.append(("ring", e.a_row, e.b_row, e.epi, e.wm, e.grouped, int(e.splitk > 1), e.family))
            out.append(("ring walk", e.a_row, e.b_row, e.epi, e.second_tile))
        elif isinstance(e, Pair):
            out.append(("pair", e.wm_w, int(e.splitk > 1), e.epi_x, e.family_x))
            out.append(("pair walk", e.second_tile))
        else:
            out.append(("reduce", e.vec, e.merged, e.deferred))
            out.append(("reduce slabs", _slab_class(e.slabs)))
    return out


def universe():
    """Every cell the dispatch code of nn.hip can name, reachable or not: the template instantiations behind
    launch_gemm_tn / launch_ring_wm / launch_ring_bwd_pair crossed with the run-time branches (wide stores, grouped
    order, one slab or several, a second tile per workgroup), and the reduction forms of launch_reduce_slabs."""
    u = []
    row_products = [(1, "bias_act", 0), (1, "bias_act", 1), (0, "store", 0), (0, "dact", 0), (0, "dact", 1), (1, "mse", 0)]
    for b_row, epi, fam in row_products:            # launch_gemm_tn<true, B_ROW, EPI, 1, 1, AF>
        for va in (0, 1):
            for vb in (0, 1):
                for wide in (0, 1):
                    u.append(("staged", 1, b_row, epi, 1, 1, va, vb, wide, 0, fam))
    for tn in (1, 2):                               # launch_gemm_tn<false, false, EPI_STORE, TN, 2>
        for va in (0, 1):
            for vb in (0, 1):
                for split in (0, 1):
                    u.append(("staged", 0, 0, "store", tn, 2, va, vb, 0, split, 0))
    for wm in (1, 2):
        for grouped in (0, 1):
            for fam in (0, 1):
                u.append(("ring", 1, 1, "bias_act", wm, grouped, 0, fam))
        u.append(("ring", 1, 0, "store", wm, 0, 0, 0))
        u.append(("ring", 1, 0, "dact", wm, 0, 0, 0))
        u.append(("ring", 1, 0, "dact", wm, 0, 0, 1))
        for split in (0, 1):
            u.append(("ring", 0, 0, "store", wm, 0, split, 0))
            for epi_x, fam in (("store", 0), ("dact", 0), ("dact", 1)):
                u.append(("pair", wm, split, epi_x, fam))
    u.append(("ring", 1, 1, "mse", 2, 0, 0, 0))
    for a_row, b_row, epi in ((1, 1, "bias_act"), (1, 1, "mse"), (1, 0, "store"), (1, 0, "dact"), (0, 0, "store")):
        for second in (0, 1):
            u.append(("ring walk", a_row, b_row, epi, second))
    u += [("pair walk", 0), ("pair walk", 1)]
    for vec in (0, 1):
        for merged in (0, 1):
            for deferred in (0, 1):
                u.append(("reduce", vec, merged, deferred))
    u += [("reduce slabs", c) for c in ("1", "2-4", ">4")]
    return u


def unreachable(cell):
    """Why no call can land in this cell (None: it can)"""
    if cell[0] == "staged" and cell[1] == 1:
        if cell[3] == "mse":
            return "itts_linear_fwd_mse requires 16-byte rows of x, w and dz, which is all the ring kernel asks for"
        if cell[6] and cell[7] and cell[8]:
            return ("16-byte loads of both operands and a 16-byte output (with its bias / yprev) is what ring_ok asks "
                    "for; it refuses such a call only from 2^30 rows on")
    return None


# ---------------------------------------------------------------------------------------------------------------------
# The rows.  Shapes of the row-form staged kernel walk M in {1, 127, 128, 129}, N in {1, 63, 64, 65}, K in
# {1, 31, 32, 33} (16-byte loads of w need K % 4 == 0: 32); an N with N % 4 != 0 under wide stores makes a float4
# straddle N.
TANH, RELU, SIG, SOFTSIGN, LEAKY = ACT_TANH, ACT_RELU, ACT_SIGMOID, ACT_SOFTSIGN, ACT_LEAKY_RELU
CASES = [
    # ---- forward, register-staged row form: load forms x wide stores x activation family
    C("fwd_staged_a0b0_base", "fwd", 1, 1, 1, [Staged(1, 1, 'bias_act', 1, 1, 0, 0, 0, 1, 0)], act=TANH, x='o', y='o'),
    C("fwd_staged_a0b0_ext", "fwd", 127, 63, 31, [Staged(1, 1, 'bias_act', 1, 1, 0, 0, 0, 1, 1)], act=SIG, x='o', y='o'),
    C("fwd_staged_a0b0_wide_base", "fwd", 128, 64, 33, [Staged(1, 1, 'bias_act', 1, 1, 0, 0, 1, 1, 0)], act=RELU, x='u'),
    C("fwd_staged_a0b0_wide_ext", "fwd", 129, 65, 1, [Staged(1, 1, 'bias_act', 1, 1, 0, 0, 1, 1, 1)], act=SOFTSIGN, x='u'),
    C("fwd_staged_a0b0_bias_off_base", "fwd", 1, 63, 31, [Staged(1, 1, 'bias_act', 1, 1, 0, 0, 0, 1, 0)], x='u', b='u'),
    C("fwd_staged_a0b0_bias_off_ext", "fwd", 127, 64, 33, [Staged(1, 1, 'bias_act', 1, 1, 0, 0, 0, 1, 1)], act=LEAKY, x='u', b='u'),
    C("fwd_staged_a1b0_base", "fwd", 128, 65, 1, [Staged(1, 1, 'bias_act', 1, 1, 1, 0, 0, 1, 0)], act=TANH, y='o'),
    C("fwd_staged_a1b0_ext", "fwd", 129, 1, 31, [Staged(1, 1, 'bias_act', 1, 1, 1, 0, 0, 1, 1)], act=SIG, y='o'),
    C("fwd_staged_a1b0_wide_base", "fwd", 1, 64, 33, [Staged(1, 1, 'bias_act', 1, 1, 1, 0, 1, 1, 0)], act=RELU, b=None),
    C("fwd_staged_a1b0_wide_ext", "fwd", 127, 65, 1, [Staged(1, 1, 'bias_act', 1, 1, 1, 0, 1, 1, 1)], act=SOFTSIGN, b=None),
    C("fwd_staged_a0b1_base", "fwd", 128, 1, 32, [Staged(1, 1, 'bias_act', 1, 1, 0, 1, 0, 1, 0)], x='o', y='u'),
    C("fwd_staged_a0b1_ext", "fwd", 129, 63, 32, [Staged(1, 1, 'bias_act', 1, 1, 0, 1, 0, 1, 1)], act=LEAKY, x='o', y='u'),
    C("fwd_staged_a0b1_wide_base", "fwd", 1, 65, 32, [Staged(1, 1, 'bias_act', 1, 1, 0, 1, 1, 1, 0)], act=TANH, x='u'),
    C("fwd_staged_a0b1_wide_ext", "fwd", 127, 1, 32, [Staged(1, 1, 'bias_act', 1, 1, 0, 1, 1, 1, 1)], act=SIG, x='u'),
    C("fwd_staged_a1b0_w_off_base", "fwd", 128, 63, 32, [Staged(1, 1, 'bias_act', 1, 1, 1, 0, 0, 1, 0)], act=RELU, w='u', y='o'),
    C("fwd_staged_a1b0_w_off_ext", "fwd", 129, 64, 32, [Staged(1, 1, 'bias_act', 1, 1, 1, 0, 0, 1, 1)], act=SOFTSIGN, w='u', y='o'),
    C("fwd_staged_a1b1_base", "fwd", 1, 1, 32, [Staged(1, 1, 'bias_act', 1, 1, 1, 1, 0, 1, 0)], y='o'),
    C("fwd_staged_a1b1_ext", "fwd", 127, 63, 32, [Staged(1, 1, 'bias_act', 1, 1, 1, 1, 0, 1, 1)], act=LEAKY, y='o'),
    C("fwd_staged_a1b0_w_off_wide_base", "fwd", 128, 64, 32, [Staged(1, 1, 'bias_act', 1, 1, 1, 0, 1, 1, 0)], act=TANH, w='u'),
    C("fwd_staged_a1b0_w_off_wide_ext", "fwd", 129, 65, 32, [Staged(1, 1, 'bias_act', 1, 1, 1, 0, 1, 1, 1)], act=SIG, w='u'),
    # ---- forward, ring: 128 x 64 (wm 2) and 64 x 128 (wm 1) tiles, grouped order (17 / 9 column tiles in groups of
    #      16 / 8: the last group holds one), a second tile per workgroup (513 row tiles x 4 column tiles)
    C("fwd_ring_wm2_base", "fwd", 128, 65, 36, [Ring(1, 1, 'bias_act', 2, 0, 1, 0, 0)], act=TANH),
    C("fwd_ring_wm2_ext", "fwd", 127, 63, 32, [Ring(1, 1, 'bias_act', 2, 0, 1, 1, 0)], act=SOFTSIGN, b=None),
    C("fwd_ring_wm1_base", "fwd", 1, 128, 4, [Ring(1, 1, 'bias_act', 1, 0, 1, 0, 0)], act=RELU),
    C("fwd_ring_wm1_ext", "fwd", 129, 65, 100, [Ring(1, 1, 'bias_act', 1, 0, 1, 1, 0)], act=SIG),
    C("fwd_ring_wm2_grouped_base", "fwd", 128, 1028, 1024, [Ring(1, 1, 'bias_act', 2, 1, 1, 0, 0)], act=TANH),
    C("fwd_ring_wm2_grouped_ext", "fwd", 65, 1025, 1024, [Ring(1, 1, 'bias_act', 2, 1, 1, 1, 0)], act=LEAKY),
    C("fwd_ring_wm1_grouped_base", "fwd", 64, 1028, 1024, [Ring(1, 1, 'bias_act', 1, 1, 1, 0, 0)]),
    C("fwd_ring_wm1_grouped_ext", "fwd", 63, 1025, 1024, [Ring(1, 1, 'bias_act', 1, 1, 1, 1, 0)], act=SIG, b=None),
    C("fwd_ring_second_tile", "fwd", 8193, 512, 4, [Ring(1, 1, 'bias_act', 1, 0, 1, 0, 1)], act=TANH),
    # ---- output layer fused with the masked MSE (always the ring kernel, 128 x 64 tiles)
    C("mse_one_tile", "mse", 1, 1, 4, [Ring(1, 1, 'mse', 2, 0, 1, 0, 0)]),
    C("mse_187", "mse", 129, 187, 36, [Ring(1, 1, 'mse', 2, 0, 1, 0, 0)], t='o'),
    C("mse_no_bias_target_off", "mse", 128, 65, 32, [Ring(1, 1, 'mse', 2, 0, 1, 0, 0)], b=None, t='u'),
    C("mse_second_tile", "mse", 22017, 187, 4, [Ring(1, 1, 'mse', 2, 0, 1, 0, 1)]),
    # ---- input gradient dx [M, K] = dz [M, N] w [N, K], register-staged row form
    C("bwd_input_staged_a0b0_store", "bwd_input", 1, 33, 63, [Staged(1, 0, 'store', 1, 1, 0, 0, 0, 1, 0)], dz='o', dx='o'),
    C("bwd_input_staged_a0b0_dact_base", "bwd_input", 127, 1, 66, [Staged(1, 0, 'dact', 1, 1, 0, 0, 0, 1, 0)], act=TANH, dz='o', yp='o', dx='o'),
    C("bwd_input_staged_a0b0_dact_ext", "bwd_input", 128, 31, 65, [Staged(1, 0, 'dact', 1, 1, 0, 0, 0, 1, 1)], act=SIG, dz='o', yp='o', dx='o'),
    C("bwd_input_staged_a0b0_wide_store", "bwd_input", 129, 33, 1, [Staged(1, 0, 'store', 1, 1, 0, 0, 1, 1, 0)], dz='u'),
    C("bwd_input_staged_a0b0_wide_dact_base", "bwd_input", 1, 1, 66, [Staged(1, 0, 'dact', 1, 1, 0, 0, 1, 1, 0)], act=RELU, dz='u', yp='v'),
    C("bwd_input_staged_a0b0_wide_dact_ext", "bwd_input", 127, 31, 65, [Staged(1, 0, 'dact', 1, 1, 0, 0, 1, 1, 1)], act=SOFTSIGN, dz='u', yp='v'),
    C("bwd_input_staged_a0b0_yprev_off_dact_base", "bwd_input", 129, 1, 63, [Staged(1, 0, 'dact', 1, 1, 0, 0, 0, 1, 0)], act=TANH, dz='u', yp='o'),
    C("bwd_input_staged_a0b0_yprev_off_dact_ext", "bwd_input", 1, 31, 65, [Staged(1, 0, 'dact', 1, 1, 0, 0, 0, 1, 1)], act=LEAKY, dz='u', yp='o'),
    C("bwd_input_staged_a1b0_store", "bwd_input", 127, 33, 1, [Staged(1, 0, 'store', 1, 1, 1, 0, 0, 1, 0)], dx='o'),
    C("bwd_input_staged_a1b0_dact_base", "bwd_input", 128, 1, 63, [Staged(1, 0, 'dact', 1, 1, 1, 0, 0, 1, 0)], act=RELU, yp='o', dx='o'),
    C("bwd_input_staged_a1b0_dact_ext", "bwd_input", 129, 31, 66, [Staged(1, 0, 'dact', 1, 1, 1, 0, 0, 1, 1)], act=SIG, yp='o', dx='o'),
    C("bwd_input_staged_a1b0_wide_store", "bwd_input", 1, 33, 1, [Staged(1, 0, 'store', 1, 1, 1, 0, 1, 1, 0)]),
    C("bwd_input_staged_a1b0_wide_dact_base", "bwd_input", 127, 1, 63, [Staged(1, 0, 'dact', 1, 1, 1, 0, 1, 1, 0)], act=TANH, yp='v'),
    C("bwd_input_staged_a1b0_wide_dact_ext", "bwd_input", 128, 31, 66, [Staged(1, 0, 'dact', 1, 1, 1, 0, 1, 1, 1)], act=SOFTSIGN, yp='v'),
    C("bwd_input_staged_a0b1_store", "bwd_input", 129, 65, 32, [Staged(1, 0, 'store', 1, 1, 0, 1, 0, 1, 0)], dz='o', dx='u'),
    C("bwd_input_staged_a0b1_dact_base", "bwd_input", 1, 63, 32, [Staged(1, 0, 'dact', 1, 1, 0, 1, 0, 1, 0)], act=RELU, dz='o', yp='u', dx='u'),
    C("bwd_input_staged_a0b1_dact_ext", "bwd_input", 127, 64, 32, [Staged(1, 0, 'dact', 1, 1, 0, 1, 0, 1, 1)], act=LEAKY, dz='o', yp='u', dx='u'),
    C("bwd_input_staged_a0b1_wide_store", "bwd_input", 128, 65, 64, [Staged(1, 0, 'store', 1, 1, 0, 1, 1, 1, 0)], dz='u'),
    C("bwd_input_staged_a0b1_wide_dact_base", "bwd_input", 129, 1, 64, [Staged(1, 0, 'dact', 1, 1, 0, 1, 1, 1, 0)], act=TANH, dz='u', yp='v'),
    C("bwd_input_staged_a0b1_wide_dact_ext", "bwd_input", 1, 64, 64, [Staged(1, 0, 'dact', 1, 1, 0, 1, 1, 1, 1)], act=SIG, dz='u', yp='v'),
    C("bwd_input_staged_a1b1_store", "bwd_input", 127, 65, 32, [Staged(1, 0, 'store', 1, 1, 1, 1, 0, 1, 0)], dx='o'),
    C("bwd_input_staged_a1b1_dact_base", "bwd_input", 128, 1, 32, [Staged(1, 0, 'dact', 1, 1, 1, 1, 0, 1, 0)], act=RELU, yp='o', dx='o'),
    C("bwd_input_staged_a1b1_dact_ext", "bwd_input", 129, 63, 32, [Staged(1, 0, 'dact', 1, 1, 1, 1, 0, 1, 1)], act=SOFTSIGN, yp='o', dx='o'),
    C("bwd_input_staged_a1b0_w_off_wide_store", "bwd_input", 1, 65, 64, [Staged(1, 0, 'store', 1, 1, 1, 0, 1, 1, 0)], w='u'),
    C("bwd_input_staged_a1b0_w_off_wide_dact_base", "bwd_input", 127, 1, 64, [Staged(1, 0, 'dact', 1, 1, 1, 0, 1, 1, 0)], act=TANH, w='u', yp='v'),
    C("bwd_input_staged_a1b0_w_off_wide_dact_ext", "bwd_input", 128, 63, 64, [Staged(1, 0, 'dact', 1, 1, 1, 0, 1, 1, 1)], act=LEAKY, w='u', yp='v'),
    # ---- input gradient, ring
    C("bwd_input_ring_wm2_store", "bwd_input", 128, 33, 68, [Ring(1, 0, 'store', 2, 0, 1, 0, 0)]),
    C("bwd_input_ring_wm1_store", "bwd_input", 1, 1, 128, [Ring(1, 0, 'store', 1, 0, 1, 0, 0)]),
    C("bwd_input_ring_wm2_dact_base", "bwd_input", 129, 63, 64, [Ring(1, 0, 'dact', 2, 0, 1, 0, 0)], act=TANH, yp='v'),
    C("bwd_input_ring_wm1_dact_base", "bwd_input", 63, 65, 68, [Ring(1, 0, 'dact', 1, 0, 1, 0, 0)], act=RELU, yp='v'),
    C("bwd_input_ring_wm2_dact_ext", "bwd_input", 128, 1, 36, [Ring(1, 0, 'dact', 2, 0, 1, 1, 0)], act=SIG, yp='v'),
    C("bwd_input_ring_wm1_dact_ext", "bwd_input", 63, 31, 100, [Ring(1, 0, 'dact', 1, 0, 1, 1, 0)], act=SOFTSIGN, yp='v'),
    C("bwd_input_ring_second_tile", "bwd_input", 8193, 5, 512, [Ring(1, 0, 'dact', 1, 0, 1, 0, 1)], act=TANH, yp='v'),
    C("bwd_input_ring_second_tile_store", "bwd_input", 8193, 3, 512, [Ring(1, 0, 'store', 1, 0, 1, 0, 1)]),
    # ---- weight gradient dw [N, K] = dz^T x, register-staged column form.  128 x 64 tiles (tn 1) unless the 128 x 128
    #      ones fill the 512 slots better: that takes more than 512 tiles of 128 x 64 -- 17 x 17 x 2 in one slab
    #      (2050 x 2052), or 4 x 8 x 17 slabs (512 x 512 from 8193 rows on: one slab per 512 rows)
    C("bwd_weight_staged_tn1_a0b0", "bwd_weight", 5, 7, 3, [Staged(0, 0, 'store', 1, 2, 0, 0, 0, 1, 0), Reduce(0, 0, 0, 1), Reduce(0, 0, 0, 1)], dz='o', x='u'),
    C("bwd_weight_staged_tn1_a0b0_slabs", "bwd_weight", 1025, 63, 65, [Staged(0, 0, 'store', 1, 2, 0, 0, 0, 3, 0), Reduce(0, 0, 0, 3)], dz='o', x='u', db=None),
    C("bwd_weight_staged_tn2_a0b0", "bwd_weight", 70, 2050, 2052, [Staged(0, 0, 'store', 2, 2, 0, 0, 0, 1, 0), Reduce(1, 0, 0, 1), Reduce(0, 0, 0, 1)], dz='o', x='u'),
    C("bwd_weight_staged_tn2_a0b0_slabs", "bwd_weight", 8193, 512, 512, [Staged(0, 0, 'store', 2, 2, 0, 0, 0, 17, 0), Reduce(1, 1, 0, 17)], dz='o', x='u', db='behind'),
    C("bwd_weight_staged_tn1_a1b0", "bwd_weight", 127, 65, 33, [Staged(0, 0, 'store', 1, 2, 1, 0, 0, 1, 0), Reduce(0, 0, 0, 1), Reduce(0, 0, 0, 1)], x='o'),
    C("bwd_weight_staged_tn1_a1b0_slabs", "bwd_weight", 1537, 187, 5, [Staged(0, 0, 'store', 1, 2, 1, 0, 0, 4, 0), Reduce(0, 0, 0, 4), Reduce(0, 0, 0, 4)], x='o'),
    C("bwd_weight_staged_tn2_a1b0", "bwd_weight", 69, 2050, 2052, [Staged(0, 0, 'store', 2, 2, 1, 0, 0, 1, 0), Reduce(1, 0, 0, 1)], x='o', db=None),
    C("bwd_weight_staged_tn2_a1b0_slabs", "bwd_weight", 8193, 512, 512, [Staged(0, 0, 'store', 2, 2, 1, 0, 0, 17, 0), Reduce(1, 0, 0, 17), Reduce(1, 0, 0, 17)], x='o'),
    C("bwd_weight_staged_tn1_a0b1", "bwd_weight", 33, 1, 129, [Staged(0, 0, 'store', 1, 2, 0, 1, 0, 1, 0), Reduce(0, 0, 0, 1), Reduce(0, 0, 0, 1)], dz='u'),
    C("bwd_weight_staged_tn1_a0b1_slabs", "bwd_weight", 2049, 64, 126, [Staged(0, 0, 'store', 1, 2, 0, 1, 0, 5, 0), Reduce(1, 1, 0, 5)], dz='u', db='behind'),
    C("bwd_weight_staged_tn2_a0b1", "bwd_weight", 68, 2050, 2052, [Staged(0, 0, 'store', 2, 2, 0, 1, 0, 1, 0), Reduce(1, 0, 0, 1), Reduce(0, 0, 0, 1)], dz='u', db='behind'),
    C("bwd_weight_staged_tn2_a0b1_slabs", "bwd_weight", 8193, 512, 512, [Staged(0, 0, 'store', 2, 2, 0, 1, 0, 17, 0), Reduce(1, 0, 0, 17)], dz='u', db=None),
    C("bwd_weight_staged_tn1_a1b1", "bwd_weight", 129, 64, 31, [Staged(0, 0, 'store', 1, 2, 1, 1, 0, 1, 0), Reduce(1, 0, 0, 1), Reduce(1, 0, 0, 1)]),
    C("bwd_weight_staged_tn1_a1b1_slabs", "bwd_weight", 2561, 130, 30, [Staged(0, 0, 'store', 1, 2, 1, 1, 0, 6, 0), Reduce(1, 0, 0, 6), Reduce(0, 0, 0, 6)]),
    C("bwd_weight_staged_tn2_a1b1", "bwd_weight", 67, 2050, 2050, [Staged(0, 0, 'store', 2, 2, 1, 1, 0, 1, 0), Reduce(1, 0, 0, 1), Reduce(0, 0, 0, 1)]),
    C("bwd_weight_staged_tn2_a1b1_slabs", "bwd_weight", 8193, 512, 510, [Staged(0, 0, 'store', 2, 2, 1, 1, 0, 17, 0), Reduce(1, 0, 0, 17), Reduce(1, 0, 0, 17)]),
    # ---- weight gradient, ring (16-byte rows of dz and x, K % 4 == 0)
    C("bwd_weight_ring_wm2", "bwd_weight", 33, 128, 64, [Ring(0, 0, 'store', 2, 0, 1, 0, 0), Reduce(1, 0, 0, 1), Reduce(1, 0, 0, 1)]),
    C("bwd_weight_ring_wm1", "bwd_weight", 1, 63, 128, [Ring(0, 0, 'store', 1, 0, 1, 0, 0), Reduce(1, 0, 0, 1)], db=None),
    C("bwd_weight_ring_wm2_slabs", "bwd_weight", 1025, 187, 36, [Ring(0, 0, 'store', 2, 0, 5, 0, 0), Reduce(1, 0, 0, 5), Reduce(0, 0, 0, 5)]),
    C("bwd_weight_ring_wm1_slabs", "bwd_weight", 3001, 63, 100, [Ring(0, 0, 'store', 1, 0, 12, 0, 0), Reduce(1, 0, 0, 12), Reduce(0, 0, 0, 12)], db='behind'),
    C("bwd_weight_ring_second_tile", "bwd_weight", 40, 2112, 2048, [Ring(0, 0, 'store', 1, 0, 1, 0, 1), Reduce(1, 0, 0, 1)], db=None),
    # ---- slab reductions: float4 / scalar columns, merged with the bias, deferred, 1 / 2-4 / more slabs
    C("reduce_merged", "bwd_weight", 700, 64, 96, [Ring(0, 0, 'store', 1, 0, 3, 0, 0), Reduce(1, 1, 0, 3)], db='behind'),
    C("reduce_merged_dw_off", "bwd_weight", 300, 4, 8, [Ring(0, 0, 'store', 2, 0, 2, 0, 0), Reduce(0, 1, 0, 2)], dw='u', db='behind'),
    C("reduce_scalar_bias_187", "bwd_weight", 300, 187, 64, [Ring(0, 0, 'store', 2, 0, 2, 0, 0), Reduce(1, 0, 0, 2), Reduce(0, 0, 0, 2)]),
    C("reduce_scalar_dw_off", "bwd_weight", 65, 8, 8, [Ring(0, 0, 'store', 2, 0, 1, 0, 0), Reduce(0, 0, 0, 1), Reduce(1, 0, 0, 1)], dw='u'),
    C("reduce_two_to_four_slabs", "bwd_weight", 600, 512, 512, [Ring(0, 0, 'store', 2, 0, 3, 0, 0), Reduce(1, 1, 0, 3)], db='behind'),
    C("reduce_deferred_merged", "bwd_weight", 700, 64, 96, [Ring(0, 0, 'store', 1, 0, 3, 0, 0), Reduce(1, 1, 1, 3)], deferred=True, db='behind'),
    C("reduce_deferred_vec_and_scalar", "bwd_weight", 3001, 187, 512, [Ring(0, 0, 'store', 1, 0, 12, 0, 0), Reduce(1, 0, 1, 12), Reduce(0, 0, 1, 12)], deferred=True),
    C("reduce_deferred_merged_dw_off", "bwd_weight", 300, 4, 8, [Ring(0, 0, 'store', 2, 0, 2, 0, 0), Reduce(0, 1, 1, 2)], deferred=True, dw='u', db='behind'),
    C("reduce_deferred_one_slab_no_bias", "bwd_weight", 5, 7, 3, [Staged(0, 0, 'store', 1, 2, 0, 1, 0, 1, 0), Reduce(0, 0, 1, 1)], deferred=True, dz='o', db=None),
    # ---- both gradients from one call: the pair launch (16-byte rows everywhere), else the two separate products
    C("bwd_pair_wm2_store", "bwd", 33, 128, 64, [Pair(2, 1, 'store', 0, 0), Reduce(1, 0, 0, 1), Reduce(1, 0, 0, 1)]),
    C("bwd_pair_wm1_store", "bwd", 1, 63, 128, [Pair(1, 1, 'store', 0, 0), Reduce(1, 0, 0, 1)], db=None),
    C("bwd_pair_wm2_dact_base", "bwd", 129, 65, 36, [Pair(2, 1, 'dact', 0, 0), Reduce(1, 0, 0, 1), Reduce(0, 0, 0, 1)], act=TANH, yp='v', db='behind'),
    C("bwd_pair_wm1_dact_base", "bwd", 127, 1, 128, [Pair(1, 1, 'dact', 0, 0), Reduce(1, 0, 0, 1), Reduce(0, 0, 0, 1)], act=RELU, yp='v'),
    C("bwd_pair_wm2_dact_ext", "bwd", 64, 128, 68, [Pair(2, 1, 'dact', 1, 0), Reduce(1, 0, 0, 1), Reduce(1, 0, 0, 1)], act=SIG, yp='v'),
    C("bwd_pair_wm1_dact_ext", "bwd", 65, 64, 100, [Pair(1, 1, 'dact', 1, 0), Reduce(1, 1, 0, 1)], act=SOFTSIGN, yp='v', db='behind'),
    C("bwd_pair_wm2_store_slabs", "bwd", 1025, 187, 36, [Pair(2, 5, 'store', 0, 0), Reduce(1, 0, 0, 5)], db=None),
    C("bwd_pair_wm1_store_slabs", "bwd", 777, 64, 100, [Pair(1, 4, 'store', 0, 0), Reduce(1, 1, 0, 4)], db='behind'),
    C("bwd_pair_wm1_dact_base_slabs", "bwd", 3001, 187, 512, [Pair(1, 12, 'dact', 0, 0), Reduce(1, 0, 0, 12), Reduce(0, 0, 0, 12)], act=TANH, yp='v', db='behind'),
    C("bwd_pair_wm2_dact_base_slabs", "bwd", 1030, 65, 100, [Pair(2, 5, 'dact', 0, 0), Reduce(1, 0, 0, 5), Reduce(0, 0, 0, 5)], act=RELU, yp='v'),
    C("bwd_pair_wm2_dact_ext_slabs", "bwd", 513, 250, 68, [Pair(2, 3, 'dact', 1, 0), Reduce(1, 0, 0, 3), Reduce(0, 0, 0, 3)], act=LEAKY, yp='v'),
    C("bwd_pair_wm1_dact_ext_slabs", "bwd", 600, 63, 128, [Pair(1, 3, 'dact', 1, 0), Reduce(1, 0, 1, 3), Reduce(0, 0, 1, 3)], act=SIG, deferred=True, yp='v'),
    C("bwd_pair_one_workgroup_per_tile", "bwd", 64, 64, 64, [Pair(2, 1, 'dact', 0, 0), Reduce(1, 0, 0, 1), Reduce(1, 0, 0, 1)], act=TANH, yp='v'),
    C("bwd_pair_second_tile", "bwd", 8193, 5, 512, [Pair(1, 33, 'dact', 0, 1), Reduce(1, 0, 0, 33)], act=RELU, yp='v', db=None),
    C("bwd_separate_odd_dx", "bwd", 129, 65, 36, [Ring(0, 0, 'store', 2, 0, 1, 0, 0), Reduce(1, 0, 0, 1), Reduce(0, 0, 0, 1), Staged(1, 0, 'dact', 1, 1, 1, 1, 0, 1, 0)], act=TANH, yp='o', dx='o', db='behind'),
    C("bwd_separate_w_off", "bwd", 127, 63, 32, [Ring(0, 0, 'store', 2, 0, 1, 0, 0), Reduce(1, 0, 0, 1), Reduce(0, 0, 0, 1), Staged(1, 0, 'store', 1, 1, 1, 0, 1, 1, 0)], w='u'),
]

BY_NAME = {c.name: c for c in CASES}
MAX_OPERAND_BYTES = 8 << 20
# rows that cannot be small, by a part of their name: why
LARGE = {"tn2": "the 128 x 128 column-form tile wins only above 512 tiles of 128 x 64 (19 MB of dw, or 8193 rows)",
         "grouped": "the grouped order starts above 4 MB of weights",
         "second_tile": "a workgroup meets a second tile only above 512 tiles of 32 KB of output"}


def pad4(n):
    return (n + 3) // 4 * 4


def pitch(width, lay):
    return pad4(width) + (5 if lay == "o" else 8)


def operand_bytes(c):
    """bytes of every buffer a row allocates, by operand"""
    M, N, K, lay = c.M, c.N, c.K, c.lay
    shapes = {"x": (M, K), "y": (M, N), "t": (M, N), "g": (M, N), "dz": (M, N), "yp": (M, K), "dx": (M, K)}
    out = {}
    for name, how in lay.items():
        if how is None:
            continue
        if name in shapes:
            out[name] = 4 * shapes[name][0] * pitch(shapes[name][1], how)
        else:
            out[name] = 4 * ({"w": N * K, "dw": N * K + N, "b": N, "db": N}[name] + 8)
    return out
