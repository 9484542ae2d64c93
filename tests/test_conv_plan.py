"""itts_conv1d_plan / ops.conv1d_plan (no device work, so no GPU): the plans that the fixed cases of
tests/test_gpu_conv1d.py state by hand (tests/conv_harness.py: CASES) are the library's, those cases between them reach
what they name, and geometries the products reject have no plan."""
import pytest

from conv_harness import CASES, expected_vec
from conv_ref import SHAPES, out_len, same_pad
from idiaptts_amd import ops


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hand_written_plans_are_the_librarys(case):
    g = case.geo
    for product in range(3):
        for vec in (True, False):          # no tile or split depends on the loads today
            assert ops.conv1d_plan(product, g.B, g.T, g.Cin, g.Cout, g.Kw, g.pad, g.dil, vec) == case.plan[product]


def test_small_shapes_take_the_64_wide_tile_in_one_slab():
    """what the older value checks of test_gpu_conv1d.py reach"""
    for B, T, Cin, Cout, Kw, dil, pad in SHAPES:
        for product in range(3):
            tile, slabs, kchunk = ops.conv1d_plan(product, B, T, Cin, Cout, Kw, same_pad(pad, Kw, dil), dil)
            assert (tile, slabs) == (64, 1) and kchunk % 32 == 0


def test_cases_cover_what_they_name():
    """both tile widths of every product with and without 16-byte loads, weight gradients over many slabs on both
    tile widths, a short last slab, both layouts"""
    seen = set()
    for c in CASES:
        g = c.geo
        rows = g.B * out_len(g.T, g.Kw, g.pad, g.dil)
        for product, (tile, slabs, kchunk) in enumerate(c.plan):
            seen.add((product, tile, expected_vec(g)[product]))
            if slabs > 1:
                seen.add(("slabs", tile))
                assert product == 2 and kchunk % 32 == 0 and (slabs - 1) * kchunk < rows <= slabs * kchunk
                if rows % kchunk:
                    seen.add("short last slab")
        seen.add("batch_first" if g.bf else "time-major")
    assert {(p, t, v) for p in range(3) for t in (64, 128) for v in (True, False)} <= seen, sorted(map(str, seen))
    assert {("slabs", 64), ("slabs", 128), "short last slab", "batch_first", "time-major"} <= seen


def test_rejected_geometries_have_no_plan():
    for args in [(0, 2, 4, 3, 5, 5, 0, 1), (1, 2, 4, 3, 5, 3, 0, 2), (2, 2, 4, 3, 5, 5, 0, 1),     # T_out <= 0
                 (3, 2, 40, 3, 5, 3, 1, 1), (-1, 2, 40, 3, 5, 3, 1, 1),                             # unknown product
                 (0, 0, 40, 3, 5, 3, 1, 1), (0, 2, 40, 0, 5, 3, 1, 1), (0, 2, 40, 3, 5, 0, 1, 1),
                 (0, 2, 40, 3, 5, 3, -1, 1), (0, 2, 40, 3, 5, 3, 1, 0),
                 (0, 1 << 16, 1 << 16, 3, 5, 3, 1, 1)]:                                              # 2^32 rows
        with pytest.raises(ValueError):
            ops.conv1d_plan(*args)
