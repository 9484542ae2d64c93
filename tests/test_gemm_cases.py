"""tests/gemm_cases.py against itself (no GPU): the rows name every variant the dense dispatch can produce, the
variants nobody can reach are listed with their reason, and the rows stay small."""
import gemm_cases as gc


def test_every_variant_the_dispatch_can_produce_has_a_row_or_a_reason():
    universe = gc.universe()
    assert len(universe) == len(set(universe))
    named = set()
    for c in gc.CASES:
        named.update(gc.cells(c.expect))
    stray = sorted(named - set(universe), key=repr)
    assert not stray, ("rows name variants the dispatch code does not have", stray)
    for cell in universe:
        why = gc.unreachable(cell)
        if why is None:
            assert cell in named, ("no row lands on", cell)
        else:
            assert cell not in named, ("a row claims a variant listed as unreachable", cell, why)
    # the example of the kind: the staged kernel's MSE epilogue
    assert gc.unreachable(("staged", 1, 1, "mse", 1, 1, 1, 1, 0, 0, 0)) is not None


def test_rows_are_well_formed():
    names = [c.name for c in gc.CASES]
    assert len(names) == len(set(names))
    for c in gc.CASES:
        assert c.entry in gc.ENTRIES and c.M >= 1 and c.N >= 1 and c.K >= 1 and c.expect, c.name
        gemms = [e for e in c.expect if not isinstance(e, gc.Reduce)]
        reds = [e for e in c.expect if isinstance(e, gc.Reduce)]
        assert len(gemms) == (2 if c.entry == "bwd" and not isinstance(c.expect[0], gc.Pair) else 1), c.name
        if c.entry in ("bwd_weight", "bwd"):
            assert len(reds) in (1, 2) and all(r.deferred == int(c.deferred) for r in reds), c.name
            slabs = {e.splitk for e in gemms if isinstance(e, gc.Pair) or not e.a_row} | {r.slabs for r in reds}
            assert len(slabs) == 1, (c.name, "the reductions sum the slabs the product wrote")
        else:
            assert not reds and not c.deferred, c.name
        if c.entry == "mse":      # itts_linear_fwd_mse refuses anything else
            assert c.lay["x"] == c.lay["w"] == c.lay["g"] == "v" and c.K % 4 == 0, c.name


def test_what_the_issue_asks_each_to_be_reached_by_some_row():
    lays = [c.lay for c in gc.CASES]
    assert any(c.entry == "fwd" and c.lay["b"] is None for c in gc.CASES)                 # bias=None
    assert any(c.entry == "mse" and c.lay["b"] is None for c in gc.CASES)
    assert any("db" in lay and lay["db"] is None for lay in lays)                           # want_bias=False / db=None
    assert any(c.entry == "bwd" and c.lay["yp"] is None for c in gc.CASES)                  # yprev=None
    assert any(c.entry == "bwd_input" and c.lay["yp"] is None for c in gc.CASES)
    # a float4 straddling N under wide stores
    assert any(isinstance(c.expect[0], gc.Staged) and c.expect[0].wide and c.entry == "fwd" and c.N % 4 for c in gc.CASES)
    # both activation families wherever the family is a template parameter
    for kind, epi in ((gc.Staged, "bias_act"), (gc.Staged, "dact"), (gc.Ring, "bias_act"), (gc.Ring, "dact")):
        fams = {e.family for c in gc.CASES for e in c.expect if isinstance(e, kind) and e.epi == epi}
        assert fams == {0, 1}, (kind.__name__, epi)
    assert {e.family_x for c in gc.CASES for e in c.expect if isinstance(e, gc.Pair) and e.epi_x == "dact"} == {0, 1}


def test_rows_stay_small():
    for c in gc.CASES:
        largest = max(gc.operand_bytes(c).values())
        why = [reason for part, reason in gc.LARGE.items() if part in c.name]
        if why:
            assert largest <= 40 << 20, (c.name, largest)
        else:
            assert largest <= gc.MAX_OPERAND_BYTES, (c.name, largest)
