"""GPU parity: HIP MLPG (through the C ABI) vs the C oracle (oracle/c/mlpg.c)."""
import numpy as np
import pytest
import torch
from mlpg_forms import FORCED, check_form

pytestmark = pytest.mark.gpu


SOLVES = ["auto", "stream", "ring", "ring-wide", "ring-plain"]


class Solve(object):
    """ops.mlpg_generation under one forced form; every call checks the form it recorded (tests/mlpg_forms.py)."""

    def __init__(self, name):
        self.name = name

    def __call__(self, feat, var, dim, offsets, **kw):
        from idiaptts_amd import ops
        out = ops.mlpg_generation(feat, var, dim, list(offsets), **kw)
        lengths = np.diff(np.asarray(offsets, dtype=np.int64))
        self.form = check_form(self.name, lengths, dim, feat.dtype == torch.float32)
        return out


@pytest.fixture(params=SOLVES)
def solve(request):
    """The library picks between its solves by batch shape (sequential sweeps under 194 frames; above that the
    one-pass ring kernel from 128 (utterance, 64-dimension) units, reduce -> scan -> solve below; in the ring, two
    dimensions a lane for float32 rows from 1 024 units and non-temporal float64 loads up to 192 MiB of rows): these
    tests run under its own choice and with the stream form, the narrow and the wide ring, and the narrow ring with
    plain float64 loads forced through ops.mlpg_forced (itts_mlpg_set_override, read at every call).  Each call
    asserts the form it recorded (ops.mlpg_last_form), so a forced form that is not taken fails."""
    from idiaptts_amd import ops
    with ops.mlpg_forced(**FORCED[request.param]):
        yield Solve(request.param)


def _case(rng, lengths, dim, extra_cols=0, col0=0):
    T = int(sum(lengths))
    feat = rng.normal(size=(T, col0 + 3 * dim + extra_cols))
    var = rng.uniform(0.01, 1.0, size=3 * dim)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return feat, var, offsets


@pytest.mark.parametrize("lengths,dim,col0", [
    ([1], 3, 0), ([2], 3, 0), ([3, 1, 2], 5, 0), ([4, 7, 300], 60, 0), ([1931], 20, 0),
    ([50, 0, 75], 1, 2), ([640, 1300], 62, 1),
    # time-parallel path: utterance lengths around the 64-frame chunk boundaries, mixed with short ones
    ([194, 195, 257, 258, 259, 130, 66, 3, 1, 322], 4, 0), ([193, 2], 2, 0), ([4098], 1, 0),
    # ring kernel: around its 24-frame segments, the five segments under the staged factor rows, the 288-frame ring
    ([200, 23, 24, 25, 47, 48, 49, 119, 120, 121, 143, 144, 145], 62, 0), ([287, 288, 289, 311, 312, 313, 575, 576, 577], 7, 0),
    ([2000, 600, 601], 64, 1),
])
def test_mlpg_matches_oracle(gpu, solve, lengths, dim, col0):
    """The solves the library holds -- the sequential sweeps for batches whose longest utterance is
    under 194 frames, the one-pass ring kernel or reduce -> scan -> solve otherwise -- against the C oracle."""
    from oracle import capi
    rng = np.random.default_rng(7)
    feat, var, offsets = _case(rng, lengths, dim, extra_cols=2, col0=col0)
    out = solve(torch.from_numpy(feat).to(gpu), torch.from_numpy(var).to(gpu), dim, offsets, col0=col0).cpu().numpy()
    for u in range(len(lengths)):
        a, b = offsets[u], offsets[u + 1]
        if b == a:
            continue
        ref = capi.mlpg(feat[a:b], var, dim, col0=col0)
        err = np.abs(out[a:b] - ref).max()
        rmse = np.sqrt(np.mean((out[a:b] - ref) ** 2))
        assert rmse <= 1e-10 and err <= 1e-9, (u, err, rmse)  # north-star bar: 1e-4 RMSE


def test_mlpg_full_size_property(gpu, solve):
    """BASELINE config 4 shape (187-dim cmp, 256 utterances): P x = b must hold to fp64
    round-off for the solution returned, checked through the normal equations on a sample."""
    rng = np.random.default_rng(11)
    lengths = rng.integers(400, 2000, size=256)
    dim = 60
    feat, var, offsets = _case(rng, lengths, dim)
    x = solve(torch.from_numpy(feat).to(gpu), torch.from_numpy(var).to(gpu), dim, offsets).cpu().numpy()
    assert np.isfinite(x).all()
    for u in (0, 100, 255):
        a, b = offsets[u], offsets[u + 1]
        T = b - a
        for d in (0, 31, 59):
            tau = np.zeros((T, 3))
            for w in range(3):
                tau[:, w] = 1.0 / var[w * dim + d]
            tau[0, 1:] = tau[-1, 1:] = 1e-11
            m = feat[a:b, [d, dim + d, 2 * dim + d]]
            xs = x[a:b, d]
            # gradient of the quadratic form: sum_w W_w^T tau_w (W_w x - m_w) = 0
            xp = np.concatenate([[0.0], xs, [0.0]])
            w1x = 0.5 * (xp[2:] - xp[:-2])
            w2x = xp[2:] - 2 * xp[1:-1] + xp[:-2]
            r0 = tau[:, 0] * (xs - m[:, 0])
            r1 = tau[:, 1] * (w1x - m[:, 1])
            r2 = tau[:, 2] * (w2x - m[:, 2])
            r1p = np.concatenate([[0.0], r1, [0.0]])
            r2p = np.concatenate([[0.0], r2, [0.0]])
            g = r0 + 0.5 * (r1p[:-2] - r1p[2:]) + (r2p[:-2] - 2 * r2p[1:-1] + r2p[2:])
            scale = np.abs(tau[:, 0] * m[:, 0]).max() + 1.0
            assert np.abs(g).max() / scale < 1e-9


@pytest.mark.parametrize("lengths,ratio", [([700, 90, 333], 1e-6), ([700, 90, 333], 1e-3), ([3000, 260], 1e-7)])
def test_mlpg_slowly_settling_factor(gpu, solve, lengths, ratio):
    """Delta variances up to 1e7 times smaller than the static ones: the Cholesky factor needs hundreds
    of frames to become stationary, so most chunks of an utterance carry their own matrices (the scan
    kernel's single-chunk segments, and -- at 3 000 frames -- its sequential road, taken when there
    are more such chunks than the workgroup has waves)."""
    from oracle import capi
    rng = np.random.default_rng(3)
    dim = 3
    feat, var, offsets = _case(rng, lengths, dim)
    var[dim:] *= ratio
    out = solve(torch.from_numpy(feat).to(gpu), torch.from_numpy(var).to(gpu), dim, offsets).cpu().numpy()
    for u in range(len(lengths)):
        a, b = offsets[u], offsets[u + 1]
        ref = capi.mlpg(feat[a:b], var, dim)
        scale = max(1.0, np.abs(ref).max())
        assert np.abs(out[a:b] - ref).max() <= 1e-9 * scale, (u, np.abs(out[a:b] - ref).max())


def test_mlpg_more_than_64_dimensions_and_an_output_slice(gpu, solve):
    """Two 64-dimension blocks (dim = 70) and a result written into columns 3 .. 72 of a wider
    array whose other columns must stay untouched (the solve also parks b in those rows)."""
    from oracle import capi
    rng = np.random.default_rng(21)
    lengths, dim = [300, 17, 500], 70
    feat, var, offsets = _case(rng, lengths, dim)
    out = torch.full((int(offsets[-1]), dim + 5), -7.0, dtype=torch.float64, device=gpu)
    solve(torch.from_numpy(feat).to(gpu), torch.from_numpy(var).to(gpu), dim, offsets, out=out, ocol0=3)
    got = out.cpu().numpy()
    assert (got[:, :3] == -7.0).all() and (got[:, 3 + dim:] == -7.0).all()
    for u in range(len(lengths)):
        a, b = offsets[u], offsets[u + 1]
        ref = capi.mlpg(feat[a:b], var, dim)
        assert np.abs(got[a:b, 3:3 + dim] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("lengths,dim", [([300, 40, 1000], 62), ([250] * 130, 5), ([120, 60], 3)])
def test_mlpg_float32_rows(gpu, solve, lengths, dim):
    """float32 input rows (the acoustic model's output type; mlpg.py:119-121 assigns them into float64 arrays): the
    result is that of the widened rows, whichever solve takes the batch -- the one-pass kernel converts in its loads,
    the others read a widened copy."""
    from oracle import capi
    rng = np.random.default_rng(17)
    feat, var, offsets = _case(rng, lengths, dim, extra_cols=3, col0=2)
    feat32 = feat.astype(np.float32)
    wide = feat32.astype(np.float64)
    got = solve(torch.from_numpy(feat32).to(gpu), torch.from_numpy(var).to(gpu), dim, offsets, col0=2).cpu().numpy()
    form32 = solve.form
    same = solve(torch.from_numpy(wide).to(gpu), torch.from_numpy(var).to(gpu), dim, offsets, col0=2).cpu().numpy()
    assert form32 != solve.form
    assert np.array_equal(got, same)
    for u in (0, len(lengths) - 1):
        a, b = offsets[u], offsets[u + 1]
        ref = capi.mlpg(wide[a:b], var, dim, col0=2)
        assert np.abs(got[a:b] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())


def _forced_call(name, feat, var, dim, offsets, **kw):
    from idiaptts_amd import ops
    with ops.mlpg_forced(**FORCED[name]):
        out = ops.mlpg_generation(feat, var, dim, list(offsets), **kw).cpu().numpy()
        form = check_form(name, np.diff(offsets), dim, feat.dtype == torch.float32)
    return out, form


# (lengths, dim, col0) around the ring's segment / ring boundaries, one and two blocks, rows 8- but not 16-byte
# aligned (col0 odd)
BIT_CASES = (([700, 25, 24, 289, 1, 2, 600, 313], 62, 1), ([400, 333], 70, 0), ([2100], 2, 3))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_mlpg_wide_helpers(gpu, dtype):
    """The one-pass kernel's helpers with two dimensions a lane and two rows a memory instruction (the library takes
    them for float32 rows from 1 024 units; forced here): the same values as with one dimension a lane, bit for bit,
    on lengths around the segment / ring boundaries, 62 and 70 dimensions (one and two blocks), column offsets that
    leave the rows 8- but not 16-byte aligned."""
    from idiaptts_amd.ops import MLPG_WIDE
    rng = np.random.default_rng(29)
    for lengths, dim, col0 in BIT_CASES:
        feat, var, offsets = _case(rng, lengths, dim, extra_cols=1, col0=col0)
        f, v = torch.from_numpy(feat.astype(dtype)).to(gpu), torch.from_numpy(var).to(gpu)
        narrow, form_n = _forced_call("ring", f, v, dim, offsets, col0=col0)
        wide, form_w = _forced_call("ring-wide", f, v, dim, offsets, col0=col0)
        assert form_w & MLPG_WIDE and not form_n & MLPG_WIDE
        assert np.array_equal(narrow, wide), (lengths, dim)


def test_mlpg_nt_loads_equal_plain_loads(gpu):
    """The float64 ring with non-temporal input loads (what the library takes up to 192 MiB of rows, the benchmark's
    shape) and with plain loads (above that): the same values bit for bit."""
    from idiaptts_amd.ops import MLPG_NT_IN
    rng = np.random.default_rng(31)
    for lengths, dim, col0 in BIT_CASES + (([577, 288, 195, 194, 3, 0, 288], 65, 2),):
        feat, var, offsets = _case(rng, lengths, dim, extra_cols=1, col0=col0)
        f, v = torch.from_numpy(feat).to(gpu), torch.from_numpy(var).to(gpu)
        nt, form_nt = _forced_call("ring-nt", f, v, dim, offsets, col0=col0)
        plain, form_plain = _forced_call("ring-plain", f, v, dim, offsets, col0=col0)
        assert form_nt ^ form_plain == MLPG_NT_IN
        assert np.array_equal(nt, plain), (lengths, dim)


# the five instances of mlpg_ring_kernel: (forced form, float32 rows)
RING_INSTANCES = [("ring-nt", False), ("ring-plain", False), ("ring-wide", False), ("ring", True), ("ring-wide", True)]
# the ring's 24-frame segments, the five segments under the staged factor rows (120 / 144), the 288-frame ring and
# twice it, the 194-frame floor of the long-utterance forms, short and empty utterances, and runs of equal lengths
# (the launch table's counting sort keeps them in their own order)
RING_EDGE_LENGTHS = [23, 24, 25, 47, 48, 49, 119, 120, 121, 143, 144, 145, 287, 288, 289, 575, 576, 577, 194, 195,
                     1, 2, 3, 0, 288, 288, 2, 2, 195, 24, 0, 577, 288, 1]


@pytest.mark.parametrize("dim", [1, 2, 3, 62, 64, 65, 70, 129])
@pytest.mark.parametrize("instance", RING_INSTANCES, ids=lambda x: "%s-%s" % (x[0], "f32" if x[1] else "f64"))
def test_mlpg_ring_geometry(gpu, instance, dim):
    """Every instance of the one-pass kernel, forced, on a batch of all its edge lengths against the C oracle per
    utterance; input columns at offsets that leave the rows 4- or 8-byte but not 16-byte aligned (float32: col0 1 or
    2 of rows of a multiple of 4 values; float64: col0 1 or 3), output columns outside the slice untouched.  (Odd
    dimensions keep the narrow helpers under a forced wide: that is the form they must record.)"""
    from oracle import capi
    name, f32 = instance
    rng = np.random.default_rng(1000 + dim)
    lengths = [int(n) for n in rng.permutation(RING_EDGE_LENGTHS)]
    col0 = (1, 2)[dim % 2] if f32 else (1, 3)[dim % 2]
    extra = (-(col0 + 3 * dim)) % 4 + 4                # rows of a multiple of 4 values (16 bytes as float32)
    feat, var, offsets = _case(rng, lengths, dim, extra_cols=extra, col0=col0)
    if f32:
        feat = feat.astype(np.float32).astype(np.float64)
    T, ocol0 = int(offsets[-1]), 1
    out = torch.full((T, ocol0 + dim + 2), -3.25, dtype=torch.float64, device=gpu)
    rows = torch.from_numpy(feat.astype(np.float32) if f32 else feat).to(gpu)
    _forced_call(name, rows, torch.from_numpy(var).to(gpu), dim, offsets, col0=col0, out=out, ocol0=ocol0)
    got = out.cpu().numpy()
    assert (got[:, :ocol0] == -3.25).all() and (got[:, ocol0 + dim:] == -3.25).all(), "columns touched"
    for u in range(len(lengths)):
        a, b = offsets[u], offsets[u + 1]
        if b == a:
            continue
        ref = capi.mlpg(feat[a:b], var, dim, col0=col0)
        diff = got[a:b, ocol0:ocol0 + dim] - ref
        rmse, err = np.sqrt(np.mean(diff ** 2)), np.abs(diff).max() / max(1.0, np.abs(ref).max())
        assert rmse <= 1e-10 and err <= 1e-9, (name, f32, dim, u, lengths[u], err, rmse)


@pytest.mark.parametrize("dim", [1, 62, 65])
def test_mlpg_stream_chunk_edges(gpu, dim):
    """reduce -> scan -> solve, forced, at its chunk edges: 16-frame chunks, two a workgroup, on top of the 194-frame
    floor (the slowly settling factor's sequential road at 3 000 frames runs under the `solve` fixture)."""
    from oracle import capi
    rng = np.random.default_rng(41 + dim)
    lengths = [194 + k for k in (15, 16, 17, 31, 32, 33, 63, 64, 65)] + [194, 195, 5, 0, 1]
    feat, var, offsets = _case(rng, lengths, dim, extra_cols=1, col0=1)
    out, _ = _forced_call("stream", torch.from_numpy(feat).to(gpu), torch.from_numpy(var).to(gpu), dim, offsets,
                          col0=1)
    for u in range(len(lengths)):
        a, b = offsets[u], offsets[u + 1]
        if b == a:
            continue
        ref = capi.mlpg(feat[a:b], var, dim, col0=1)
        diff = out[a:b] - ref
        rmse, err = np.sqrt(np.mean(diff ** 2)), np.abs(diff).max() / max(1.0, np.abs(ref).max())
        assert rmse <= 1e-10 and err <= 1e-9, (dim, u, lengths[u], err, rmse)


def test_mlpg_ring_table_past_2_20_frames(gpu):
    """An utterance longer than 2^20 frames: the ring's launch table is then ordered by a comparison sort instead of
    the counting sort (mlpg_sorted_table), equal lengths still in their own order.  One dimension, ring forced."""
    from oracle import capi
    rng = np.random.default_rng(43)
    lengths, dim = [5, 300, (1 << 20) + 3, 194, 0, 300, 5], 1
    feat, var, offsets = _case(rng, lengths, dim)
    out, _ = _forced_call("ring", torch.from_numpy(feat).to(gpu), torch.from_numpy(var).to(gpu), dim, offsets)
    for u in range(len(lengths)):
        a, b = offsets[u], offsets[u + 1]
        if b == a:
            continue
        ref = capi.mlpg(feat[a:b], var, dim)
        diff = out[a:b] - ref
        rmse, err = np.sqrt(np.mean(diff ** 2)), np.abs(diff).max() / max(1.0, np.abs(ref).max())
        assert rmse <= 1e-10 and err <= 1e-9, (u, lengths[u], err, rmse)


def _bench_lengths(n_utts):
    from idiaptts_amd.bench_support import utterance_lengths
    return utterance_lengths(n_utts, seed=5)


@pytest.mark.parametrize("shape,f32,solve_code", [
    ("short", False, 1), ("few", False, 2), ("few", True, 2), ("bench", False, 3), ("bench", True, 3),
    ("over_192_mib", False, 3), ("many_f32", True, 3)])
def test_mlpg_library_choice_on_the_device(gpu, shape, f32, solve_code):
    """Under the library's own choice the form a call records is the one itts_mlpg_choose_form names (pinned on the
    CPU by tests/test_mlpg_dispatch.py), over the batch shapes that take each form: the benchmark's (256 x 62, ring
    with non-temporal float64 loads; float32: the narrow ring), more than 192 MiB of float64 rows (plain loads),
    1 024+ units of float32 rows (wide helpers).  A few utterances of each against the C oracle."""
    from idiaptts_amd import ops
    from idiaptts_amd.ops import MLPG_NT_IN, MLPG_RING, MLPG_WIDE
    from oracle import capi
    rng = np.random.default_rng(47)
    lengths = {"short": lambda: rng.integers(1, 194, size=40), "few": lambda: rng.integers(150, 2000, size=16),
               "bench": lambda: _bench_lengths(256), "over_192_mib": lambda: rng.integers(1600, 1700, size=256),
               "many_f32": lambda: rng.integers(100, 400, size=1100)}[shape]()
    dim = 62
    feat, var, offsets = _case(rng, lengths, dim)
    rows = feat.astype(np.float32) if f32 else feat
    with ops.mlpg_forced():
        out = ops.mlpg_generation(torch.from_numpy(rows).to(gpu), torch.from_numpy(var).to(gpu), dim,
                                  offsets.tolist()).cpu().numpy()
        form = ops.mlpg_last_form()
        assert form == ops.mlpg_choose_form(len(lengths), dim, int(lengths.max()), int(offsets[-1]), f32)
    assert form & 3 == solve_code, ops.mlpg_form_name(form)
    if shape in ("bench", "over_192_mib") and not f32:
        assert form == (MLPG_RING | MLPG_NT_IN if shape == "bench" else MLPG_RING), ops.mlpg_form_name(form)
    if shape in ("bench", "many_f32") and f32:
        assert bool(form & MLPG_WIDE) == (shape == "many_f32"), ops.mlpg_form_name(form)
    for u in sorted({0, len(lengths) // 2, len(lengths) - 1, int(np.argmax(lengths))}):
        a, b = offsets[u], offsets[u + 1]
        ref = capi.mlpg(rows[a:b].astype(np.float64), var, dim)
        diff = out[a:b] - ref
        rmse, err = np.sqrt(np.mean(diff ** 2)), np.abs(diff).max() / max(1.0, np.abs(ref).max())
        assert rmse <= 1e-10 and err <= 1e-9, (shape, f32, u, err, rmse)


def test_planned_calls_equal_plain_calls(gpu, solve):
    """ops.MlpgPlan (itts_mlpg_plan_create / itts_mlpg_generation_planned): the offsets' share of a call prepared
    once -- the same trajectories bit for bit and the same form, under every forced form, float64 and float32 rows,
    several streams on one plan (misc/mlpg.py:94-127 is called once per stream)."""
    from idiaptts_amd import ops
    g = torch.Generator().manual_seed(4)
    for n_utts, dim in ((3, 5), (300, 62), (1, 1)):
        lens = torch.randint(40, 400, (n_utts,), generator=g).tolist()
        off = [0]
        for n in lens:
            off.append(off[-1] + n)
        feat = torch.randn(off[-1], 3 * dim + 4, dtype=torch.float64, generator=g).to(gpu)
        var = (torch.rand(3 * dim, dtype=torch.float64, generator=g) + 0.05).to(gpu)
        plan = ops.MlpgPlan(off)
        for rows in (feat, feat.float()):
            for col0 in (0, 4):
                want = solve(rows, var, dim, off, col0=col0)
                got = ops.mlpg_generation(rows, var, dim, off, col0=col0, plan=plan)
                assert ops.mlpg_last_form() == solve.form
                assert torch.equal(want, got)
        plan.close()
    with pytest.raises(Exception):
        ops.MlpgPlan([0, 5, 3])
