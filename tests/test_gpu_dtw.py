"""ops.dtw_align (csrc/dtw.hip) and the DTW scores of Metrics against the float64 numpy restatement tests/dtw_spec.py.

Paths are compared for EQUALITY.  On continuous data that is a fair demand only where no choice of the recurrence hangs
on rounding, so every such case first asserts, on the CPU, that the smallest gap between a chosen predecessor and the
runner-up (dtw_spec.decision_margin, relative to the total cost) is above 1e-9; the seeds below were chosen with the
spec so that it holds.  Costs and scores: 2e-12 relative -- float64, at most D + L + 3 <= 8 322 roundings of 2^-53
each is 9.3e-13, and 2e-12 is twice that.  Exact ties are tested on small integers, where every sum is exact in any
order and the tie rule alone decides.

Inputs: independent randn frames for all but the long pair.  Among 4.15 M cells of independent frames the smallest gap
is about 5e-11 of the cost whatever the seed (seeds 0, 1, 2: 7.0e-11, 4.5e-12, 4.1e-11), so the long pair is what the
package aligns in practice: y holds the frames of x on a stretched time axis plus randn noise of 1e-3."""
import os

import numpy as np
import pytest
import torch

import dtw_spec

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
RTOL = 2e-12


def iid_pair(T1, T2, D, seed):
    """randn frames.  D == 1: y is moved up by 8, out of x's range -- on a line |a - b| + |b - c| = |a - c| for every
    b between a and c, so overlapping ranges give paths of mathematically EQUAL cost (margin 0.0 for every seed)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T1, D)), rng.standard_normal((T2, D)) + (8.0 if D == 1 else 0.0)


def warped_pair(T1, T2, D, seed, noise=1e-3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T1, D))
    idx = np.round(np.linspace(0, T1 - 1, T2)).astype(np.int64)
    return x, x[idx] + noise * rng.standard_normal((T2, D))


def plan():
    from idiaptts_amd import ops
    p = ops.dtw_plan(100, 100, 24)
    return p["col_block"], p["rows_per_pass"]


def align(xs, ys, band=None, dtype=torch.float64):
    from idiaptts_amd import ops
    cost, length, path = ops.dtw_align([torch.from_numpy(x).to("cuda", dtype) for x in xs], None,
                                       [torch.from_numpy(y).to("cuda", dtype) for y in ys], None, band=band)
    return cost.cpu().numpy(), length.cpu().numpy(), path.cpu().numpy()


def check_pairs(xs, ys, band=None, dtype=torch.float64, margin=True):
    """one dtw_align call for all pairs; every pair against the spec: equal path and length, cost to RTOL"""
    if dtype == torch.float32:
        xs = [x.astype(np.float32).astype(np.float64) for x in xs]
        ys = [y.astype(np.float32).astype(np.float64) for y in ys]
    if margin:
        for x, y in zip(xs, ys):
            assert dtw_spec.decision_margin(x, y, band) > MARGIN, (x.shape, y.shape)
    cost, length, path = align(xs, ys, band, dtype)
    for n, (x, y) in enumerate(zip(xs, ys)):
        ref_cost, ref_path = dtw_spec.dtw(x, y, band)
        assert length[n] == len(ref_path), (x.shape, y.shape)
        np.testing.assert_array_equal(path[n, :length[n]], ref_path)
        assert (path[n, length[n]:] == -1).all()
        if np.isfinite(ref_cost):
            assert abs(cost[n] - ref_cost) <= RTOL * ref_cost, (x.shape, y.shape, cost[n], ref_cost)
        else:
            assert cost[n] == np.inf
    return cost, length, path


def feature_tuple(sp, seed, n_bap=1):
    """(coded_sp with a bin 0, lf0, vuv, bap) around the aligned spectrum sp [T, D]"""
    rng = np.random.default_rng(seed)
    T = len(sp)
    return (np.concatenate([rng.standard_normal((T, 1)), sp], axis=1), 5.0 + 0.3 * rng.standard_normal(T),
            (rng.standard_normal(T) > -0.3).astype(np.float64), rng.standard_normal((T, n_bap)))


def assert_scores(got, ref):
    for g, r in zip(got, ref):
        assert abs(g - r) <= RTOL * abs(r), (got, ref)


# ---------------------------------------------------------------------------------------- paths on continuous data
def test_tile_edges(gpu):
    """every T1 around the rows of a pass against every T2 around the columns of a block, one ragged batch"""
    W, R = plan()
    t1s = [1, 2, 63, 64, 65, R - 1, R, R + 1, 2 * R + 3]
    t2s = [1, 2, W - 1, W, W + 1, 2 * W + 1]
    pairs = [iid_pair(T1, T2, 24, 1000 + 37 * a + b) for a, T1 in enumerate(t1s) for b, T2 in enumerate(t2s)]
    check_pairs([p[0] for p in pairs], [p[1] for p in pairs])


@pytest.mark.parametrize("D", [1, 24, 59, 60, 128])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_feature_widths(gpu, D, dtype):
    from idiaptts_amd.src.Metrics import Metrics
    W, R = plan()
    x, y = iid_pair(R + 1, W + 1, D, 2000 + D)
    check_pairs([x], [y], dtype=dtype)
    if dtype == torch.float64:
        n_bap = 1 if D != 60 else 3                                        # both forms of the BAP distortion
        org, out = feature_tuple(x, 1, n_bap), feature_tuple(y, 2, n_bap)
        assert_scores(Metrics.get_metrics_dtw(org, out), dtw_spec.scores(org, out))


@pytest.mark.parametrize("shape", [(3, 300), (300, 3)])
def test_very_unequal_lengths(gpu, shape):
    x, y = iid_pair(shape[0], shape[1], 24, 3000 + shape[0])
    check_pairs([x], [y])


def test_long_pair(gpu):
    from idiaptts_amd.src.Metrics import Metrics
    x, y = warped_pair(1977, 2100, 59, 4000)
    check_pairs([x], [y])
    org, out = feature_tuple(x, 1), feature_tuple(y, 2)
    assert_scores(Metrics.get_metrics_dtw(org, out), dtw_spec.scores(org, out))


# ------------------------------------------------------------------------------------------------------ exact ties
def test_exact_ties(gpu):
    rng = np.random.default_rng(5)
    x = rng.integers(-3, 4, size=(70, 1)).astype(np.float64)
    xs = [x, x, np.full((40, 1), 2.0), np.array([[1.0]])]
    ys = [x.copy(), np.repeat(x, 2, axis=0), np.full((150, 1), -1.0), rng.integers(-3, 4, size=(50, 1)).astype(np.float64)]
    cost, length, path = check_pairs(xs, ys, margin=False)
    assert cost[0] == 0.0 and length[0] == 70 and (path[0, :70, 0] == path[0, :70, 1]).all()
    assert cost[1] == 0.0 and length[1] == 140
    assert length[3] == 50 and (path[3, :50, 0] == 0).all()


# --------------------------------------------------------------------------------------------------------- batches
def ragged(B, seed):
    rng = np.random.default_rng(seed)
    return [iid_pair(int(rng.integers(1, 200)), int(rng.integers(1, 300)), 24, seed + 1 + b) for b in range(B)]


@pytest.mark.parametrize("B", [1, 3, 17])
def test_ragged_batches(gpu, B, monkeypatch):
    from idiaptts_amd import ops
    pairs = ragged(B, 6000 + B)
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    cost, length, path = check_pairs(xs, ys)
    if B == 17:
        c1, l1, p1 = align(xs[16:], ys[16:])                               # the same pair alone: the same bits
        assert c1[0].tobytes() == cost[16].tobytes() and l1[0] == length[16]
        np.testing.assert_array_equal(p1[0, :l1[0]], path[16, :l1[0]])
        t1, t2 = [len(x) for x in xs], [len(y) for y in ys]
        monkeypatch.setattr(ops, "DTW_WORKSPACE_CAP", 6 * max(t1) * max(t2))   # several workspace groups
        assert len(ops._dtw_groups(t1, t2, ops.DTW_WORKSPACE_CAP)) >= 2
        c2, l2, p2 = align(xs, ys)
        assert c2.tobytes() == cost.tobytes()
        np.testing.assert_array_equal(l2, length)
        np.testing.assert_array_equal(p2, path)


def test_padding_is_never_read(gpu):
    """NaN behind every length and in a frame around both operands: the results of the list form, the frame intact"""
    from idiaptts_amd import ops
    pairs = ragged(5, 7000)
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    cost, length, path = align(xs, ys)

    def framed(seqs):
        D, Tm = seqs[0].shape[1], max(len(s) for s in seqs)
        big = torch.full((len(seqs) + 2, Tm + 3, D + 5), float("nan"), dtype=torch.float64, device="cuda")
        inner = big[1:-1, 2:2 + Tm, 3:3 + D]
        for b, s in enumerate(seqs):
            inner[b, :len(s)] = torch.from_numpy(s).to("cuda")
        return big, inner

    bx, ix = framed(xs)
    by, iy = framed(ys)
    kx, ky = bx.clone(), by.clone()
    c2, l2, p2 = ops.dtw_align(ix, [len(x) for x in xs], iy, [len(y) for y in ys])
    assert c2.cpu().numpy().tobytes() == cost.tobytes()
    np.testing.assert_array_equal(l2.cpu().numpy(), length)
    np.testing.assert_array_equal(p2.cpu().numpy(), path)
    for now, before in ((bx, kx), (by, ky)):
        assert torch.equal(torch.isnan(now), torch.isnan(before))
        assert torch.equal(torch.nan_to_num(now), torch.nan_to_num(before))


# ------------------------------------------------------------------------------------------------------------ band
@pytest.mark.parametrize("r", [0, 5, 50])
def test_band(gpu, r):
    a, b = iid_pair(200, 150, 24, 8000 + r), iid_pair(150, 200, 24, 8100 + r)
    cost, length, _ = check_pairs([a[0], b[0]], [a[1], b[1]], band=r)
    assert np.isfinite(cost[0])
    if r == 0:                                                             # 150 rows cannot reach 200 columns in steps of 1
        assert cost[1] == np.inf and length[1] == 0


def test_band_wider_than_the_grid_is_no_band(gpu):
    pairs = ragged(4, 9000)
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    free, wide = align(xs, ys), align(xs, ys, band=5000)
    assert free[0].tobytes() == wide[0].tobytes()
    np.testing.assert_array_equal(free[1], wide[1])
    np.testing.assert_array_equal(free[2], wide[2])


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_value():
    """(host tensors: a refusal comes before anything looks for a device)"""
    from idiaptts_amd import ops
    z = torch.zeros
    with pytest.raises(ValueError, match="T1 = 0"):
        ops.dtw_align(z(1, 4, 3), [0], z(1, 4, 3), [4])
    with pytest.raises(ValueError, match="T2 = 4097"):
        ops.dtw_align([z(5, 3)], None, [z(4097, 3)], None)
    with pytest.raises(ValueError, match="D = 129"):
        ops.dtw_align([z(5, 129)], None, [z(5, 129)], None)
    with pytest.raises(ValueError, match=r"y_lens\[1\] = 9 is longer than the buffer's 8"):
        ops.dtw_align(z(2, 8, 3), [8, 8], z(2, 8, 3), [8, 9])
    with pytest.raises(ValueError, match="x has D = 3, y has D = 4"):
        ops.dtw_align([z(5, 3)], None, [z(5, 4)], None)
    with pytest.raises(ValueError, match="T1 = 4097"):
        ops.dtw_plan(4097, 5, 3)


# --------------------------------------------------------------------------------------------------------- metrics
def golden_tuple(golden_dir, name):
    from idiaptts_amd.src.data_preparation.world.WorldFeatLabelGen import WorldFeatLabelGen
    cmp_ = np.fromfile(os.path.join(golden_dir, name + ".cmp"), dtype=np.float32).reshape(-1, 67)
    return WorldFeatLabelGen.convert_to_world_features(cmp_, contains_deltas=True, num_coded_sps=20, num_bap=1)


def resampled(feats, factor):
    """the tuple on a time axis of `factor` times its length (np.interp per column; V/UV thresholded again)"""
    T = len(feats[0])
    t_new = np.linspace(0, T - 1, int(round(factor * T)))
    cols = [np.asarray(f, dtype=np.float64).reshape(T, -1) for f in feats]
    out = [np.stack([np.interp(t_new, np.arange(T), c[:, k]) for k in range(c.shape[1])], axis=1) for c in cols]
    return out[0], out[1][:, 0], (out[2][:, 0] >= 0.5).astype(np.float64), out[3]


def test_metrics_against_itself_and_doubled(gpu, golden_dir):
    from idiaptts_amd.src.Metrics import Metrics
    org = golden_tuple(golden_dir, "LJ001-0008")
    T = len(org[0])
    assert Metrics.get_metrics_dtw(org, org) == [0.0, 0.0, 0.0, 0.0]
    path, cost = Metrics.dtw_path(org[0], org[0])
    assert cost == 0.0 and len(path) == T
    doubled = tuple(np.repeat(np.asarray(f), 2, axis=0) for f in org)
    assert Metrics.get_metrics_dtw(org, doubled) == [0.0, 0.0, 0.0, 0.0]
    path, cost = Metrics.dtw_path(org[0], doubled[0])
    assert cost == 0.0 and len(path) == 2 * T


def test_metrics_on_golden_features(gpu, golden_dir):
    from idiaptts_amd.src.Metrics import Metrics
    orgs = [golden_tuple(golden_dir, "LJ001-0008"), golden_tuple(golden_dir, "LJ001-0002")]
    outs = [resampled(orgs[0], 0.9), orgs[0]]
    singles = [Metrics.get_metrics_dtw(o, p) for o, p in zip(orgs, outs)]
    for got, o, p in zip(singles, orgs, outs):
        assert_scores(got, dtw_spec.scores(o, p))
    batch = Metrics.get_metrics_dtw_batch(orgs, outs)
    assert batch.shape == (2, 4)
    assert batch.tobytes() == np.array(singles, dtype=np.float64).tobytes()


def test_compare_wav_lists_against_themselves(gpu, golden_dir):
    from idiaptts_amd.src.Metrics import Metrics
    from idiaptts_amd.src.data_preparation.audio.AudioProcessing import AudioProcessing
    from idiaptts_amd.src.model_trainers.AcousticModelTrainer import AcousticModelTrainer
    files = [os.path.join(golden_dir, n + ".wav") for n in ("LJ001-0002", "LJ001-0008")]
    hp = AcousticModelTrainer.create_hparams()
    hp.synth_fs = AudioProcessing.read_wav(files[0])[1]
    hp.num_coded_sps = 20
    hp.frame_size_ms = 5
    scores = Metrics.compare_wav_lists(files, files, hp)
    assert scores.shape == (2, 4) and (scores == 0.0).all()


def test_compute_score_dtw_equals_the_batch_scorer(gpu, golden_dir, tmp_path):
    import logging
    from fixture_dirs import materialise
    from idiaptts_amd.src.Metrics import Metrics
    from idiaptts_amd.src.data_preparation.world.WorldFeatLabelGen import WorldFeatLabelGen
    from idiaptts_amd.src.model_trainers.AcousticModelTrainer import AcousticModelTrainer
    ids, wdir, _, g = materialise(golden_dir, str(tmp_path))
    hp = AcousticModelTrainer.create_hparams()
    hp.num_coded_sps = 20
    hp.world_dir = wdir
    hp.add_hparam("metrics_alignment", "dtw")
    trainer = AcousticModelTrainer.__new__(AcousticModelTrainer)
    trainer.logger = logging.getLogger("test_dtw")
    orgs, outs, data = [], [], {}
    for n, i in enumerate(ids[:3]):
        org = WorldFeatLabelGen.convert_to_world_features(np.asarray(g["cmp/" + i], dtype=np.float32),
                                                          contains_deltas=True, num_coded_sps=20, num_bap=1)
        out = resampled(org, 0.8 + 0.15 * n)
        orgs.append(tuple(np.asarray(f) for f in org))
        outs.append(out)
        data[i] = {"pred_acoustic_features": WorldFeatLabelGen.convert_from_world_features(*out).astype(np.float32)}
    got = trainer.compute_score(data, None, hp)["pred_acoustic_features"]
    outs32 = [WorldFeatLabelGen.convert_to_world_features(data[i]["pred_acoustic_features"], contains_deltas=False,
                                                          num_coded_sps=20, num_bap=1) for i in ids[:3]]
    want = Metrics.get_metrics_dtw_batch(orgs, outs32).mean(axis=0)
    np.testing.assert_array_equal(np.array(got), want)
