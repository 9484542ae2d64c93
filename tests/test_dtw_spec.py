"""The numpy restatement of the DTW (tests/dtw_spec.py) against an enumeration of every path, its tie rule and band, and
the host side of the DTW scores: AcousticModelTrainer.compute_score's metrics_alignment switch, compare_wav_lists'
refusal.  No GPU."""
import logging
import os

import numpy as np
import pytest

import dtw_spec


@pytest.mark.parametrize("D", [1, 3])
def test_spec_cost_is_the_minimum_over_every_path(D):
    rng = np.random.default_rng(11 + D)
    for T1 in range(1, 7):
        for T2 in range(1, 7):
            x, y = rng.standard_normal((T1, D)), rng.standard_normal((T2, D))
            cost, path = dtw_spec.dtw(x, y)
            best = dtw_spec.exhaustive_cost(x, y)
            assert abs(cost - best) <= 1e-14 * best, (T1, T2)
            d = dtw_spec.distances(x, y)
            assert abs(d[path[:, 0], path[:, 1]].sum() - cost) <= 1e-14 * cost
            assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (T1 - 1, T2 - 1)
            steps = np.diff(path, axis=0)
            assert set(map(tuple, steps)) <= {(1, 1), (1, 0), (0, 1)}


def test_spec_tie_rule_on_integers():
    """all distances equal (C(i, j) = max(i, j) + 1): diagonal steps from the end while both indices last, then the edge"""
    def const(T, v):
        return np.full((T, 1), float(v))
    cost, path = dtw_spec.dtw(const(3, 0), const(5, 1))
    assert cost == 5.0 and path.tolist() == [[0, 0], [0, 1], [0, 2], [1, 3], [2, 4]]
    cost, path = dtw_spec.dtw(const(5, 0), const(3, 1))
    assert cost == 5.0 and path.tolist() == [[0, 0], [1, 0], [2, 0], [3, 1], [4, 2]]
    cost, path = dtw_spec.dtw(const(4, 2), const(4, 2))
    assert cost == 0.0 and path.tolist() == [[0, 0], [1, 1], [2, 2], [3, 3]]


def test_spec_choices_follow_the_rule():
    """every choice of small-integer tables is the rule's: the diagonal on equal values, then (i-1, j), then (i, j-1);
    cells whose up and left are equal and below the diagonal occur among them"""
    rng = np.random.default_rng(0)
    seen = 0
    for _ in range(400):
        x = rng.integers(0, 3, size=(4, 1)).astype(np.float64)
        y = rng.integers(0, 3, size=(4, 1)).astype(np.float64)
        C, dec, _ = dtw_spec.fill(x, y)
        for i in range(1, 4):
            for j in range(1, 4):
                diag, up, left = C[i - 1, j - 1], C[i - 1, j], C[i, j - 1]
                want = 0 if diag <= up and diag <= left else 1 if up <= left else 2
                assert dec[i, j] == want
                seen += up == left < diag
    assert seen > 0


def test_band_admits_both_corners():
    for T1 in range(1, 41):
        for T2 in range(1, 41):
            assert dtw_spec.admissible(0, 0, T1, T2, 0)
            assert dtw_spec.admissible(T1 - 1, T2 - 1, T1, T2, 0)
            cost, path = dtw_spec.dtw(np.zeros((T1, 1)), np.ones((T2, 1)), band=max(T1, T2))
            assert cost == len(path)


def _trainer_and_data(golden_dir, root):
    from fixture_dirs import materialise
    from idiaptts_amd.src.data_preparation.world.WorldFeatLabelGen import WorldFeatLabelGen
    from idiaptts_amd.src.model_trainers.AcousticModelTrainer import AcousticModelTrainer
    ids, wdir, _, g = materialise(golden_dir, root)
    hp = AcousticModelTrainer.create_hparams()
    hp.num_coded_sps = 20
    hp.world_dir = wdir
    trainer = AcousticModelTrainer.__new__(AcousticModelTrainer)
    trainer.logger = logging.getLogger("test_dtw_spec")
    rng = np.random.default_rng(3)
    data, orgs, outs = {}, [], []
    for i in ids[:3]:
        org = WorldFeatLabelGen.convert_to_world_features(np.asarray(g["cmp/" + i], dtype=np.float32),
                                                          contains_deltas=True, num_coded_sps=20, num_bap=1)
        T = len(org[0]) - 7                                               # shorter than the original: truncation at work
        static = WorldFeatLabelGen.convert_from_world_features(*org)[:T]
        pred = (static + 0.1 * rng.standard_normal(static.shape)).astype(np.float32)
        data[i] = {"pred_acoustic_features": pred}
        orgs.append(org)
        outs.append(WorldFeatLabelGen.convert_to_world_features(pred, contains_deltas=False, num_coded_sps=20,
                                                                num_bap=1))
    return trainer, hp, data, orgs, outs


def test_compute_score_refuses_an_unknown_alignment(golden_dir, tmp_path):
    trainer, hp, data, _, _ = _trainer_and_data(golden_dir, str(tmp_path))
    hp.add_hparam("metrics_alignment", "nonsense")
    with pytest.raises(ValueError, match="nonsense"):
        trainer.compute_score(data, None, hp)


@pytest.mark.parametrize("explicit", [False, True])
def test_compute_score_truncate_is_get_metrics(golden_dir, tmp_path, explicit):
    from idiaptts_amd.src.Metrics import Metrics
    trainer, hp, data, orgs, outs = _trainer_and_data(golden_dir, str(tmp_path))
    if explicit:
        hp.add_hparam("metrics_alignment", "truncate")
    got = trainer.compute_score(data, None, hp)["pred_acoustic_features"]
    want = np.mean(np.array([Metrics.get_metrics(o, p) for o, p in zip(orgs, outs)], dtype=np.float64), axis=0)
    assert np.array(got).tobytes() == want.tobytes()
    assert np.isfinite(want).all()


def test_compare_wav_lists_refuses_another_rate_by_name(golden_dir):
    from idiaptts_amd.src.Metrics import Metrics
    from idiaptts_amd.src.data_preparation.audio.AudioProcessing import AudioProcessing
    from idiaptts_amd.src.model_trainers.AcousticModelTrainer import AcousticModelTrainer
    name = os.path.join(golden_dir, "LJ001-0002.wav")
    hp = AcousticModelTrainer.create_hparams()
    hp.synth_fs = AudioProcessing.read_wav(name)[1] + 1
    with pytest.raises(ValueError, match="LJ001-0002.wav"):
        Metrics.compare_wav_lists([name], [name], hp)
