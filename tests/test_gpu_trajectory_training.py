"""Trajectory training from AcousticModelTrainer (hparams.trajectory_training) on the GPU, on the fixture of
tests/test_gpu_trainer.py: utterances of about 1 000 .. 1 900 frames, so every adjoint call runs on the stream form.
Initial weights and the pred_acoustic_features route are those of the frame-level model; the parameter gradients of one
batch equal those of the same chain with the layer's gradient composed from the forward solve and torch window ops
(tests/mlpg_adjoint_long_spec.py: composed_gradient); three epochs lower the loss and resume; checkpoints go both ways."""
import os

import numpy as np
import pytest
import scipy.io.wavfile
import torch

import mlpg_adjoint_long_spec as long_spec
from fixture_dirs import materialise
from idiaptts_amd.src.model_trainers.AcousticModelTrainer import AcousticModelTrainer

pytestmark = pytest.mark.gpu
LOSS = "MSELoss_trajectory"


@pytest.fixture(scope="module")
def fixture(golden_dir, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("trajectory_fixture"))
    ids, wdir, qdir, g = materialise(golden_dir, root)
    return root, ids, wdir, qdir, g


def _hparams(root, wdir, name, trajectory=True, seed=1):
    """the hparams of tests/test_gpu_trainer.py, plus the switch"""
    hp = AcousticModelTrainer.create_hparams()
    hp.num_questions = 409
    hp.voice = "full"
    hp.out_dir = os.path.join(root, name)
    hp.frame_size_ms = 5
    hp.num_coded_sps = 20
    hp.seed = seed
    hp.epochs = 3
    hp.use_gpu = True
    hp.dataset_num_workers_gpu = 0
    hp.model_type = "RNNDYN-1_RELU_32-1_FC_67"
    hp.batch_size_train = 2
    hp.batch_size_val = 50
    hp.use_saved_learning_rate = True
    hp.optimiser_args["lr"] = 0.001
    hp.model_name = "test_model"
    hp.epochs_per_checkpoint = 2
    hp.world_dir = wdir
    hp.use_best_as_final_model = False
    hp.trajectory_training = trajectory
    return hp


def _trainer(fixture, hp):
    root, ids, wdir, qdir, g = fixture
    trainer = AcousticModelTrainer(**AcousticModelTrainer.legacy_support_init(wdir, qdir, ids, hp.num_questions, hp))
    trainer.init(hp)
    return trainer


def _nn_dir(hp):
    return os.path.join(hp.out_dir, hp.model_name, hp.networks_dir)


def test_init_with_the_switch_leaves_weights_and_benchmark_alone(gpu, fixture):
    hp_frame = _hparams(fixture[0], fixture[2], "init_frame", trajectory=False)
    frame = _trainer(fixture, hp_frame)
    hp = _hparams(fixture[0], fixture[2], "init_trajectory")
    trainer = _trainer(fixture, hp)
    ours, theirs = dict(trainer.model_handler.model.named_parameters()), dict(frame.model_handler.model.named_parameters())
    assert list(ours) == list(theirs) and len(ours) == 4
    for key in ours:
        assert ours[key].is_cuda and torch.equal(ours[key], theirs[key]), key
    assert [loss.name for loss in trainer.loss_modules] == [LOSS]
    assert sorted(os.listdir(_nn_dir(hp))) == ["config.json", "params_e0"]
    # the model directory is that of the frame-level model: same config.json, the head is not part of it
    assert open(os.path.join(_nn_dir(hp), "config.json")).read() == \
        open(os.path.join(_nn_dir(hp_frame), "config.json")).read()
    assert len(trainer.model_handler.model._forward_hooks) == 1 and not frame.model_handler.model._forward_hooks
    scores = trainer.benchmark(hp)
    np.testing.assert_almost_equal((8.616, 78.4, 0.609, 37.352), scores["pred_acoustic_features"], 3)


def test_parameter_gradients_of_one_batch_equal_the_composed_chain(gpu, fixture, monkeypatch):
    from idiaptts_amd import ops
    hp = _hparams(fixture[0], fixture[2], "one_batch")
    trainer = _trainer(fixture, hp)
    handler = trainer.model_handler
    handler.set_dataset(hp, trainer.dataset_train, trainer.dataset_val, trainer.batch_collate_fn)
    batch, lengths = next(iter(handler.dataloader_train))
    n_frames = [int(n) for n in lengths["acoustic_features"]]
    assert len(n_frames) == 2 and min(n_frames) >= 194
    params = dict(handler.model.named_parameters())
    real_adjoint, forms, composed_calls = ops.mlpg_adjoint, [], []

    def recording(*args, **kwargs):
        out = real_adjoint(*args, **kwargs)
        forms.append(ops.mlpg_adjoint_last_form())
        return out

    def composed(gout, variances, dim, offsets, gcol0=0, out=None, col0=0, plan=None):
        grad = long_spec.composed_gradient(gout[:, gcol0:gcol0 + dim], [(0, dim, variances)], offsets, 3 * dim)
        out[:, col0:col0 + 3 * dim] = grad.to(out.dtype)
        composed_calls.append((dim, ops.mlpg_adjoint_last_form()))
        return out

    def gradients(adjoint):
        monkeypatch.setattr(ops, "mlpg_adjoint", adjoint)
        data = handler._to_device({k: v.clone() if torch.is_tensor(v) else v for k, v in batch.items()}, handler._device())
        max_lengths = {k: int(lengths[k].max()) for k in data if k in lengths}
        handler.model.zero_grad()
        handler.model.train()
        handler.model.init_hidden(len(n_frames))
        handler.model(data, lengths, max_lengths)
        loss = trainer.loss_modules[0](data, lengths, 0)[LOSS]
        loss.backward()
        return float(loss.detach()), {k: p.grad.detach().double().cpu().numpy().copy() for k, p in params.items()}

    loss, got = gradients(recording)
    assert forms == [ops.MLPG_STREAM] * 3          # coded sp, lf0, bap: one adjoint call each
    ref_loss, ref = gradients(composed)
    assert [d for d, _ in composed_calls] == [20, 1, 1] and len(forms) == 3          # no adjoint kernel ran in between
    assert np.isfinite(loss) and loss == ref_loss          # (the forward is the same code)
    for key in params:
        err = np.linalg.norm(got[key] - ref[key]) / np.linalg.norm(ref[key])
        print(key, "relative gradient error", err)
        assert np.linalg.norm(ref[key]) > 0 and err < 1e-5, (key, err)


def test_three_epochs_lower_the_trajectory_loss_and_a_resumed_run_goes_on(gpu, fixture):
    hp = _hparams(fixture[0], fixture[2], "train", seed=1234)
    trainer = _trainer(fixture, hp)
    val, train, handler = trainer.train(hp)
    assert list(train) == [LOSS] and list(val) == [LOSS]
    print("train", train[LOSS], "validation", val[LOSS])
    assert np.isfinite(train[LOSS]).all() and np.isfinite(val[LOSS]).all() and len(train[LOSS]) == 3
    assert train[LOSS][-1] < train[LOSS][0]
    assert {"config.json", "params_e2", "params_e3", "optimiser_e3"} <= set(os.listdir(_nn_dir(hp)))
    hp2 = _hparams(fixture[0], fixture[2], "train", seed=1234)
    hp2.load_checkpoint_epoch = 3
    hp2.epochs = 1
    trainer2 = _trainer(fixture, hp2)
    assert (trainer2.total_epoch, trainer2.total_steps) == (3, trainer.total_steps)
    _, train2, _ = trainer2.train(hp2)
    assert trainer2.total_epoch == 4 and trainer2.total_steps > trainer.total_steps
    assert np.isfinite(train2[LOSS]).all() and train2[LOSS][-1] < train[LOSS][-1]


def test_checkpoints_go_both_ways(gpu, fixture):
    root, ids = fixture[0], fixture[1]
    # frame-level pre-training, then the trajectory model from its second epoch
    hp = _hparams(root, fixture[2], "both_ways_frame", trajectory=False, seed=1234)
    hp.epochs = 2
    _trainer(fixture, hp).train(hp)
    saved = torch.load(os.path.join(_nn_dir(hp), "params_e2"), map_location="cpu", weights_only=False)["params"]
    hp2 = _hparams(root, fixture[2], "both_ways_frame", seed=1234)
    hp2.load_checkpoint_epoch = 2
    hp2.epochs = 1
    fine_tune = _trainer(fixture, hp2)
    state = fine_tune.model_handler.model.state_dict()
    assert list(state) == list(saved) and fine_tune.total_epoch == 2
    for key in saved:
        assert torch.equal(state[key].cpu(), saved[key]), key
    _, train, _ = fine_tune.train(hp2)          # and it trains on the trajectory from there
    assert list(train) == [LOSS] and np.isfinite(train[LOSS]).all()
    assert "params_e3" in os.listdir(_nn_dir(hp2))
    # the checkpoint trajectory training wrote, without the switch
    hp3 = _hparams(root, fixture[2], "both_ways_frame", trajectory=False, seed=1234)
    hp3.load_checkpoint_epoch = 3
    hp3.synth_fs = 16000
    plain = _trainer(fixture, hp3)
    written = torch.load(os.path.join(_nn_dir(hp3), "params_e3"), map_location="cpu", weights_only=False)["params"]
    state = plain.model_handler.model.state_dict()
    assert list(state) == list(written) and not plain.model_handler.model._forward_hooks
    for key in written:
        assert torch.equal(state[key].cpu(), written[key]), key
    assert [loss.name for loss in plain.loss_modules] == ["MSELoss_acoustic_features"]
    outputs, outputs_post = plain.synth(hp3, ids[:2])
    synth_dir = os.path.join(hp3.out_dir, hp3.model_name, "synth", "e3")
    for i in ids[:2]:
        post = outputs_post[i]["pred_acoustic_features"]
        assert post.shape == (len(outputs[i]["pred_acoustic_features"]), 23)
        fs, wav = scipy.io.wavfile.read(os.path.join(synth_dir, i + "_20mcep_WORLD.wav"))
        assert fs == 16000 and len(wav) == len(post) * 80
