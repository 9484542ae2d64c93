"""Reference capture for vanilla RNN layer groups (reference rnn_dyn/RNNWrapper.py: torch.nn.RNN behind the legacy
`..RNNTANH..` / `..RNNRELU..` group names), run on the CPU against the reference package with the stub harness of
make_golden.py.  Writes tests/golden/rnn_vanilla_fixture.npz:

  trainer/init/<key>, trainer/final/<key>, trainer/val_losses, trainer/train_losses -- the reference
  AcousticModelTrainer on the trainer fixture data (seed 1234, 3 epochs, batch size 2, Adam 1e-3, batch_first: the
  recipe of make_golden_lnorm.py's trainer case) with model_type MODEL_TYPE.

Usage: python tests/golden/make_golden_rnn_vanilla.py (needs the reference checkout; data only is stored)."""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

MODEL_TYPE = "RNNDYN-1_TANH_32-1_BiRNNTANH_16-1_FC_67"


def capture_trainer(out):
    from idiaptts.src.model_trainers.AcousticModelTrainer import AcousticModelTrainer
    os.chdir(os.path.join(mg.REF, "test"))
    with open(os.path.join("integration", "fixtures", "database", "file_id_list.txt")) as f:
        id_list = [s.strip() for s in f.readlines()]
    out_dir = "/tmp/idiaptts_amd_golden_rnn_vanilla_train"
    hp = mg._ref_hparams(AcousticModelTrainer, out_dir)
    hp.model_type = MODEL_TYPE
    hp.batch_first = True
    hp.seed = 1234
    hp.use_best_as_final_model = False
    trainer = AcousticModelTrainer(**AcousticModelTrainer.legacy_support_init(
        hp.world_dir, os.path.join("integration", "fixtures", "questions"), id_list, hp.num_questions, hp))
    trainer.init(hp)
    for k, v in trainer.model_handler.model.state_dict().items():
        out["trainer/init/" + k] = np.array(v.cpu().numpy(), copy=True)
    all_loss, all_loss_train, _ = trainer.train(hp)
    key = "MSELoss_acoustic_features"
    out["trainer/val_losses"] = np.asarray(all_loss[key], dtype=np.float64)
    out["trainer/train_losses"] = np.asarray(all_loss_train[key], dtype=np.float64)
    for k, v in trainer.model_handler.model.state_dict().items():
        out["trainer/final/" + k] = v.cpu().numpy()
    print("reference vanilla RNN trainer losses: val", out["trainer/val_losses"], "train", out["trainer/train_losses"])
    shutil.rmtree(out_dir, ignore_errors=True)


def _main():
    mg.install_stub_harness()
    out = {}
    capture_trainer(out)
    path = os.path.join(HERE, "rnn_vanilla_fixture.npz")
    np.savez_compressed(path, **out)
    print("rnn_vanilla_fixture.npz:", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    _main()
