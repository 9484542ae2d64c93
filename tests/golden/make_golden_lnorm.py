"""Reference captures for LayerNorm layer groups (reference rnn_dyn/FFWrapper.py: `getattr(torch.nn, "LayerNorm")(**kwargs)`
behind its generic path, followed by the group's non-linearity), run on the CPU against the reference package with the
stub harness of make_golden.py.  Writes tests/golden/lnorm_fixture.npz:

  module cases  <case>/sd/<key>, <case>/modules, <case>/len, <case>/y, <case>/loss, <case>/grad/<param>,
                <case>/grad_x -- a reference RNNDyn built under torch.manual_seed, the names and torch.nn types of its
                layer-group modules ("2.module.0:LayerNorm"), a zero-padded batch of unequal lengths, its output, a
                masked MSE (sum of squared differences over the valid frames / (frames * features)) and the gradients.
                The input batch and the target are not stored: `case_inputs` draws them from a seeded CPU generator
                (the tests call it too);
  trainer case  trainer/init/<key>, trainer/final/<key>, trainer/val_losses, trainer/train_losses -- the reference
                AcousticModelTrainer on the trainer fixture data (seed 1234, 3 epochs, batch_first) with the new-style
                model_config of lnorm_cases.TRAINER_GROUPS.

Usage: python tests/golden/make_golden_lnorm.py (needs the reference checkout; data only is stored)."""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
from lnorm_cases import CASES, case_config, case_inputs, masked_mse, trainer_model_config  # noqa: E402


def module_types(model):
    """'<group>.module.<k>:<torch.nn class>' of every module inside the layer groups' nn.Sequential (a recurrent
    group's `module` is the cell itself and has no children)"""
    return np.array(["{}:{}".format(k, type(m).__name__) for k, m in model.named_modules() if ".module." in k])


def capture_modules(out):
    import torch
    from idiaptts.src.neural_networks.pytorch.models.rnn_dyn.Config import Config
    from idiaptts.src.neural_networks.pytorch.models.rnn_dyn.RNNDyn import RNNDyn
    for index, case in enumerate(CASES):
        name, _, in_dim, bf, seed, lens, scale = case[:7]
        torch.manual_seed(seed)
        model = RNNDyn(case_config(Config, case))
        lens_t = torch.tensor(lens)
        T, B = max(lens), len(lens)
        model.init_hidden(B)
        with torch.no_grad():
            y_shape = model(torch.zeros((B, T, in_dim) if bf else (T, B, in_dim)), seq_lengths_input=lens_t,
                            max_length_inputs=torch.tensor(T))[0].shape
        x, tgt = case_inputs(torch, index, in_dim, bf, lens, y_shape, scale)
        x.requires_grad_(True)
        model.init_hidden(B)
        y, _ = model(x, seq_lengths_input=lens_t, max_length_inputs=torch.tensor(T))
        loss = masked_mse(torch, y, tgt, lens_t, bf)
        loss.backward()
        p = name + "/"
        for k, v in model.state_dict().items():
            out[p + "sd/" + k] = v.detach().numpy().copy()
        for k, prm in model.named_parameters():
            if prm.grad is not None:
                out[p + "grad/" + k] = prm.grad.numpy().copy()
        out[p + "modules"] = module_types(model)
        out[p + "len"], out[p + "y"], out[p + "loss"] = np.asarray(lens), y.detach().numpy(), loss.detach().numpy()
        out[p + "grad_x"] = x.grad.numpy()
        print(name, tuple(y.shape), float(loss), list(out[p + "modules"]))


def capture_trainer(out):
    from idiaptts.src.model_trainers.AcousticModelTrainer import AcousticModelTrainer
    from idiaptts.src.neural_networks.pytorch.models import rnn_dyn
    from idiaptts.src.neural_networks.pytorch.models.NamedForwardWrapper import NamedForwardWrapper
    os.chdir(os.path.join(mg.REF, "test"))
    with open(os.path.join("integration", "fixtures", "database", "file_id_list.txt")) as f:
        id_list = [s.strip() for s in f.readlines()]
    out_dir = "/tmp/idiaptts_amd_golden_lnorm_train"
    hp = mg._ref_hparams(AcousticModelTrainer, out_dir)
    hp.batch_first = True
    hp.seed = 1234
    hp.use_best_as_final_model = False
    trainer = AcousticModelTrainer(**AcousticModelTrainer.legacy_support_init(
        hp.world_dir, os.path.join("integration", "fixtures", "questions"), id_list, hp.num_questions, hp))
    trainer.init(hp, model_config=trainer_model_config(rnn_dyn, NamedForwardWrapper, name_lists=False))
    for k, v in trainer.model_handler.model.state_dict().items():
        out["trainer/init/" + k] = np.array(v.cpu().numpy(), copy=True)
    out["trainer/modules"] = module_types(trainer.model_handler.model)
    all_loss, all_loss_train, _ = trainer.train(hp)
    key = "MSELoss_acoustic_features"
    out["trainer/val_losses"] = np.asarray(all_loss[key], dtype=np.float64)
    out["trainer/train_losses"] = np.asarray(all_loss_train[key], dtype=np.float64)
    for k, v in trainer.model_handler.model.state_dict().items():
        out["trainer/final/" + k] = v.cpu().numpy()
    print("reference lnorm trainer losses: val", out["trainer/val_losses"], "train", out["trainer/train_losses"])
    print(list(out["trainer/modules"]))
    shutil.rmtree(out_dir, ignore_errors=True)


def _main():
    mg.install_stub_harness()
    out = {}
    capture_modules(out)
    capture_trainer(out)
    path = os.path.join(HERE, "lnorm_fixture.npz")
    np.savez_compressed(path, **out)
    print("lnorm_fixture.npz:", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    _main()
