"""Reference capture for utterance and frame classification: reference RNNDyn classifiers under the reference's
NamedLoss(type_="CrossEntropyLoss", squeeze_inputs=True), and its OneHotCrossEntropyLoss, run on the CPU against the
reference package with the stub harness of make_golden.py.  Writes tests/golden/xent_fixture.npz (data only):

  <case>/x [B, T, D], <case>/lens [B], <case>/target [B, 1] int64, <case>/cw [C] (class weights), <case>/sd/<key>
  (state dict), <case>/logits [B, 1, C], and per variant v in mean, sum, mean_cw (reduction 'mean' / 'sum' / 'mean'
  with class weights): <case>/<v>/loss and <case>/<v>/grad/<key>, the parameter gradients of that loss.
  cases (xent_cases.MODEL_CASES): gru_cls    GRU(8) -> PoolLast -> Linear(5) on 6 inputs
                                  conv_cls   Conv1d(10, k 3, ReLU) -> GRU(8) -> PoolLast -> Linear(3) on 7 inputs
  onehot/x [2, 6, 9] logits, onehot/target [2, 6, 9] one-hot, onehot/elem [2, 8, 1] (OneHotCrossEntropyLoss(shift=1),
  reduction 'none'), onehot/grad [2, 6, 9] of its sum, and onehot/named_loss, onehot/named_grad: the reference's
  NamedLoss(type_="OneHotCrossEntropyLoss", seq_mask, 'mean_per_frame', shift=1) with onehot/mask [2, 8, 1],
  onehot/lens.
  acc/: UnWeightedAccuracy(num_per_class = acc/num_per_class) on gru_cls' logits and acc/target -> acc/value, when
  scikit-learn imports (the reference's class needs it); the generator says so when it does not.

  trainer/: the reference's ClassificationTrainer on the trainer fixture data (questions as input, a
  CategoryDataReader mapping an id to one of 3 classes by xent_cases.trainer_table; GRU(8) -> PoolLast -> Linear(3);
  3 epochs, seed 1234, batch_first): trainer/ids, trainer/classes (the table), trainer/init/<key>, trainer/final/<key>,
  trainer/val_losses (before training and after each epoch), trainer/train_losses, trainer/ids_val,
  trainer/val_logits, trainer/W_acc, trainer/U_acc, trainer/conf_matrix (compute_score on the validation set).  The
  generator asserts that every validation utterance's top-two logit gap exceeds 1e-3, so that a float32 difference
  cannot flip a prediction.  It needs scikit-learn (the reference's trainer imports it); without it the generator says
  so and leaves trainer/ out.
Usage: python tests/golden/make_golden_xent.py (needs the reference checkout)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import xent_cases as xc  # noqa: E402


def capture_model(out, case):
    import torch
    from idiaptts.src.neural_networks.pytorch.loss.NamedLoss import NamedLoss
    from idiaptts.src.neural_networks.pytorch.models import rnn_dyn
    name, groups, in_dim, n_cls, lens, seed = case
    torch.manual_seed(seed)
    model = xc.model_config(rnn_dyn.Config, case).create_model()
    x, target, cw = xc.model_inputs(torch, case)
    lens_t = torch.tensor(lens, dtype=torch.int64)
    p = name + "/"
    out[p + "x"], out[p + "lens"], out[p + "target"], out[p + "cw"] = x.numpy(), lens_t.numpy(), target.numpy(), cw.numpy()
    for k, v in model.state_dict().items():
        out[p + "sd/" + k] = np.array(v.numpy(), copy=True)
    for variant, reduction, weight in xc.MODEL_VARIANTS:
        model.zero_grad()
        model.init_hidden(len(lens))
        logits, _ = model(x, seq_lengths_input=lens_t.clone(), max_length_inputs=torch.tensor(int(max(lens))))
        kwargs = dict(weight=cw) if weight else {}
        loss_fn = NamedLoss.Config(name="ce", type_="CrossEntropyLoss", seq_mask=None,
                                   input_names=["class_pred", "class_true"], batch_first=True, squeeze_inputs=True,
                                   reduction=reduction, **kwargs).create_loss()
        loss = loss_fn({"class_pred": logits, "class_true": target}, {}, 0)["ce"]
        loss.backward()
        out[p + "logits"] = logits.detach().numpy()
        out[p + variant + "/loss"] = np.asarray(float(loss), dtype=np.float64)
        for k, v in model.named_parameters():
            out[p + variant + "/grad/" + k] = np.array(v.grad.numpy(), copy=True)
        print(name, variant, "logits", tuple(logits.shape), "loss", float(loss))
    return logits.detach(), target


def capture_onehot(out):
    import torch
    from idiaptts.src.neural_networks.pytorch.loss.NamedLoss import NamedLoss
    from idiaptts.src.neural_networks.pytorch.loss.OneHotCrossEntropyLoss import OneHotCrossEntropyLoss
    x, onehot, mask, lens = xc.onehot_inputs(torch)
    leaf = x.clone().requires_grad_(True)
    elem = OneHotCrossEntropyLoss(reduction="none", shift=1)(leaf, onehot)
    elem.sum().backward()
    out["onehot/x"], out["onehot/target"] = x.numpy(), onehot.numpy()
    out["onehot/elem"], out["onehot/grad"] = elem.detach().numpy(), leaf.grad.numpy()
    out["onehot/mask"], out["onehot/lens"] = mask.numpy(), lens.numpy()
    leaf = x.clone().requires_grad_(True)
    loss_fn = NamedLoss.Config(name="oh", type_="OneHotCrossEntropyLoss", seq_mask="mask", input_names=["pred", "true"],
                               batch_first=True, reduction="mean_per_frame", shift=1).create_loss()
    loss = loss_fn({"pred": leaf, "true": onehot, "mask": mask}, {"mask": lens}, 0)["oh"]
    loss.backward()
    out["onehot/named_loss"] = np.asarray(float(loss), dtype=np.float64)
    out["onehot/named_grad"] = leaf.grad.numpy()
    print("onehot: elem", tuple(elem.shape), "named loss", float(loss))


def capture_accuracy(out, logits, target):
    import torch
    try:
        from idiaptts.src.neural_networks.pytorch.loss.UnWeightedAccuracy import UnWeightedAccuracy
    except ImportError as e:
        print("acc NOT captured: the reference's UnWeightedAccuracy does not import (scikit-learn):", e)
        return
    num_per_class = torch.tensor(xc.ACC_NUM_PER_CLASS)
    out["acc/num_per_class"] = num_per_class.numpy().copy()
    target = target.clone()
    target[::2] = logits.argmax(dim=-1)[::2]          # every other utterance classified correctly
    out["acc/target"] = target.numpy()
    value = UnWeightedAccuracy(num_per_class.clone())(logits.squeeze(1), target.squeeze(1))
    out["acc/value"] = value.numpy()
    print("acc:", value)


def capture_trainer(out):
    import shutil
    from idiaptts.src.data_preparation.CategoryDataReader import CategoryDataReader
    from idiaptts.src.data_preparation.DataReaderConfig import DataReaderConfig
    from idiaptts.src.model_trainers.ClassificationTrainer import ClassificationTrainer
    from idiaptts.src.neural_networks.pytorch.loss.NamedLoss import NamedLoss
    from idiaptts.src.neural_networks.pytorch.models import rnn_dyn
    from idiaptts.src.neural_networks.pytorch.models.NamedForwardWrapper import NamedForwardWrapper
    os.chdir(os.path.join(mg.REF, "test"))
    with open(os.path.join("integration", "fixtures", "database", "file_id_list.txt")) as f:
        ids = [s.strip() for s in f.readlines()]
    table = xc.trainer_table(ids)
    hp = xc.trainer_hparams(ClassificationTrainer.create_hparams(), "/tmp/idiaptts_amd_golden_xent_train")
    hp.use_gpu = False
    readers = [DataReaderConfig(name="questions", feature_type="QuestionLabelGen",
                                directory=os.path.join("integration", "fixtures", "questions"), features="questions",
                                num_questions=409),
               CategoryDataReader.Config("class_true", lambda i: np.array([table[i]], dtype=np.int64))]
    trainer = ClassificationTrainer(hp, ids, data_reader_configs=readers)
    trainer.init(hp, model_config=xc.trainer_model_config(rnn_dyn, NamedForwardWrapper),
                 loss_configs=[xc.trainer_loss_config(NamedLoss)])
    p = "trainer/"
    out[p + "ids"], out[p + "classes"] = np.array(ids), np.array([table[i] for i in ids], dtype=np.int64)
    for k, v in trainer.model_handler.model.state_dict().items():
        out[p + "init/" + k] = np.array(v.cpu().numpy(), copy=True)
    val, train, _ = trainer.train(hp)
    out[p + "val_losses"] = np.asarray(val["ce"], dtype=np.float64)
    out[p + "train_losses"] = np.asarray(train["ce"], dtype=np.float64)
    for k, v in trainer.model_handler.model.state_dict().items():
        out[p + "final/" + k] = np.array(v.cpu().numpy(), copy=True)
    ids_val = list(trainer.id_list_val)
    output, _ = trainer.forward(hp, ids_val, post_processing_mapping={})
    logits = np.stack([np.asarray(output[i]["class_pred"]).reshape(-1) for i in ids_val])
    top = np.sort(logits, axis=1)
    assert float((top[:, -1] - top[:, -2]).min()) > 1e-3, "a top-two logit gap below 1e-3: pick another seed"
    score = trainer.compute_score({}, output, hp)
    out[p + "ids_val"], out[p + "val_logits"] = np.array(ids_val), logits
    out[p + "W_acc"], out[p + "U_acc"] = np.asarray(score["W_acc"]), np.asarray(score["U_acc"])
    out[p + "conf_matrix"] = np.asarray(score["conf_matrix"], dtype=np.float64)
    print("reference classification trainer: val", out[p + "val_losses"], "train", out[p + "train_losses"],
          "W_acc", score["W_acc"], "U_acc", score["U_acc"], "gap", float((top[:, -1] - top[:, -2]).min()))
    shutil.rmtree(hp.out_dir, ignore_errors=True)


def _main():
    mg.install_stub_harness()
    out = {}
    for case in xc.MODEL_CASES:
        logits, target = capture_model(out, case)
        if case[0] == "gru_cls":
            capture_accuracy(out, logits, target)
    capture_onehot(out)
    try:
        capture_trainer(out)
    except ImportError as e:
        print("trainer NOT captured: the reference's ClassificationTrainer does not import (scikit-learn):", e)
    path = os.path.join(HERE, "xent_fixture.npz")
    np.savez_compressed(path, **out)
    print("xent_fixture.npz:", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    _main()
