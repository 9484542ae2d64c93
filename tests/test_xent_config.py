"""The classification stack on the CPU side: the float64 restatement the GPU tests compare against
(xent_cases.reference64 / reference64_strided) is pinned to torch's own cross_entropy and autograd in float64;
NamedLoss.Config fields and fallbacks, squeeze_inputs shapes, refusals by name; the CPU path of the three new loss
types; CategoryDataReader through prepare_batch; ClassificationTrainer.compute_score and UnWeightedAccuracy against
numbers written out by hand."""
import numpy as np
import pytest
import torch

import xent_cases as xc
from idiaptts_amd.src.data_preparation.CategoryDataReader import CategoryDataReader
from idiaptts_amd.src.data_preparation.PyTorchDatareadersDataset import PyTorchDatareadersDataset
from idiaptts_amd.src.model_trainers.ClassificationTrainer import ClassificationTrainer, confusion_counts
from idiaptts_amd.src.neural_networks.pytorch.ModularModelHandlerPyTorch import ModularModelHandlerPyTorch
from idiaptts_amd.src.neural_networks.pytorch.loss.NamedLoss import NamedLoss
from idiaptts_amd.src.neural_networks.pytorch.loss.OneHotCrossEntropyLoss import OneHotCrossEntropyLoss
from idiaptts_amd.src.neural_networks.pytorch.loss.UnWeightedAccuracy import UnWeightedAccuracy

F = torch.nn.functional


# ---- the restatement equals torch in float64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,C", [(1, 1), (2, 2), (7, 5), (7, 17), (69, 64), (7, 257), (3, 4096)])
@pytest.mark.parametrize("weights", (False, True))
def test_restatement_equals_torch_float64(N, C, weights):
    x, t, cw, w = xc.rows_inputs(torch, N, C)
    t[::4] = xc.IGNORE
    w[N // 2] = 0.0
    cw = cw if weights else None
    ref = xc.reference64(torch, x, t, cw, w)
    leaf = x.double().requires_grad_(True)
    elem = F.cross_entropy(leaf, t, weight=None if cw is None else cw.double(), ignore_index=xc.IGNORE,
                           reduction="none") * w.double()
    elem.sum().backward()
    assert (elem.detach() - ref["elem"]).abs().max() < 1e-12
    assert abs(elem.detach().sum() - ref["loss"]) < 1e-12 * max(1.0, N)
    assert (leaf.grad - ref["grad"]).abs().max() < 1e-12


@pytest.mark.parametrize("shift", xc.SHIFTS)
def test_strided_restatement_equals_torch_float64(shift):
    B, C, T = 3, 5, 9
    x, onehot, idx, cw = xc.strided_inputs(torch, B, C, T)
    s = shift or 0
    w = 0.5 + torch.rand(B, T - s, generator=torch.Generator().manual_seed(3))
    ref = xc.reference64_strided(torch, x, onehot, cw, w, xc.IGNORE, shift)
    leaf = x.double().requires_grad_(True)
    # loss/OneHotCrossEntropyLoss.py:16-30, in float64
    targets = onehot.max(dim=1)[1]
    inp = leaf[..., :-s] if s else leaf
    elem = F.cross_entropy(inp, targets[..., s:], weight=cw.double(), reduction="none") * w.double()
    elem.sum().backward()
    assert (elem.detach() - ref["elem"]).abs().max() < 1e-12
    assert (leaf.grad - ref["grad"]).abs().max() < 1e-12
    if s:
        assert ref["grad"][:, :, -s:].abs().max() == 0


def test_restatement_special_rows():
    x, t, cw, w = xc.rows_inputs(torch, 5, 7)
    t[1] = 7                                  # out of range on a live row
    t[2] = -3
    w[2] = 0.0                                # .. and on a row of weight 0
    x[2] = float("nan")
    ref = xc.reference64(torch, x, t, cw, w)
    assert torch.isnan(ref["elem"][1]) and torch.isnan(ref["loss"]) and ref["grad"][1].abs().max() == 0
    assert ref["elem"][2] == 0 and ref["grad"][2].abs().max() == 0
    # arg-max order: lowest index among equals, first NaN
    v = torch.tensor([[1.0, 3.0, 3.0, 2.0], [0.0, float("nan"), 5.0, float("nan")], [float("inf"), 1.0, 2.0, 3.0]])
    assert xc.first_argmax(torch, v, -1).tolist() == [1, 1, 0] == torch.argmax(v, dim=-1).tolist()


def test_a_case_outside_the_named_ones_cannot_relax_the_bound():
    ref = torch.ones(4, dtype=torch.float64)
    sloppy = ref.float() * (1 + 1e-4)
    with pytest.raises(AssertionError, match="only the named"):
        xc.check("elem", ref.float(), ref, case="rows_7x5", torch32=sloppy)
    with pytest.raises(AssertionError, match="only the named"):
        xc.check("elem", ref.float(), ref, case=None, torch32=sloppy)
    with pytest.raises(AssertionError):
        xc.check("elem", sloppy, ref)                                  # the dense bound holds without a case
    xc.check("elem", sloppy, ref, case=xc.HAZARDS[0], torch32=sloppy * (1 + 1e-4))


# ---- NamedLoss ---------------------------------------------------------------------------------------------------------
def test_config_fields_and_fallbacks():
    c = NamedLoss.Config("ce", "CrossEntropyLoss", ["pred", "true"])
    assert c.squeeze_inputs is False and c.reduction == "mean" and c.seq_mask is None
    for type_ in ("CrossEntropyLoss", "OneHotCrossEntropyLoss", "UnWeightedAccuracy"):
        for red in ("mean_per_frame", "mean_per_sample"):
            assert NamedLoss.Config("l", type_, ["a", "b"], reduction=red).reduction == "mean"
            assert NamedLoss.Config("l", type_, ["a", "b"], seq_mask="m", reduction=red).reduction == red
        for red in ("mean", "sum", "none"):
            assert NamedLoss.Config("l", type_, ["a", "b"], reduction=red).reduction == red
    c = NamedLoss.Config("ce", "CrossEntropyLoss", ["pred", "true"], squeeze_inputs=True, batch_first=True,
                         weight=[1.0, 2.0], ignore_index=3, loss_weight=0.5, start_step=2)
    assert c.squeeze_inputs and c.kwargs == dict(weight=[1.0, 2.0], ignore_index=3)
    loss = c.create_loss()
    assert loss.ignore_index == 3 and loss.class_weight.tolist() == [1.0, 2.0] and loss.squeeze_inputs
    # MSELoss / L1Loss keep their fields, and today's refusal
    assert NamedLoss.Config("m", "MSELoss", ["a", "b"]).reduction == "mean_per_frame"
    for type_ in ("MSELoss", "L1Loss"):
        with pytest.raises(ValueError, match="needs a seq_mask"):
            NamedLoss.Config("m", type_, ["a", "b"]).create_loss()
    with pytest.raises(NotImplementedError, match="VAEKLDLoss"):
        NamedLoss.Config("k", "VAEKLDLoss", ["a", "b"]).create_loss()
    with pytest.raises(NotImplementedError, match="NLLLoss"):
        NamedLoss.Config("k", "NLLLoss", ["a", "b"]).create_loss()


def test_refusals_by_name():
    with pytest.raises(NotImplementedError, match="label_smoothing = 0.1"):
        NamedLoss.Config("ce", "CrossEntropyLoss", ["a", "b"], label_smoothing=0.1).create_loss()
    NamedLoss.Config("ce", "CrossEntropyLoss", ["a", "b"], label_smoothing=0.0).create_loss()
    with pytest.raises(NotImplementedError, match="'size_average'"):
        NamedLoss.Config("ce", "CrossEntropyLoss", ["a", "b"], size_average=True).create_loss()
    with pytest.raises(NotImplementedError, match="'shift'"):
        NamedLoss.Config("ce", "CrossEntropyLoss", ["a", "b"], shift=1).create_loss()
    with pytest.raises(NotImplementedError, match="'weight'"):
        NamedLoss.Config("ua", "UnWeightedAccuracy", ["a", "b"], num_per_class=[1, 2], weight=[1.0]).create_loss()
    # probability targets
    ce = NamedLoss.Config("ce", "CrossEntropyLoss", ["pred", "true"], batch_first=True).create_loss()
    with pytest.raises(NotImplementedError, match="probability"):
        ce({"pred": torch.randn(4, 3), "true": torch.rand(4)}, {}, 0)
    with pytest.raises(NotImplementedError, match=r"\(4, 3, 6\)"):
        ce({"pred": torch.randn(4, 3, 6), "true": torch.zeros(4, 6, dtype=torch.int64)}, {}, 0)
    # a mask of the wrong extent names both
    oh = NamedLoss.Config("oh", "OneHotCrossEntropyLoss", ["pred", "true"], seq_mask="m", batch_first=True,
                          shift=1).create_loss()
    x = torch.randn(2, 6, 9)
    data = {"pred": x, "true": torch.zeros(2, 6, 9), "m": torch.ones(2, 9, 1)}
    with pytest.raises(ValueError, match=r"2 x 9 frames .* 2 x 8 frames"):
        oh(data, {"m": torch.tensor([9, 7])}, 0)
    with pytest.raises(ValueError, match="shift = 9"):
        NamedLoss.Config("oh", "OneHotCrossEntropyLoss", ["pred", "true"], batch_first=True, shift=9) \
            .create_loss()(dict(data), {}, 0)
    with pytest.raises(NotImplementedError, match="'mean'"):
        OneHotCrossEntropyLoss(reduction="mean")


@pytest.mark.parametrize("B", (1, 4))
@pytest.mark.parametrize("batch_first", (True, False))
def test_squeeze_inputs_shapes(B, batch_first):
    """[B, 1, C] / [B, 1] (time-major [1, B, C] / [1, B]) -> [B, C] / [B]; batch size 1 keeps its batch extent"""
    C = 5
    g = torch.Generator().manual_seed(B)
    pred = torch.randn((B, 1, C) if batch_first else (1, B, C), generator=g, requires_grad=True)
    true = torch.randint(0, C, (B, 1) if batch_first else (1, B), generator=g)
    cw = 0.5 + torch.rand(C, generator=g)
    loss = NamedLoss.Config("ce", "CrossEntropyLoss", ["pred", "true"], batch_first=batch_first, squeeze_inputs=True,
                            reduction="none", weight=cw).create_loss()
    sq = loss._squeeze([pred, true])
    assert sq[0].shape == (B, C) and sq[1].shape == (B,)
    out = loss({"pred": pred, "true": true}, {}, 0)["ce"]
    ref = xc.reference64(torch, pred.detach().reshape(B, C), true.reshape(B), cw)
    assert out.shape == (B,) and (out.detach().double() - ref["elem"]).abs().max() < 1e-5
    for red, expect in (("mean", ref["loss"] / B), ("sum", ref["loss"]), ("mean_per_frame", ref["loss"] / B)):
        loss = NamedLoss.Config("ce", "CrossEntropyLoss", ["pred", "true"], batch_first=batch_first,
                                squeeze_inputs=True, reduction=red, weight=cw, loss_weight=2.0).create_loss()
        data = {"pred": pred, "true": true}
        out = loss(data, {}, 0)["ce"]
        assert out.dim() == 0 and abs(out.item() - 2.0 * expect.item()) < 1e-5 and data["ce"] is out
        pred.grad = None
        out.backward()
        scale = 2.0 / B if red != "sum" else 2.0
        assert (pred.grad.reshape(B, C).double() - scale * ref["grad"]).abs().max() < 1e-5
    # start_step: weight 0 before it
    loss = NamedLoss.Config("ce", "CrossEntropyLoss", ["pred", "true"], batch_first=batch_first, squeeze_inputs=True,
                            start_step=3).create_loss()
    assert loss({"pred": pred, "true": true}, {}, 2)["ce"].item() == 0.0


@pytest.mark.parametrize("reduction", xc.REDUCTIONS)
@pytest.mark.parametrize("shift", xc.SHIFTS)
def test_onehot_reductions_on_cpu_tensors(reduction, shift):
    """the reference's `seq_mask * v` and _reduce (loss/NamedLoss.py:93-131) on the [B, T', 1] loss, written out"""
    B, C, T = 3, 6, 9
    s = shift or 0
    x, onehot, idx, cw = xc.strided_inputs(torch, B, C, T, seed=2)
    lens = torch.tensor([T - s, 4, 6])
    mask = (torch.arange(T - s)[None, :] < lens[:, None]).float()
    v = xc.reference64_strided(torch, x, onehot, cw, None, xc.IGNORE, shift)["elem"][..., None] * mask[..., None]
    if reduction == "mean_per_frame":
        expect = (v.sum(dim=(0, 1)) / lens.sum().float()).mean()
    elif reduction == "mean_per_sample":
        expect = (v.sum(dim=1) / lens.unsqueeze(-1).float()).mean()
    else:
        expect = {"mean": v.mean(), "sum": v.sum(), "none": v}[reduction]
    w = xc.reduction_weight(torch, reduction, mask, lens)
    folded = xc.reference64_strided(torch, x, onehot, cw, w, xc.IGNORE, shift)
    assert ((folded["elem"][..., None] if reduction == "none" else folded["loss"]) - expect).abs().max() < 1e-12
    loss = NamedLoss.Config("oh", "OneHotCrossEntropyLoss", ["pred", "true"], seq_mask="m", batch_first=True,
                            reduction=reduction, weight=cw, shift=shift).create_loss()
    leaf = x.clone().requires_grad_(True)
    out = loss({"pred": leaf, "true": onehot, "m": mask[..., None]}, {"m": lens}, 0)["oh"]
    assert out.shape == expect.shape and (out.detach().double() - expect).abs().max() < 1e-5
    out.sum().backward()
    assert (leaf.grad.double() - folded["grad"]).abs().max() < 1e-5
    # the class itself: the reference's return shape
    fn = OneHotCrossEntropyLoss(weight=cw, shift=shift)
    assert fn(x, onehot).shape == (B, T - s, 1)


# ---- reader --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((1,), (1, 1)))
@pytest.mark.parametrize("batch_first", (True, False))
def test_category_reader_round_trip(shape, batch_first):
    table = {"utt_a": 2, "utt_b": 0, "utt_c": 1, "utt_d": 2}
    cfg = CategoryDataReader.Config("class_true", lambda id_: np.full(shape, table[id_], dtype=np.int64))
    assert cfg.output_names == ["class_true"] and cfg.match_length is None
    reader = cfg.create_reader()
    item = reader["utt_c"]
    assert list(item) == ["class_true"] and item["class_true"].dtype == np.int64 and item["class_true"].shape == shape
    assert reader.name == "class_true" and reader.match_length is None and not reader.requires_seq_mask

    class Frames(CategoryDataReader):           # a float stream of 3 .. 6 frames beside it
        def __getitem__(self, id_):
            return {self.name: np.full((3 + table[id_] + len(id_) % 2, 4), 0.5, dtype=np.float32), "_id_list": id_}
    frames = Frames(CategoryDataReader.Config("questions", None))
    dataset = PyTorchDatareadersDataset(list(table), [frames, reader])
    out, _ = dataset[1]
    assert out["class_true"].dtype == np.int64 and out["class_true"].shape == shape
    data, lengths = ModularModelHandlerPyTorch.prepare_batch([dataset[i] for i in range(4)],
                                                             batch_first=batch_first)
    got = data["class_true"]
    assert got.dtype == torch.int64
    assert got.shape == ((4, 1) if batch_first else (1, 4)) + shape[1:]
    assert got.reshape(-1).tolist() == [2, 0, 1, 2] and lengths["class_true"].tolist() == [1, 1, 1, 1]
    assert data["questions"].dtype == torch.float32 and data["_id_list"] == list(table)
    # .. and through squeeze_inputs into the loss as int64 class indices
    loss = NamedLoss.Config("ce", "CrossEntropyLoss", ["pred", "class_true"], batch_first=batch_first,
                            squeeze_inputs=True).create_loss()
    pred = torch.randn((4, 1, 3) if batch_first else (1, 4, 3))
    data["pred"] = pred
    assert abs(loss(data, lengths, 0)["ce"].item() - F.cross_entropy(pred.reshape(4, 3), torch.tensor([2, 0, 1, 2])).item()) < 1e-6


# ---- scores ----------------------------------------------------------------------------------------------------------------
def _score_case():
    """7 utterances, 4 classes (class 3 empty): true 0 0 0 1 1 2 2, predicted 0 0 1 1 2 2 2"""
    true = [0, 0, 0, 1, 1, 2, 2]
    pred = [0, 0, 1, 1, 2, 2, 2]
    output = {}
    for i, (t, p) in enumerate(zip(true, pred)):
        logits = np.full((1, 4), -1.0, dtype=np.float32)
        logits[0, p] = 0.25 * (i + 1)
        output["utt{}".format(i)] = {"class_pred": logits, "class_true": np.array([[t]], dtype=np.int64)}
    return true, pred, output


def test_compute_score_against_numbers_by_hand():
    true, pred, output = _score_case()
    hparams = ClassificationTrainer.create_hparams()
    assert (hparams.class_pred_name, hparams.class_true_name, hparams.num_classes, hparams.class_names) == \
        ("class_pred", "class_true", -1, None)
    hparams.num_classes = 4
    hparams.class_names = ["a", "b", "c", "d"]
    trainer = ClassificationTrainer.__new__(ClassificationTrainer)
    score = trainer.compute_score({}, output, hparams)
    assert sorted(score) == ["U_acc", "W_acc", "conf_matrix"]
    assert score["W_acc"] == 5 / 7
    assert abs(score["U_acc"] - (2 / 3 + 1 / 2 + 1 + 0) / 4) < 1e-15
    expect = np.array([[2 / 3, 1 / 3, 0, 0], [0, 1 / 2, 1 / 2, 0], [0, 0, 1, 0], [0, 0, 0, 0]])
    assert np.array_equal(score["conf_matrix"], expect)
    assert np.array_equal(confusion_counts(true, pred, 4),
                          np.array([[2, 1, 0, 0], [0, 1, 1, 0], [0, 0, 2, 0], [0, 0, 0, 0]]))


def test_compute_score_against_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    true, pred, output = _score_case()
    hparams = ClassificationTrainer.create_hparams()
    hparams.num_classes = 4
    score = ClassificationTrainer.__new__(ClassificationTrainer).compute_score({}, output, hparams)
    conf = metrics.confusion_matrix(true, pred, labels=range(4))
    assert np.array_equal(confusion_counts(true, pred, 4), conf)
    assert score["W_acc"] == metrics.accuracy_score(true, pred)
    per_class = conf.sum(axis=1)[:, None]
    per_class[per_class == 0] = 1
    assert np.array_equal(score["conf_matrix"], conf / per_class)


def test_unweighted_accuracy_on_cpu_tensors():
    """reference loss/UnWeightedAccuracy.py:13-35: the divisors are the constructor's, not the batch's"""
    true, pred, output = _score_case()
    logits = torch.from_numpy(np.concatenate([o["class_pred"] for o in output.values()]))
    num_per_class = torch.tensor([10, 4, 0, 6])
    fn = UnWeightedAccuracy(num_per_class)
    assert num_per_class.tolist() == [10, 4, 0, 6]                       # the caller's tensor is left alone
    out = fn(logits, torch.tensor(true))
    assert out.shape == (1,) and out.dtype == torch.float32 and not out.requires_grad
    weighted = np.float32(5) / np.float32(20)
    unweighted = np.float32((2 / 10 + 1 / 4 + 2 / 1 + 0 / 6) / 4)
    assert out.item() == -(weighted + unweighted)
    # through NamedLoss as a validation loss, with squeeze_inputs
    loss = NamedLoss.Config("acc", "UnWeightedAccuracy", ["class_pred", "class_true"], batch_first=True,
                            squeeze_inputs=True, num_per_class=torch.tensor([10, 4, 0, 6])).create_loss()
    data = {"class_pred": logits[:, None, :].clone().requires_grad_(True), "class_true": torch.tensor(true)[:, None]}
    got = loss(data, {}, 0)["acc"]
    assert got.dim() == 0 and got.item() == out.item() and not got.requires_grad
    with pytest.raises(ValueError, match="seq_mask"):
        NamedLoss.Config("acc", "UnWeightedAccuracy", ["a", "b"], seq_mask="m", num_per_class=[1]).create_loss()


def test_no_scikit_learn_import_in_the_package():
    import os
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "idiaptts_amd")
    for folder, _, files in os.walk(root):
        for name in files:
            if name.endswith(".py"):
                text = open(os.path.join(folder, name)).read()
                assert "import sklearn" not in text and "from sklearn" not in text, name
