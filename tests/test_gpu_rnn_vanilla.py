"""Vanilla RNN layers (tanh / ReLU) on the step kernels of csrc/rnn_step.h against torch.nn.RNN(...).double() on a
pack_padded_sequence(enforce_sorted=False): the oracle, the comparison routine and the budget of tests/rnn_cases.py
(2e-5 absolute on outputs and final states, every gradient tensor -- dx, all parameters, dh0 -- within
1e-4 * max(1, max |ref|)).  rc.compare also asserts that the inference output equals the training-mode output bit for
bit and that the padding holds exact zeros; every case has a non-zero shared h_0.

What the cases reach (forward kernel: a workgroup owns 16 hidden units, its four waves split K by ksplit / kiter of
rnn_step_forward, NT = min(tiles, 4) batch tiles of 16 rows per pass; backward: 16 units x 16 rows per workgroup):
  H = 16 (ksplit 1, kiter 1), 48 / 96 / 288 / 576 (ksplit 1 / 2 / 2 / 4 with kiter 3 / 3 / 9 / 9: partly empty chunks
  of 8 k-steps), 512 (ksplit 4, kiter 8: one full chunk), 40 and 1 (zero-padded to 48 and 16); B = 1 with T = 1,
  B = 16 exactly, B = 17 (a second tile of one row), 70 rows in one direction (five tiles: a second NT = 4 pass), rows
  of length 1, lengths=None, batch_first, two layers.

Further: a loss on h_n (which the LSTM / GRU layers refuse), two identical calls give identical bits, the layer-call
counts, and AcousticModelTrainer on a BiRNNTANH model against the reference's own CPU run
(tests/golden/rnn_vanilla_fixture.npz, written by tests/golden/make_golden_rnn_vanilla.py).

Measured on one MI355X, worst over the file: outputs 4.6e-7, final states 3.8e-7, gradients 1.3e-6 of their scale;
the file takes 7 s, the trainer 3.5 s of it."""
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rnn_cases as rc  # noqa: E402
from fixture_dirs import materialise  # noqa: E402

pytestmark = pytest.mark.gpu

_RAGGED = [7, 11, 1, 7, 3]
CASES = [rc._case("v16_%ddir" % ndir, ndir, _RAGGED, H=16) for ndir in (1, 2)] + [
    rc._case("v%d" % H, 2, rc.WIDTH_LENGTHS, H=H) for H in (48, 96, 288, 576)] + [
    rc._case("v512", 2, [9] * 16 + [8] * 16 + [5] * 16 + [4] * 3, H=512),
    rc._case("v40_padded", 2, _RAGGED, H=40),
    rc._case("v1_padded", 2, _RAGGED, H=1),
    rc._case("v_one_frame_one_row", 1, [1], H=32),
    rc._case("v_exact_tile", 2, (list(range(10, 0, -1)) * 2)[:16], H=32),
    rc._case("v_17_rows", 2, (list(range(10, 0, -1)) * 2)[:17], H=32),
    rc._case("v_five_tiles", 1, [6, 5, 4, 3, 2, 1, 1] * 10, H=64),
    rc._case("v_one_frame", 2, [1] * 20, H=32),
    rc._case("v_lengths_none", 2, [6] * 18, H=32, batch_first=True, lengths_none=True),
    rc._case("v_batch_first", 1, _RAGGED, H=32, batch_first=True),
    rc._case("v_two_layers", 2, [12, 12, 11, 9, 9, 8, 7, 7, 6, 5, 5, 4, 3, 3, 2, 2, 1, 1, 1, 12], H=32, layers=2),
]
_BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(autouse=True)
def _registered(monkeypatch):
    """rc.reference / rc.compare look a case up by name: ours are in the table while one of these tests runs"""
    for c in CASES:
        monkeypatch.setitem(rc.ALL_CASES, c.name, c)


def _kwargs(nonlinearity):
    return (("nonlinearity", nonlinearity),)


@pytest.mark.parametrize("nonlinearity", ["tanh", "relu"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_matches_torch_float64(gpu, case, nonlinearity):
    rc.compare(case, "RNN", gpu, kwargs=_kwargs(nonlinearity))


def _module(r, case, nonlinearity, gpu):
    from idiaptts_amd import nn as inn
    mine = rc._new_module(inn, "RNN", case, _kwargs(nonlinearity))
    mine.load_state_dict(r.state)
    return mine.to(gpu)


@pytest.mark.parametrize("with_output", [True, False], ids=["out_and_hn", "hn_only"])
@pytest.mark.parametrize("name,nonlinearity", [("v_two_layers", "tanh"), ("v40_padded", "relu"), ("v_17_rows", "tanh"),
                                               ("v_batch_first", "relu")])
def test_loss_on_the_final_state_matches_torch_float64(gpu, name, nonlinearity, with_output):
    """out.sum() + h_n.sum() (and h_n.sum() alone: no gradient into the output at all): h_n of a row is y at the last
    frame its direction processes, so its gradient enters dy there -- in every layer, at a padded hidden size too"""
    case = _BY_NAME[name]
    r = rc.reference(name, "RNN", _kwargs(nonlinearity))
    B, T = len(r.lens), max(r.lens)
    ref = rc._new_module(torch.nn, "RNN", case, _kwargs(nonlinearity)).double()
    ref.load_state_dict({k: v.double() for k, v in r.state.items()})
    xr, h0r = r.x.double().requires_grad_(True), r.h0.double().requires_grad_(True)
    out_p, hn_r = ref(pack_padded_sequence(xr, torch.tensor(r.lens), batch_first=case.batch_first,
                                           enforce_sorted=False), h0r.expand(-1, B, -1))
    out_r, _ = pad_packed_sequence(out_p, batch_first=case.batch_first, total_length=T)
    (hn_r.sum() + (out_r.sum() if with_output else 0.0)).backward()

    mine = _module(r, case, nonlinearity, gpu)
    x, h0 = r.x.to(gpu).requires_grad_(True), r.h0.to(gpu).requires_grad_(True)
    out, hn = mine(x, h0.expand(-1, B, -1), torch.tensor(r.lens, dtype=torch.int64))
    (hn.sum() + (out.sum() if with_output else 0.0)).backward()
    assert rc._abs_err(out, out_r.detach()) < rc.OUT_ABS and rc._abs_err(hn, hn_r.detach()) < rc.OUT_ABS
    errs = {"dx": rc._grad_err(x.grad, xr.grad), "dh0": rc._grad_err(h0.grad, h0r.grad)}
    grads_r = dict(ref.named_parameters())
    for n, p in mine.named_parameters():
        errs[n] = rc._grad_err(p.grad, grads_r[n].grad)
    print(errs)
    for n, e in errs.items():
        assert e < rc.GRAD_REL, (n, e)


@pytest.mark.parametrize("nonlinearity", ["tanh", "relu"])
def test_two_identical_calls_give_identical_bits(gpu, nonlinearity):
    case = _BY_NAME["v_two_layers"]
    r = rc.reference(case.name, "RNN", _kwargs(nonlinearity))
    mine = _module(r, case, nonlinearity, gpu)
    B = len(r.lens)
    runs = []
    for _ in range(2):
        x, h0 = r.x.to(gpu).requires_grad_(True), r.h0.to(gpu).requires_grad_(True)
        out, hn = mine(x, h0.expand(-1, B, -1), torch.tensor(r.lens, dtype=torch.int64))
        (out * r.w.to(gpu)).sum().backward()
        runs.append((out.detach(), hn.detach(), x.grad, h0.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_layer_counts_move_by_the_layer_calls_made_and_the_path_counts_do_not(gpu):
    from idiaptts_amd import ops
    case = _BY_NAME["v_two_layers"]
    r = rc.reference(case.name, "RNN", _kwargs("tanh"))
    mine = _module(r, case, "tanh", gpu)
    x = r.x.to(gpu).requires_grad_(True)
    lens = torch.tensor(r.lens, dtype=torch.int64)
    layers0, paths0 = ops.rnn_layer_counts(), ops.rnn_path_counts()
    out, _ = mine(x, None, lens)
    assert tuple(ops.rnn_layer_counts()) == (layers0.fwd + 2, layers0.bwd)
    out.sum().backward()
    assert tuple(ops.rnn_layer_counts()) == (layers0.fwd + 2, layers0.bwd + 2)
    with torch.no_grad():
        mine(x, None, lens)
    torch.cuda.synchronize()
    assert tuple(ops.rnn_layer_counts()) == (layers0.fwd + 4, layers0.bwd + 2)
    assert ops.rnn_path_counts() == paths0


def test_trainer_reproduces_reference_losses(gpu, golden_dir, tmp_path):
    """The reference AcousticModelTrainer run of make_golden_rnn_vanilla.py (trainer data of trainer_fixture.npz,
    seed 1234, 3 epochs, batch size 2, Adam 1e-3, batch_first) with RNNDYN-1_TANH_32-1_BiRNNTANH_16-1_FC_67: same
    initial weights, per-epoch losses to rtol 2e-5 and final weights to atol 2e-5, the recurrent group on the layer
    entry points"""
    from idiaptts_amd import ops
    from idiaptts_amd.src.model_trainers.AcousticModelTrainer import AcousticModelTrainer
    g = np.load(os.path.join(golden_dir, "rnn_vanilla_fixture.npz"))
    root = str(tmp_path)
    ids, wdir, qdir, _ = materialise(golden_dir, root)
    hp = AcousticModelTrainer.create_hparams()
    hp.num_questions = 409
    hp.voice = "full"
    hp.out_dir = os.path.join(root, "rnn_vanilla_train")
    hp.frame_size_ms = 5
    hp.num_coded_sps = 20
    hp.seed = 1234
    hp.epochs = 3
    hp.use_gpu = True
    hp.dataset_num_workers_gpu = 0
    hp.batch_first = True
    hp.model_type = "RNNDYN-1_TANH_32-1_BiRNNTANH_16-1_FC_67"
    hp.batch_size_train = 2
    hp.batch_size_val = 50
    hp.use_saved_learning_rate = True
    hp.optimiser_args["lr"] = 0.001
    hp.model_name = "test_model"
    hp.epochs_per_checkpoint = 2
    hp.world_dir = wdir
    hp.use_best_as_final_model = False
    trainer = AcousticModelTrainer(**AcousticModelTrainer.legacy_support_init(wdir, qdir, ids, hp.num_questions, hp))
    trainer.init(hp)
    sd = trainer.model_handler.model.state_dict()
    init = {k[len("trainer/init/"):] for k in g.files if k.startswith("trainer/init/")}
    assert set(sd.keys()) == init
    for k in init:
        assert np.array_equal(sd[k].cpu().numpy(), g["trainer/init/" + k]), k
    before = ops.rnn_layer_counts()
    all_loss, all_loss_train, handler = trainer.train(hp)
    after = ops.rnn_layer_counts()
    assert after.fwd > before.fwd and after.bwd > before.bwd
    key = "MSELoss_acoustic_features"
    np.testing.assert_allclose(all_loss[key], g["trainer/val_losses"], rtol=2e-5)
    np.testing.assert_allclose(all_loss_train[key], g["trainer/train_losses"], rtol=2e-5)
    sd = handler.model.state_dict()
    for k in sd:
        np.testing.assert_allclose(sd[k].cpu().numpy(), g["trainer/final/" + k], rtol=0, atol=2e-5)
