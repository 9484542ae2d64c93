"""RNNDyn with self-attention layer groups on the GPU: the reference's own CPU runs (tests/golden/attention_fixture.npz,
written by tests/golden/make_golden_attention.py; the reference passes no mask) at every padded position, the masked
mode against the float64 block restatement and torch's float64 modules under src_key_padding_mask, bit-identity of a
masked utterance across batches, which kernels ran, the rule for groups behind an attention group, the block's own
dropout, config.json / checkpoints, and AcousticModelTrainer on the module path."""
import os

import numpy as np
import pytest
import torch

import attention_spec as spec
from fixture_dirs import materialise
from idiaptts_amd import ops
from idiaptts_amd.native_ff import FlatFFModel
from idiaptts_amd.nn.functional import padding_rows_identical
from idiaptts_amd.nn.modules import TransformerEncoderLayer
from idiaptts_amd.src.neural_networks.pytorch.models import rnn_dyn
from idiaptts_amd.src.neural_networks.pytorch.models.rnn_dyn import Config, RNNDyn

pytestmark = pytest.mark.gpu

LENS = list(spec.MODEL_LENS)
B, T = len(LENS), max(LENS)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "attention_fixture.npz"))


@pytest.fixture
def attention_calls(monkeypatch):
    """(shape of qkv, whether lengths were given, p) of every ops.attention_forward call"""
    calls = []
    real = ops.attention_forward

    def spy(qkv, nhead, klen=None, batch_first=True, p=0.0, seed=0, salt=0):
        calls.append((tuple(qkv.shape), klen is not None, p))
        return real(qkv, nhead, klen, batch_first, p, seed, salt)

    monkeypatch.setattr(ops, "attention_forward", spy)
    return calls


def _state_dict(g, name):
    p = name + "/sd/"
    return {k[len(p):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(p)}


def _model(g, name, bf, norm_first=False, **extra):
    """this package's RNNDyn of a fixture case with the reference's weights, on the GPU"""
    model = RNNDyn(spec.model_config(Config, bf, norm_first, **extra))
    sd = _state_dict(g, name)
    assert list(model.state_dict().keys()) == list(sd.keys())          # key for key
    model.load_state_dict(sd)
    return model.cuda()


def _forward(model, x, lens=LENS):
    n = len(lens)
    model.init_hidden(n)
    return model(x, seq_lengths_input=torch.tensor(lens), max_length_inputs=torch.tensor(max(lens)))


def _check_grads(model, ref_of, label):
    for k, prm in model.named_parameters():
        spec.check(label + " d" + k, prm.grad, torch.from_numpy(ref_of(k)), reduced=prm.dim() == 1)


@pytest.mark.parametrize("name,bf,norm_first,seed", spec.MODEL_CASES, ids=[c[0] for c in spec.MODEL_CASES])
def test_reference_case_default_mode(gpu, golden, attention_calls, name, bf, norm_first, seed):
    """the reference's model: outputs at EVERY position (padded positions are keys and are computed) and all
    parameter gradients of sum(y * w) against its float64 run, at the dense layers' bounds; train() with the block's
    dropout at 0 and eval() agree bit for bit"""
    g = golden
    p = name + "/"
    model = _model(g, name, bf, norm_first, layer_dropout=0.0).train()
    x, w = torch.from_numpy(g[p + "x"]).cuda(), torch.from_numpy(g[p + "w"]).cuda()
    xs, ws = spec.model_inputs(seed, bf)
    assert torch.equal(xs, x.cpu()) and torch.equal(ws, w.cpu())
    y, kwargs = _forward(model, x)
    assert attention_calls == [((B, T, 48) if bf else (T, B, 48), False, 0.0)] * 2
    assert np.array_equal(np.asarray(kwargs["seq_lengths_input"]), g[p + "seq_lengths_input"])
    assert int(kwargs["max_length_inputs"]) == int(g[p + "max_length_inputs"])
    (y * w).sum().backward()
    ref = torch.from_numpy(g[p + "y"])
    spec.check(name + " y", y.detach(), ref)
    # the reference's own float32 run sits inside the same bounds
    spec.check(name + " y (reference float32)", torch.from_numpy(g[p + "y32"]), ref)
    _check_grads(model, lambda k: g[p + "grad/" + k], name)
    model.eval()
    with torch.no_grad():
        y_eval, _ = _forward(model, x)
    assert torch.equal(y_eval, y.detach())
    assert len(attention_calls) == 4                     # no torch fallback under no_grad either
    assert FlatFFModel.from_module(model) is None


def _torch_float64_model(sd, bf, norm_first):
    """Linear + Tanh, two torch.nn.TransformerEncoderLayer, Linear in float64 with the fixture's weights"""
    blocks = [torch.nn.TransformerEncoderLayer(spec.MODEL_D, spec.MODEL_H, spec.MODEL_F, dropout=0.0, batch_first=bf,
                                               norm_first=norm_first) for _ in range(2)]
    for i, blk in enumerate(blocks):
        blk.load_state_dict({k[len("2.module.{}.".format(i)):]: v for k, v in sd.items()
                             if k.startswith("2.module.{}.".format(i))})
    lin1, lin2 = torch.nn.Linear(spec.MODEL_IN, spec.MODEL_D), torch.nn.Linear(spec.MODEL_D, spec.MODEL_OUT)
    lin1.load_state_dict({"weight": sd["1.module.0.weight"], "bias": sd["1.module.0.bias"]})
    lin2.load_state_dict({"weight": sd["3.module.0.weight"], "bias": sd["3.module.0.bias"]})
    mods = torch.nn.ModuleList([lin1, blocks[0], blocks[1], lin2]).double().train()

    def forward(x, lens):
        n_t = x.shape[1 if bf else 0]
        pad = ~(torch.arange(n_t)[None, :] < torch.tensor(lens)[:, None])
        h = torch.tanh(mods[0](x.double()))
        for blk in (mods[1], mods[2]):
            h = blk(h, src_key_padding_mask=pad)
        return mods[3](h)

    return mods, forward


@pytest.mark.parametrize("name,bf,norm_first,seed", spec.MODEL_CASES, ids=[c[0] for c in spec.MODEL_CASES])
def test_mask_padding_against_spec_and_torch_float64(gpu, golden, attention_calls, name, bf, norm_first, seed):
    g = golden
    model = _model(g, name, bf, norm_first, mask_padding=True, layer_dropout=0.0).train()
    x, w = spec.model_inputs(seed, bf)
    y, _ = _forward(model, x.cuda())
    assert [c[1] for c in attention_calls] == [True, True]
    (y * w.cuda()).sum().backward()
    sd = _state_dict(g, name)
    mods, forward64 = _torch_float64_model(sd, bf, norm_first)
    ref = forward64(x, LENS)
    (ref * w.double()).sum().backward()
    spec.check(name + " masked y", y.detach(), ref.detach())
    names = ["1.module.0.", "2.module.0.", "2.module.1.", "3.module.0."]
    grads = {}
    for prefix, mod in zip(names, mods):
        grads.update({prefix + k: prm.grad for k, prm in mod.named_parameters()})
    for k, prm in model.named_parameters():
        spec.check(name + " masked d" + k, prm.grad, grads[k], reduced=prm.dim() == 1)
    # the block restatement of tests/attention_spec.py on the same weights
    sd64 = {k: v.double() for k, v in sd.items()}
    xb = (x if bf else x.transpose(0, 1)).double()
    h = torch.tanh(xb @ sd64["1.module.0.weight"].t() + sd64["1.module.0.bias"])
    for i in range(2):
        h = spec.block_forward(h, sd64, spec.MODEL_H, LENS, norm_first, prefix="2.module.{}.".format(i))
    ours = h @ sd64["3.module.0.weight"].t() + sd64["3.module.0.bias"]
    assert ((ours if bf else ours.transpose(0, 1)) - ref.detach()).abs().max() < 1e-12
    # masking changes the valid frames: the default mode is another function
    assert (torch.from_numpy(g[name + "/y"]) - ref.detach()).abs().max() > 1e-3


@pytest.mark.parametrize("bf", [True, False])
def test_masked_utterance_is_bit_identical_in_any_batch(gpu, golden, bf):
    name = "bf" if bf else "tm"
    model = _model(golden, name, bf, mask_padding=True).eval()
    g = torch.Generator().manual_seed(9)
    lens = [50, 37, 64, 9]
    utts = [torch.randn(n, spec.MODEL_IN, generator=g) for n in lens]

    def batch(ids):
        n_t = max(lens[i] for i in ids)
        x = torch.zeros(len(ids), n_t, spec.MODEL_IN)
        for row, i in enumerate(ids):
            x[row, :lens[i]] = utts[i]
        with torch.no_grad():
            y, _ = _forward(model, (x if bf else x.transpose(0, 1).contiguous()).cuda(), [lens[i] for i in ids])
        y = y if bf else y.transpose(0, 1)
        return {i: y[row, :lens[i]].cpu() for row, i in enumerate(ids)}

    alone = batch([1])
    assert alone[1].abs().max() > 0
    for ids in ([0, 1, 2, 3], [1, 3], [2, 1]):
        assert torch.equal(batch(ids)[1], alone[1]), ids
    # the default mode is the reference's: the padding an utterance gets changes its valid frames
    plain = _model(golden, name, bf).eval()
    model = plain
    assert not torch.equal(batch([0, 1])[1], batch([1])[1])


def test_linear_group_behind_attention_in_a_vouched_batch(gpu, golden, attention_calls):
    """inside padding_rows_identical() the groups in front of the attention group may run on the valid rows; behind
    it no representative row stands in for the padding positions: the same values as every position computed"""
    model = _model(golden, "bf", True, layer_dropout=0.0).train()
    x, w = spec.model_inputs(61, True)
    results = []
    for vouched in (False, True):
        model.zero_grad()
        with padding_rows_identical(vouched):
            y, _ = _forward(model, x.cuda())
        (y * w.cuda()).sum().backward()
        results.append((y.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
    assert torch.equal(results[0][0], results[1][0])
    spec.check("vouched y", results[1][0], torch.from_numpy(golden["bf/y"]))
    for k in results[0][1]:
        spec.check("vouched d" + k, results[1][1][k], torch.from_numpy(golden["bf/grad/" + k]),
                   reduced=results[1][1][k].dim() == 1)
    assert len(attention_calls) == 4 and all(c[0] == (B, T, 48) for c in attention_calls)


def test_layer_dropout(gpu, golden, attention_calls):
    x, _ = spec.model_inputs(61, True)
    x = x.cuda()
    model = _model(golden, "bf", True).train()                # the default: 0.1 inside the block, as in the reference
    assert [m.p for m in model.modules() if isinstance(m, TransformerEncoderLayer)] == [0.1, 0.1]
    y1, _ = _forward(model, x)
    y2, _ = _forward(model, x)
    assert not torch.equal(y1, y2)
    assert [c[2] for c in attention_calls] == [0.1] * 4
    (y1.sum()).backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
    model.eval()
    e1, _ = _forward(model, x)
    e2, _ = _forward(model, x)
    assert torch.equal(e1, e2) and [c[2] for c in attention_calls[4:]] == [0.0] * 4
    off = _model(golden, "bf", True, layer_dropout=0).train()
    t1, _ = _forward(off, x)
    t2, _ = _forward(off, x)
    assert torch.equal(t1, t2) and torch.equal(t1, e1)
    # a LayerConfig(dropout=p) puts the package's Dropout behind each block
    cfg = spec.model_config(Config, True, layer_dropout=0.0)
    cfg.layer_configs[1].dropout = 0.5
    dropped = RNNDyn(cfg)
    assert [type(m).__name__ for m in dropped[1].module] == ["TransformerEncoderLayer", "Dropout"] * 2
    # the Dropout slots hold no parameters and move the second block to slot 2, as in the reference's Sequential
    dropped.load_state_dict({k.replace("2.module.1.", "2.module.2."): v for k, v in _state_dict(golden, "bf").items()})
    dropped = dropped.cuda().train()
    d1, _ = _forward(dropped, x)
    d2, _ = _forward(dropped, x)
    assert not torch.equal(d1, d2)


def test_config_json_and_checkpoint_round_trip(gpu, golden, tmp_path):
    from idiaptts_amd.src.ExtendedHParams import ExtendedHParams
    from idiaptts_amd.src.neural_networks.pytorch.ModularModelHandlerPyTorch import ModularModelHandlerPyTorch as Handler
    from idiaptts_amd.src.neural_networks.pytorch.models.NamedForwardWrapper import NamedForwardWrapper
    cfg = spec.model_config(rnn_dyn.Config, True, norm_first=True, mask_padding=True, layer_dropout=0.25)
    cfg.layer_configs[1].dropout = 0.125
    wrapped = NamedForwardWrapper.Config(wrapped_model_config=cfg, input_names=["questions"], batch_first=True,
                                         name="AcousticModel", output_names=["pred_acoustic_features"])
    torch.manual_seed(3)
    h = Handler()
    h.create_model(wrapped)
    h.set_optimiser("Adam", lr=1e-3)
    h.save_checkpoint(str(tmp_path), epoch=1, step=5)
    assert {"config.json", "params_e1"} <= set(os.listdir(str(tmp_path)))
    hp = ExtendedHParams.create_hparams()
    hp.use_gpu = True
    hp.optimiser_args["lr"] = 1e-3
    h2 = Handler()                       # the model is rebuilt from config.json
    h2.load_checkpoint(hp, str(tmp_path), epoch=1)
    assert repr(h2.model) == repr(h.model)
    sd, sd2 = h.model.state_dict(), h2.model.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k].cpu(), sd2[k].cpu()) for k in sd)
    group = [m for m in h2.model.modules() if isinstance(m, rnn_dyn.TransformerWrapper)][0]
    assert group.mask_padding and [type(m).__name__ for m in group.module] == ["TransformerEncoderLayer", "Dropout"] * 2
    assert group.module[0].p == 0.25 and group.module[0].norm_first and group.module[1].p == 0.125


def test_acoustic_model_trainer(gpu, golden_dir, tmp_path, attention_calls):
    """two epochs on the golden corpus with mask_padding=True and layer_dropout=0.1: finite, decreasing losses on the
    module path, and synthesis still runs"""
    from idiaptts_amd.src.model_trainers.AcousticModelTrainer import AcousticModelTrainer
    from idiaptts_amd.src.neural_networks.pytorch.models.NamedForwardWrapper import NamedForwardWrapper
    root = str(tmp_path)
    ids, wdir, qdir, _ = materialise(golden_dir, root)
    hp = AcousticModelTrainer.create_hparams()
    hp.num_questions = 409
    hp.voice = "full"
    hp.out_dir = os.path.join(root, "attention_train")
    hp.frame_size_ms = 5
    hp.num_coded_sps = 20
    hp.seed = 1234
    hp.epochs = 2
    hp.use_gpu = True
    hp.dataset_num_workers_gpu = 0
    hp.batch_first = True
    hp.batch_size_train = 2
    hp.batch_size_val = 50
    hp.use_saved_learning_rate = True
    hp.optimiser_args["lr"] = 0.001
    hp.model_name = "test_model"
    hp.epochs_per_checkpoint = 2
    hp.world_dir = wdir
    hp.use_best_as_final_model = False
    hp.synth_fs = 16000
    LC = rnn_dyn.Config.LayerConfig
    cfg = rnn_dyn.Config(in_dim=409, batch_first=True, layer_configs=[
        LC("Linear", out_dim=32, nonlin="Tanh"),
        LC("TransformerEncoderLayer", d_model=32, nhead=2, dim_feedforward=64, batch_first=True, mask_padding=True,
           layer_dropout=0.1),
        LC("Linear", out_dim=67)])
    model_config = NamedForwardWrapper.Config(wrapped_model_config=cfg, input_names=["questions"], batch_first=True,
                                              name="AcousticModel", output_names=["pred_acoustic_features"])
    trainer = AcousticModelTrainer(**AcousticModelTrainer.legacy_support_init(wdir, qdir, ids, hp.num_questions, hp))
    trainer.init(hp, model_config=model_config)
    all_loss, all_loss_train, handler = trainer.train(hp)
    assert handler._resident is None
    key = "MSELoss_acoustic_features"
    train, val = all_loss_train[key], all_loss[key]
    assert np.isfinite(train).all() and np.isfinite(val).all()
    assert len(train) == 2 and train[-1] < train[0], train
    assert attention_calls and all(c[1] for c in attention_calls)            # the kernel ran, with the lengths
    assert {c[2] for c in attention_calls} == {0.1, 0.0}                     # training and validation
    outputs, outputs_post = trainer.synth(hp, ids[:1])
    assert outputs[ids[0]]["pred_acoustic_features"].shape[1] == 67
    assert np.isfinite(outputs_post[ids[0]]["pred_acoustic_features"]).all()
