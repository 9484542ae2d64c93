"""Reference capture for utterance embeddings: the PoolLast / PoolMean and VAE groups of rnn_dyn, VAEKLDLoss and an
EncDecDyn encoder + decoder chain, run on the CPU against the reference package with the stub harness of
make_golden.py.  Writes tests/golden/latent_fixture.npz (data only):

  <case>/x [B, T, D], <case>/lens [B], <case>/mask [B, T, 1], <case>/sd/<key> (state dict), <case>/eps (what the
  model's one torch.randn_like call returned), <case>/z, /mu, /log_var, <case>/out_lens, <case>/out_max_len,
  <case>/kl_steps and <case>/kl (VAEKLDLoss, annealing_points (-1, 100), annealing_steps 10, mask = the frame mask,
  'mean_per_frame', at each of the steps), <case>/gz (a weight tensor of z's shape) and <case>/grad/<key>: the
  parameter gradients of  KL(step 10) + sum(z * gz).
  cases: gru_poollast_vae  GRU(8) -> PoolLast -> VAE(4) on 6 inputs
         lin_poolmean_vae  Linear(6, Tanh) -> PoolMean -> VAE(3) on 5 inputs
         frame_vae         VAE(4) on 67 inputs, one latent per frame (the model of the reference's test_vaekld_loss)
  chain/: questions [B, T, 9], acoustic_features [B, T, 6], lens, mask, sd/<key> of an EncDecDyn of
         encoder  (GRU(8) -> PoolLast -> VAE(4) on acoustic_features -> emb_z, emb_mu, emb_logvar) and
         decoder  (Linear(16, Tanh) -> Linear(6) on [questions, emb_z] -> pred_acoustic_features),
         eps, emb_z, pred, mse (NamedLoss MSELoss 'mean_per_frame'), kl (as above, step 10), grad/<key> of mse + kl.
         (absent when the reference's enc_dec_dyn package does not import under the stubs; the generator says so)

torch.randn_like is wrapped HERE, around the reference's forward, never inside the reference.
Usage: python tests/golden/make_golden_latent.py (needs the reference checkout)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

KL_STEPS = (0, 5, 10, 50, 100, 110)


class RecordRandn:
    """records what torch.randn_like returns while active"""

    def __enter__(self):
        import torch
        self.torch, self.orig, self.draws = torch, torch.randn_like, []

        def randn_like(*args, **kwargs):
            out = self.orig(*args, **kwargs)
            self.draws.append(out.clone())
            return out
        torch.randn_like = randn_like
        return self

    def __exit__(self, *exc):
        self.torch.randn_like = self.orig


def _mask(lens, T):
    import torch
    return (torch.arange(T)[None, :] < lens[:, None]).float().unsqueeze(-1)


def _kl_config(VAEKLDLoss, mask_name):
    return VAEKLDLoss.Config(name="VAEKLD_loss", type_="VAEKLDLoss", input_names=["emb_mu", "emb_logvar"],
                             seq_mask=mask_name, start_step=0, annealing_points=(-1, 100), annealing_steps=10,
                             batch_first=True)


def capture_single(out, case, in_dim, layer_configs, lens, seed):
    import torch
    from idiaptts.src.neural_networks.pytorch.loss.VAEKLDLoss import VAEKLDLoss
    from idiaptts.src.neural_networks.pytorch.models import rnn_dyn
    torch.manual_seed(seed)
    lens = torch.tensor(lens, dtype=torch.int64)
    B, T = len(lens), int(lens.max())
    model = rnn_dyn.Config(in_dim=in_dim, batch_first=True, layer_configs=layer_configs).create_model()
    for p in model.parameters():            # away from the small default initialisation: the KL term has a gradient
        p.data.mul_(2.0)
    x = torch.randn(B, T, in_dim) + 0.5
    mask = _mask(lens, T)
    x = x * mask                            # zero padding, as the handler's pad_sequence leaves it
    p = case + "/"
    out[p + "x"], out[p + "lens"], out[p + "mask"] = x.numpy(), lens.numpy(), mask.numpy()
    for k, v in model.state_dict().items():
        out[p + "sd/" + k] = np.array(v.numpy(), copy=True)
    model.init_hidden(B)
    with RecordRandn() as rec:
        (z, mu, log_var), kwargs = model(x, seq_lengths_input=lens.clone(), max_length_inputs=torch.tensor(T))
    assert len(rec.draws) == 1 and rec.draws[0].shape == z.shape
    out[p + "eps"] = rec.draws[0].numpy()
    out[p + "z"], out[p + "mu"], out[p + "log_var"] = (t.detach().numpy() for t in (z, mu, log_var))
    out[p + "out_lens"] = np.asarray(kwargs["seq_lengths_input"])
    out[p + "out_max_len"] = np.asarray(int(kwargs["max_length_inputs"]))
    loss_fn = _kl_config(VAEKLDLoss, "mask").create_loss()
    data = {"emb_mu": mu, "emb_logvar": log_var, "mask": mask}
    kls = [float(loss_fn(dict(data), {"mask": lens}, step)["VAEKLD_loss"]) for step in KL_STEPS]
    out[p + "kl_steps"], out[p + "kl"] = np.asarray(KL_STEPS), np.asarray(kls, dtype=np.float64)
    gz = torch.randn(z.shape)
    out[p + "gz"] = gz.numpy()
    total = loss_fn(dict(data), {"mask": lens}, 10)["VAEKLD_loss"] + (z * gz).sum()
    total.backward()
    for k, v in model.named_parameters():
        out[p + "grad/" + k] = v.grad.numpy()
    print(case, "z", tuple(z.shape), "out_lens", out[p + "out_lens"], "kl", kls)


def capture_chain(out, seed=7):
    import torch
    from idiaptts.src.neural_networks.pytorch.loss.NamedLoss import NamedLoss
    from idiaptts.src.neural_networks.pytorch.loss.VAEKLDLoss import VAEKLDLoss
    from idiaptts.src.neural_networks.pytorch.models import rnn_dyn
    from idiaptts.src.neural_networks.pytorch.models import enc_dec_dyn
    LC = rnn_dyn.Config.LayerConfig
    torch.manual_seed(seed)
    lens = torch.tensor([9, 4, 7], dtype=torch.int64)
    B, T, Q, A, L = 3, 9, 9, 6, 4
    config = enc_dec_dyn.Config(modules=[
        enc_dec_dyn.Config.ModuleConfig(
            name="encoder", input_names=["acoustic_features"], process_group=0,
            output_names=["emb_z", "emb_mu", "emb_logvar"],
            config=rnn_dyn.Config(in_dim=A, batch_first=True, layer_configs=[
                LC("GRU", out_dim=8), LC("PoolLast", batch_first=True), LC("VAE", out_dim=L)])),
        enc_dec_dyn.Config.ModuleConfig(
            name="decoder", input_names=["questions", "emb_z"], process_group=1,
            output_names=["pred_acoustic_features"],
            config=rnn_dyn.Config(in_dim=Q + L, batch_first=True, layer_configs=[
                LC("Linear", out_dim=16, nonlin="Tanh"), LC("Linear", out_dim=A)]))])
    model = config.create_model()
    for p in model.parameters():
        p.data.mul_(2.0)
    mask = _mask(lens, T)
    questions = (torch.randn(B, T, Q) > 0.3).float() * mask
    acoustic = (torch.randn(B, T, A) + 0.5) * mask
    p = "chain/"
    out[p + "questions"], out[p + "acoustic_features"] = questions.numpy(), acoustic.numpy()
    out[p + "lens"], out[p + "mask"] = lens.numpy(), mask.numpy()
    for k, v in model.state_dict().items():
        out[p + "sd/" + k] = np.array(v.numpy(), copy=True)
    data = {"questions": questions, "acoustic_features": acoustic, "acoustic_features_mask": mask}
    lengths = {"questions": lens.clone(), "acoustic_features": lens.clone(), "acoustic_features_mask": lens.clone()}
    max_lengths = {k: torch.tensor(T) for k in lengths}
    model.init_hidden(B)
    with RecordRandn() as rec:
        model(data, lengths, max_lengths)
    assert len(rec.draws) == 1
    out[p + "eps"] = rec.draws[0].numpy()
    out[p + "emb_z"] = data["emb_z"].detach().numpy()
    out[p + "pred"] = data["pred_acoustic_features"].detach().numpy()
    mse = NamedLoss.Config(name="MSELoss_acoustic_features", type_="MSELoss", seq_mask="acoustic_features_mask",
                           input_names=["acoustic_features", "pred_acoustic_features"], batch_first=True).create_loss()
    kld = _kl_config(VAEKLDLoss, "acoustic_features_mask").create_loss()
    length_dict = {"acoustic_features_mask": lens}
    l_mse = mse(data, length_dict, 10)["MSELoss_acoustic_features"]
    l_kl = kld(data, length_dict, 10)["VAEKLD_loss"]
    out[p + "mse"], out[p + "kl"] = np.asarray(float(l_mse)), np.asarray(float(l_kl))
    (l_mse + l_kl).backward()
    for k, v in model.named_parameters():
        out[p + "grad/" + k] = v.grad.numpy()
    print("chain: keys", [k for k, _ in model.named_parameters()], "mse", float(l_mse), "kl", float(l_kl))


def _main():
    mg.install_stub_harness()
    from idiaptts.src.neural_networks.pytorch.models import rnn_dyn
    LC = rnn_dyn.Config.LayerConfig
    out = {}
    capture_single(out, "gru_poollast_vae", 6,
                   [LC("GRU", out_dim=8), LC("PoolLast", batch_first=True), LC("VAE", out_dim=4)], [11, 1, 7, 11, 5], 1)
    capture_single(out, "lin_poolmean_vae", 5,
                   [LC("Linear", out_dim=6, nonlin="Tanh"), LC("PoolMean", batch_first=True), LC("VAE", out_dim=3)],
                   [3, 13, 8, 1], 2)
    capture_single(out, "frame_vae", 67, [LC("VAE", out_dim=4)], [10, 6, 3], 3)
    try:
        capture_chain(out)
    except ImportError as e:
        print("chain NOT captured: the reference's enc_dec_dyn does not import under the stubs:", e)
    path = os.path.join(HERE, "latent_fixture.npz")
    np.savez_compressed(path, **out)
    print("latent_fixture.npz:", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    _main()
