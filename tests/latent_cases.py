"""The cases of tests/golden/latent_fixture.npz (written by tests/golden/make_golden_latent.py against the reference,
read by tests/test_latent_config.py and tests/test_gpu_latent_model.py), the configs that rebuild its models here,
and the float64 restatements and bounds of the kernel tests (tests/test_gpu_latent.py)."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latent_fixture.npz")

# name -> (in_dim, groups as (type, out_dim, nonlin, kwargs with batch_first left to the model's layout))
SINGLE = {
    "gru_poollast_vae": (6, [("GRU", 8, None, {}), ("PoolLast", None, None, "bf"), ("VAE", 4, None, {})]),
    "lin_poolmean_vae": (5, [("Linear", 6, "Tanh", {}), ("PoolMean", None, None, "bf"), ("VAE", 3, None, {})]),
    "frame_vae": (67, [("VAE", 4, None, {})]),
}
KL_ARGS = dict(annealing_points=(-1, 100), annealing_steps=10, start_step=0)     # the generator's VAEKLDLoss


def load_fixture():
    return np.load(FIXTURE)


def sub(fix, prefix):
    """{key without the prefix: array} of the fixture entries under `prefix`"""
    return {k[len(prefix):]: fix[k] for k in fix.files if k.startswith(prefix)}


def single_config(rnn_dyn, name, batch_first=True):
    in_dim, groups = SINGLE[name]
    LC = rnn_dyn.Config.LayerConfig
    layers = [LC(t, out_dim=d, nonlin=a, **(dict(batch_first=batch_first) if kw == "bf" else kw))
              for t, d, a, kw in groups]
    return rnn_dyn.Config(in_dim=in_dim, batch_first=batch_first, layer_configs=layers)


def chain_config(enc_dec_dyn, rnn_dyn):
    LC = rnn_dyn.Config.LayerConfig
    return enc_dec_dyn.Config(modules=[
        enc_dec_dyn.Config.ModuleConfig(
            name="decoder", input_names=["questions", "emb_z"], process_group=1,
            output_names=["pred_acoustic_features"],
            config=rnn_dyn.Config(in_dim=9 + 4, batch_first=True, layer_configs=[
                LC("Linear", out_dim=16, nonlin="Tanh"), LC("Linear", out_dim=6)])),
        enc_dec_dyn.Config.ModuleConfig(
            name="encoder", input_names=["acoustic_features"], process_group=0,
            output_names=["emb_z", "emb_mu", "emb_logvar"],
            config=rnn_dyn.Config(in_dim=6, batch_first=True, layer_configs=[
                LC("GRU", out_dim=8), LC("PoolLast", batch_first=True), LC("VAE", out_dim=4)]))])


# ---- kernel tests: the dense layers' bounds (tests/lnorm_cases.py: check) -------------------------------------------
REL_BOUND, ELEM_BOUND = 2e-6, 2e-5


def check(what, got, ref):
    """asserts `got` against the float64 `ref`: 2e-6 relative in the 2-norm, 2e-5 * max(1, max|ref|) per element;
    returns the two errors as fractions of their tolerance"""
    d = (got.double().cpu() - ref.cpu()).abs()
    rel = d.norm().item() / (ref.norm().item() + 1e-30)
    el = d.max().item() / max(1.0, ref.abs().max().item()) if d.numel() else 0.0
    print("latent {}: rel {:.3g} ({:.2f} of tol), elem {:.3g} ({:.2f} of tol)".format(
        what, rel, rel / REL_BOUND, el, el / ELEM_BOUND))
    assert rel < REL_BOUND and el < ELEM_BOUND, (what, rel, el)
    return rel / REL_BOUND, el / ELEM_BOUND


def pool64(torch, x, lens, batch_first, mean):
    """float64 restatement of the pooling: x [B, T, D] / [T, B, D] -> [B, D]"""
    x = x.double()
    if not batch_first:
        x = x.transpose(0, 1)
    B, T, _ = x.shape
    if mean:
        return x.sum(dim=1) / lens.double()[:, None]
    idx = lens - 1 if lens is not None else torch.full((B,), T - 1, dtype=torch.int64)
    return x[torch.arange(B), idx]


def pool64_bwd(torch, dy, lens, T, batch_first, mean):
    """.. and of its backward: dy [B, D] -> dx [B, T, D] / [T, B, D]"""
    dy = dy.double()
    B, D = dy.shape
    if mean:
        dx = (dy / lens.double()[:, None])[:, None, :].expand(B, T, D).clone()
    else:
        dx = torch.zeros(B, T, D, dtype=torch.float64)
        idx = lens - 1 if lens is not None else torch.full((B,), T - 1, dtype=torch.int64)
        dx[torch.arange(B), idx] = dy
    return dx if batch_first else dx.transpose(0, 1).contiguous()


def kl64(mu, log_var):
    """0.5 * sum_c (exp(lv) + mu^2 - 1 - lv) per row, float64"""
    mu, lv = mu.double(), log_var.double()
    return 0.5 * (lv.exp() + mu ** 2 - 1.0 - lv).sum(dim=-1)
