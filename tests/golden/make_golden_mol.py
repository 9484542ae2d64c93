"""Reference capture for the discretized mixture-of-logistics loss: the reference's DiscretizedMixturelogisticLoss
(loss/DiscretizedMixturelogisticLoss.py, loaded by its file: it imports with torch alone) run in float64 on the CPU
with autograd.  Writes tests/golden/mol_fixture.npz (data only), per case of mol_cases.GOLDEN_CASES -- K in {1, 10},
num_classes 256 and 65536, log_scale_min -7 and log(1e-14), shift None, 1 and 3, hinge on and off, B = 2, T = 12:

  <case>/x [B, 3K, T] float32, <case>/y [B, 1, T] float32 (mol_cases.inputs), <case>/w [B, T - shift] float64 row
  weights in 0.5 .. 1.5, <case>/elem [B, T - shift, 1] float64 (the module's return value, unweighted),
  <case>/grad [B, 3K, T] float64 = d sum(w elem) / d x.

The generator asserts that all four branches of the loss occur over the cases, and prints the share of each.
Usage: python tests/golden/make_golden_mol.py (needs the reference checkout)."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import mol_cases as mc  # noqa: E402


def reference_module():
    path = os.path.join(mg.REF, "idiaptts", "src", "neural_networks", "pytorch", "loss",
                        "DiscretizedMixturelogisticLoss.py")
    spec = importlib.util.spec_from_file_location("ref_mol_loss", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import torch
    ref = reference_module()
    out, counts = {}, np.zeros(4, dtype=np.int64)
    for n, case in enumerate(mc.GOLDEN_CASES):
        K, nc, lsm, shift, hinge = case
        x, y = mc.inputs(mc.GOLDEN_B, K, mc.GOLDEN_T, nc, lsm, shift, seed=n)
        Tn = mc.GOLDEN_T - (shift or 0)
        w = 0.5 + np.random.default_rng(500 + n).random((mc.GOLDEN_B, Tn))
        leaf = torch.from_numpy(x).double().requires_grad_(True)
        loss_fn = ref.DiscretizedMixturelogisticLoss(nc, lsm, shift=shift, hinge_loss=hinge)
        elem = loss_fn(leaf, torch.from_numpy(y).double())
        (elem[..., 0] * torch.from_numpy(w)).sum().backward()
        p = mc.case_name(*case) + "/"
        out[p + "x"], out[p + "y"], out[p + "w"] = x, y, w
        out[p + "elem"] = elem.detach().numpy()
        out[p + "grad"] = leaf.grad.numpy()
        counts += mc.branch_counts(x, y, nc, lsm, shift)
    print("entries per branch (low edge, high edge, cdf_delta > 1e-5, bin centre):", counts, counts / counts.sum())
    assert (counts > 0).all()
    path = os.path.join(HERE, "mol_fixture.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
