"""tests/encdec_spec.py, the float64 restatement the GPU tests of the decoder compare with, held to the reference's own
float64 outputs in tests/golden/decoder_fixture.npz: 1e-12 relative (the margin of the mixture-of-logistics
restatement; the capture ran the reference in float64)."""
import numpy as np
import torch

import encdec_spec as spec

FIX = spec.load_fixture()
F64 = torch.float64


def _close(what, got, ref):
    ref = torch.as_tensor(np.asarray(ref))
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    rel = (got - ref).norm().item() / (ref.norm().item() + 1e-300)
    assert rel < 1e-12, (what, rel)


def _inputs():
    inputs = spec.tensors(spec.sub(FIX, "in/"), F64)
    return inputs, torch.as_tensor(FIX["in/frame_lens"])


def test_case1_parallel_decoder():
    inputs, lens = _inputs()
    out = spec.case1(spec.tensors(spec.sub(FIX, "case1/sd/"), F64), inputs, lens)
    ref = spec.sub(FIX, "case1/out/")
    assert sorted(out) == sorted(ref)
    for k in ref:
        _close(k, out[k], ref[k])


def test_case2_batched_outputs_loss_and_gradients():
    inputs, lens = _inputs()
    sd = spec.tensors(spec.sub(FIX, "case2/sd/"), F64)
    names = [str(n) for n in FIX["case2/param_names"]]
    for n in names:
        sd[n].requires_grad_(True)
    out = spec.decoder_batched(sd, inputs, lens)
    ref = spec.sub(FIX, "case2/out/")
    assert sorted(out) == sorted(ref)
    for k in ref:
        _close(k, out[k].detach(), ref[k])
    loss = spec.mse(out["pred_acoustic_features"], inputs["acoustic_features"], inputs["mask"])
    assert abs(loss.item() - float(FIX["case2/mse"])) < 1e-12 * abs(float(FIX["case2/mse"]))
    loss.backward()
    for n in names:
        _close("grad " + n, sd[n].grad, FIX["case2/grad/" + n])


def test_case3_inference_and_case4_scheduled_sampling():
    inputs, _ = _inputs()
    sd = spec.tensors(spec.sub(FIX, "case2/sd/"), F64)
    out = spec.decoder_iterative(sd, inputs, with_target=False)
    for k, ref in spec.sub(FIX, "case3/out/").items():
        _close("case3 " + k, out[k], ref)
    draws = [float(d) for d in FIX["case4/draws"]]
    assert len(draws) == 3 and draws[0] <= 0.5 < draws[1]         # both branches of the loop are taken
    out = spec.decoder_iterative(sd, inputs, with_target=True, p_teacher_forcing=0.5, draws=draws)
    for k, ref in spec.sub(FIX, "case4/out/").items():
        _close("case4 " + k, out[k], ref)


def test_partial_last_chunk_is_the_mean_of_the_rows_it_has():
    A, enc = (torch.as_tensor(FIX["quirk/partial/" + k]) for k in ("A", "enc"))
    ctx, abar = spec.attention(A, enc, 5, partial_last=True)
    assert ctx.shape[1] == 2
    _close("ctx", ctx[:, 1:2], FIX["quirk/partial/ctx5"])
    _close("w", abar[:, 1:2], FIX["quirk/partial/w5"])
    assert bool(FIX["quirk/partial/empty_is_nan"])                # what the reference does past the last frame
