"""The raw-waveform kernels of csrc/mol.hip on the GPU: mu-law indices of all 65 536 PCM-16 values equal numpy's
exactly (tests/test_rawwave_host.py shows why that is a fair demand), the inverse to 1e-15 of full scale, one-hot
targets of a ragged batch between sentinels, the same bytes alone and in a list, sample_linearly against scipy's
interp1d, and two wav files from the reader into both losses."""
import numpy as np
import pytest
import torch
from scipy.interpolate import interp1d

import rawwave_cases as rc
from idiaptts_amd import ops
from idiaptts_amd.misc.utils import sample_linearly, sample_linearly_batch
from idiaptts_amd.src.data_preparation.audio.RawWaveformLabelGen import RawWaveformLabelGen
from idiaptts_amd.src.data_preparation.DataReaderConfig import DataReaderConfig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("mu", rc.MUS)
def test_mulaw_on_every_pcm16_value(mu):
    x = rc.pcm16_values()
    want = rc.mulaw_encode(x, mu)
    got = RawWaveformLabelGen.mu_law_companding(x, mu)
    assert got.dtype == np.int64 and got.shape == x.shape and np.array_equal(got, want)
    # as a ragged batch: the same indices at any place
    offsets = [0, 1, 3, 66, 1066, x.size]
    batch = ops.mulaw_encode(torch.from_numpy(x).to(DEV), offsets, mu).cpu().numpy()
    assert np.array_equal(batch, want)
    # decode(encode(x)) against the numpy restatement, to 1e-15 of the signal's scale
    back = RawWaveformLabelGen.mu_law_companding_reversed(got, mu)
    ref = rc.mulaw_decode(want, mu)
    assert back.dtype == np.float64
    err = np.abs(back - ref).max() / np.abs(ref).max()
    print("mu {}: decode error {:.3g} of full scale".format(mu, err))
    assert err <= 1e-15
    # a 2-D array keeps its shape
    assert RawWaveformLabelGen.mu_law_companding(x[:12].reshape(3, 4), mu).shape == (3, 4)


def _signals(lengths, seed=0):
    rng = np.random.default_rng(seed)
    return [np.clip(0.4 * rng.standard_normal(n), -1.0, 32767.0 / 32768.0) for n in lengths]


@pytest.mark.parametrize("mu", (255, 1023))
def test_onehot_batch_ragged_lengths_and_sentinels(mu):
    lengths = (1, 2, 63, 1000)
    signals = _signals(lengths)
    x = torch.from_numpy(np.concatenate(signals)).to(DEV)
    begins = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    rows, W, pad = sum(lengths), mu + 1, 1000
    buf = torch.full((rows * W + 2 * pad,), -7.0, dtype=torch.float32, device=DEV)
    out = buf[pad:pad + rows * W].view(rows, W)
    got, out_off = ops.mulaw_onehot(x, begins, lengths, mu, out=out)
    assert out_off == [0, 1, 3, 66, 1066] and got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:pad] == -7.0).all() and (host[-pad:] == -7.0).all()       # nothing outside the rows
    onehot = host[pad:-pad].reshape(rows, W)
    index = rc.mulaw_encode(np.concatenate(signals), mu)
    assert set(np.unique(onehot)) == {0.0, 1.0} and (onehot.sum(axis=1) == 1.0).all()
    assert np.array_equal(onehot.argmax(axis=1), index)
    # through the reader: a list of views, each equal to the file processed alone, byte for byte
    gen = RawWaveformLabelGen(mu=mu)
    batch = gen.preprocess_batch(signals)
    assert [tuple(b.shape) for b in batch] == [(n, W) for n in lengths] and all(b.is_cuda for b in batch)
    for s, b in zip(signals, batch):
        alone = gen.preprocess_sample(s)
        assert alone.dtype == np.float32 and alone.tobytes() == b.cpu().numpy().tobytes()
    # and back: arg-max and the inverse, times norm_params
    gen.set_normalisation_params(2.0)
    back = gen.postprocess_sample(batch[3].cpu().numpy())
    assert np.allclose(back, 2.0 * rc.mulaw_decode(index[66:], mu), rtol=0, atol=1e-14)


def test_silence_trim_in_the_batch():
    gen = RawWaveformLabelGen(mu=255, silence_threshold_quantized=20)
    quiet, loud = np.full(30, 1e-4), _signals((200,), seed=4)[0]
    loud[:2] = 0.0
    signals = [np.concatenate([quiet, loud, quiet]), np.concatenate([loud, quiet[:5]])]
    batch = gen.preprocess_batch(signals)
    for s, b in zip(signals, batch):
        index = rc.mulaw_encode(s, 255)
        start, end = RawWaveformLabelGen.start_and_end_indices(index, 20)
        assert 0 < end - start < len(s)
        assert np.array_equal(b.cpu().numpy().argmax(axis=1), index[start:end])
        assert gen.preprocess_sample(s).tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("m", (2, 80))
@pytest.mark.parametrize("D", (1, 5, 80))
def test_sample_linearly_against_interp1d(D, m):
    rng = np.random.default_rng(10 * D + m)
    samples = [rng.standard_normal((T, D)).astype(np.float32) * 3 for T in (2, 3, 201)]
    got = sample_linearly_batch(samples, m)
    assert all(g.is_cuda and g.dtype == torch.float32 for g in got)
    for s, g in zip(samples, got):
        T = len(s)
        ref = np.array(interp1d(np.arange(0.0, T), s, axis=0)(np.linspace(0.0, T - 1, m * T)), dtype=np.float32)
        g = g.cpu().numpy()
        assert g.shape == ref.shape == (m * T, D)
        assert np.array_equal(g[0], s[0]) and np.array_equal(g[-1], s[-1])         # first and last rows exact
        # every other element within one float32 ulp of interp1d's (its own last row, slope * 1 + y_lo with the slope
        # rounded to float32, misses the input's by up to hundreds of ulps where |y_hi| is far below |y_lo|)
        inner, ref_inner = g[1:-1].astype(np.float64), ref[1:-1]
        assert (np.abs(inner - ref_inner) <= np.spacing(np.abs(ref_inner))).all()
        print("sample_linearly T{} D{} m{}: {} of {} inner elements differ from interp1d's float32".format(
            T, D, m, int((inner != ref_inner).sum()), inner.size))
        # the single-utterance call: numpy in, numpy out, the same bytes
        alone = sample_linearly(s, m)
        assert isinstance(alone, np.ndarray) and alone.tobytes() == g.tobytes()
    # float64 in and out, a non-integer multiplier is truncated
    s = samples[2].astype(np.float64)
    out = sample_linearly(s, m + 0.9, dtype=np.float64)
    ref = interp1d(np.arange(0.0, 201), s, axis=0)(np.linspace(0.0, 200, m * 201))
    assert out.dtype == np.float64 and np.allclose(out, ref, rtol=0, atol=1e-14)


def test_reader_to_both_losses(tmp_path):
    from idiaptts_amd.src.neural_networks.pytorch.loss.DiscretizedMixturelogisticLoss import \
        DiscretizedMixturelogisticLoss
    from idiaptts_amd.src.neural_networks.pytorch.loss.OneHotCrossEntropyLoss import OneHotCrossEntropyLoss
    T = 300
    pcm = [rc.write_wav(str(tmp_path / "u{}.wav".format(n)), T, seed=n) for n in (1, 2)]
    g = torch.Generator().manual_seed(3)
    # mu-law classes against the one-hot loss
    reader = DataReaderConfig(name="raw", feature_type="RawWaveformLabelGen", directory=str(tmp_path), mu=255,
                              output_names=["wave"]).create_reader()
    items = [reader["u1"]["wave"], reader["u2"]["wave"]]
    for item, p in zip(items, pcm):
        assert item.shape == (T, 256) and np.array_equal(item.argmax(axis=1), rc.mulaw_encode(p / 32768.0, 255))
    target = torch.from_numpy(np.stack(items)).transpose(1, 2).contiguous()            # [B, 256, T]
    logits = torch.randn(2, 256, T, generator=g)
    loss_fn = OneHotCrossEntropyLoss(shift=1)
    gpu, cpu = loss_fn(logits.to(DEV), target.to(DEV)).cpu(), loss_fn(logits, target)
    assert gpu.shape == (2, T - 1, 1) and torch.isfinite(gpu).all()
    assert torch.allclose(gpu, cpu, rtol=2e-6, atol=2e-6)
    # the samples themselves against the mixture of logistics
    reader = DataReaderConfig(name="raw", feature_type="RawWaveformLabelGen", directory=str(tmp_path), mu=None,
                              output_names=["wave"]).create_reader()
    wave = torch.from_numpy(np.stack([reader["u1"]["wave"], reader["u2"]["wave"]])).transpose(1, 2).contiguous()
    assert wave.shape == (2, 1, T) and wave.dtype == torch.float32
    pred = torch.randn(2, 30, T, generator=g)
    pred[:, 20:] = pred[:, 20:] - 4.0
    loss_fn = DiscretizedMixturelogisticLoss(65536, float(np.log(1e-14)), shift=1)
    gpu, cpu = loss_fn(pred.to(DEV), wave.to(DEV)).cpu(), loss_fn(pred, wave)
    assert gpu.shape == (2, T - 1, 1) and torch.isfinite(gpu).all()
    assert torch.allclose(gpu, cpu, rtol=1e-5, atol=1e-5)
