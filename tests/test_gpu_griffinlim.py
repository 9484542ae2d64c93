"""Griffin-Lim on the GPU (csrc/griffinlim.hip) against the numpy restatement of librosa.griffinlim
(tests/griffinlim_spec.py), and through the public surface (AudioProcessing.amp_sp_to_raw, Synthesiser.run_griffin_lim /
run_griffin_lim_on_log, ModularTrainer.gen_waveform with "GL" / "GL_on_log")."""
import os
import types

import numpy as np
import pytest
import scipy.io.wavfile
import scipy.signal

import griffinlim_spec as gl
from idiaptts_amd import world

pytestmark = pytest.mark.gpu


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    return np.abs(got - ref).max() / np.abs(ref).max()


def _spectrum(name, golden_dir, hop, n_fft, seconds=None):
    from idiaptts_amd.src.data_preparation.audio.AudioProcessing import AudioProcessing
    from idiaptts_amd.synthetic_audio import make_audio
    if name == "synthetic22050":
        raw = make_audio(22050, 1.5, 11)
    else:
        raw, fs = AudioProcessing.get_raw(os.path.join(golden_dir, name + ".wav"))
        if seconds is not None:
            raw = raw[:int(seconds * fs)]
    return np.abs(gl.stft(raw, hop, n_fft))


CASES = [("LJ001-0001", 1024, 80), ("p225_001", 2048, 240), ("synthetic22050", 1024, 110)]


@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
@pytest.mark.parametrize("name,n_fft,hop", CASES)
def test_float64_matches_spec(name, n_fft, hop, pad_mode, gpu, golden_dir):
    S = _spectrum(name, golden_dir, hop, n_fft)
    y = world.griffinlim(S.T, n_iter=60, hop_length=hop, pad_mode=pad_mode, random_state=17)
    assert y.dtype == np.float64 and len(y) == hop * (S.shape[0] - 1)
    ref = gl.griffinlim(S, gl.init_phases(S.shape, 17), 60, hop, pad_mode=pad_mode)
    assert _rel(y, ref) <= 1e-9


@pytest.mark.parametrize("name,n_fft,hop", CASES[:2])
def test_float32_matches_complex64_spec(name, n_fft, hop, gpu, golden_dir):
    S = _spectrum(name, golden_dir, hop, n_fft, seconds=3.0).astype(np.float32)
    a0 = gl.init_phases(S.shape, 5)
    y1 = world.griffinlim(S.T, n_iter=1, hop_length=hop, random_state=5)
    assert y1.dtype == np.float32
    r1 = _rel(y1, gl.griffinlim(S, a0, 1, hop, c64=True))
    assert r1 <= 1e-6, r1
    y60 = world.griffinlim(S.T, n_iter=60, hop_length=hop, random_state=5)
    ref60 = gl.griffinlim(S, a0, 60, hop, c64=True)
    r60 = _rel(y60, ref60)
    assert r60 <= 1e-4, r60
    sc, sc_ref = gl.spectral_convergence(S, y60, hop), gl.spectral_convergence(S, ref60, hop)
    assert abs(sc - sc_ref) <= 1e-4 * sc_ref, (sc, sc_ref)


def test_spectral_convergence_does_not_increase_without_momentum(gpu, golden_dir):
    S = _spectrum("LJ001-0001", golden_dir, 80, 1024)
    sc = [gl.spectral_convergence(S, world.griffinlim(S.T, n_iter=n, hop_length=80, momentum=0.0, random_state=2),
                                  80) for n in range(1, 9)]
    assert all(b <= a for a, b in zip(sc[:-1], sc[1:])), sc


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ragged_batch_equals_single_calls_bit_for_bit(dtype, gpu):
    from idiaptts_amd import lib
    F = lib.load().itts_griffinlim_tile_frames(1024, 80)
    assert F > 8
    lengths = [2, 3, F // 2 + 1, F, 2 * F, 7 * F + 5, 1999, 3 * F + 1]
    rng = np.random.default_rng(0)
    spectra = [(rng.random((t, 513)) ** 3).astype(dtype) for t in lengths]
    kw = dict(n_iter=7, hop_length=80)
    batch = world.griffinlim_batch(spectra, random_state=np.random.RandomState(3), **kw)
    again = world.griffinlim_batch(spectra, random_state=np.random.RandomState(3), **kw)
    rs = np.random.RandomState(3)
    single = [world.griffinlim_batch([sp], random_state=rs, **kw)[0] for sp in spectra]
    for t, b, a, s in zip(lengths, batch, again, single):
        assert b.dtype == dtype and len(b) == 80 * (t - 1)
        assert np.array_equal(b, a) and np.array_equal(b, s), t
    # and the short ones against the restatement
    phases = world.griffinlim_init_phases([sp.shape for sp in spectra], "random", np.random.RandomState(3))
    for sp, a0, b in list(zip(spectra, phases, batch))[:4]:
        assert _rel(b, gl.griffinlim(sp, a0, 7, 80, c64=dtype == np.float32)) <= (1e-9 if dtype == np.float64
                                                                                  else 1e-4)


def test_amp_sp_to_raw_matches_reference(gpu, golden_dir):
    from idiaptts_amd.src.data_preparation.audio.AudioProcessing import AudioProcessing
    raw, fs = AudioProcessing.get_raw(os.path.join(golden_dir, "LJ001-0001.wav"))
    amp = AudioProcessing.librosa_extract_amp_sp(raw, fs)
    np.random.seed(123)
    y = AudioProcessing.amp_sp_to_raw(amp, fs, preemphasis=0.97)
    # reference :279-289: griffinlim(amp_sp.T * sqrt(K), hop_length=80) with np.random's phases, then depreemphasis
    np.random.seed(123)
    S = amp * np.sqrt(amp.shape[1])
    a0 = np.exp(2j * np.pi * np.random.rand(*S.T.shape)).T
    ref = scipy.signal.lfilter([1], [1, -0.97], gl.griffinlim(S, a0, 32, 80))
    assert _rel(y, ref) <= 1e-9


def _hparams(tmp_path, **kw):
    hp = types.SimpleNamespace(synth_fs=16000, hop_size_ms=5, win_length_ms=None, out_dir=str(tmp_path),
                               model_name="m", synth_file_suffix="_gl", synth_ext="wav", griffin_lim_iters=20,
                               synth_vocoder="GL")
    hp.__dict__.update(kw)
    return hp


def _expected_pcm(outputs, seed, n_iter=20, power=1.2, hop=80, preemphasis=0.0):
    np.random.seed(seed)
    res = []
    for out in outputs:
        S = out.astype(np.float64) ** power if out.dtype == np.float64 else out ** power
        a0 = np.exp(2j * np.pi * np.random.rand(*S.T.shape)).T
        y = gl.griffinlim(S, a0, n_iter, hop, c64=out.dtype == np.float32)
        if preemphasis:
            y = scipy.signal.lfilter([1], [1, -preemphasis], y)
        res.append(y)
    return res


def _check_wav(path, ref, exact=True):
    fs, pcm = scipy.io.wavfile.read(path)
    assert fs == 16000 and pcm.dtype == np.int16 and len(pcm) == len(ref)
    expect = np.clip(ref * 32768.0, -32768, 32767).astype(np.int16)
    diff = np.abs(pcm.astype(np.int32) - expect.astype(np.int32))
    # the restatement equals the kernel to 1e-9 relative: at most a sample on a truncation boundary moves by one
    assert diff.max() <= 1 and (diff > 0).sum() <= (0 if exact else 2)


def test_run_griffin_lim_writes_reference_files(gpu, golden_dir, tmp_path):
    from idiaptts_amd.src.Synthesiser import Synthesiser
    amp = {n: np.abs(gl.stft(_raw(golden_dir, n), 80, 1024)) / np.sqrt(513) * 4 for n in ("LJ001-0002", "LJ001-0003")}
    hp = _hparams(tmp_path, preemphasis=0.5)
    np.random.seed(9)
    wavs = Synthesiser.run_griffin_lim(dict(amp), hp, return_waveforms=True)
    refs = _expected_pcm(list(amp.values()), 9, preemphasis=0.5)
    for (name, ref) in zip(amp, refs):
        assert _rel(wavs[name], ref) <= 1e-9
        _check_wav(os.path.join(str(tmp_path), "m", "synth", name + "_m_gl.wav"), ref)
    # on log: db_to_amp first; no model name in the file name with use_model_name=False
    log_amp = {n: 20 * np.log10(np.maximum(1e-5, a)) for n, a in amp.items()}
    np.random.seed(9)
    Synthesiser.run_griffin_lim_on_log(log_amp, _hparams(tmp_path, synth_dir=str(tmp_path / "s")), epoch=1,
                                       use_model_name=False)
    refs = _expected_pcm([np.power(10.0, a * 0.05) for a in log_amp.values()], 9)
    for name, ref in zip(amp, refs):
        _check_wav(os.path.join(str(tmp_path), "s", name + "_gl.wav"), ref)


def _raw(golden_dir, name):
    from idiaptts_amd.src.data_preparation.audio.AudioProcessing import AudioProcessing
    return AudioProcessing.get_raw(os.path.join(golden_dir, name + ".wav"))[0]


@pytest.mark.parametrize("vocoder", ["GL", "GL_on_log"])
def test_gen_waveform_routes_griffin_lim(vocoder, gpu, golden_dir, tmp_path):
    from idiaptts_amd.src.model_trainers.ModularTrainer import ModularTrainer
    amp = (np.abs(gl.stft(_raw(golden_dir, "LJ001-0004"), 80, 1024)) / np.sqrt(513) * 4).astype(np.float32)
    out = 20 * np.log10(np.maximum(np.float32(1e-5), amp)) if vocoder == "GL_on_log" else amp
    hp = _hparams(tmp_path, synth_vocoder=vocoder, griffin_lim_iters=10)
    trainer = types.SimpleNamespace(total_epoch=2, total_steps=40)
    np.random.seed(4)
    ModularTrainer.gen_waveform(trainer, ["LJ001-0004"], {"LJ001-0004": out}, hp)
    src = np.power(10.0, out * 0.05) if vocoder == "GL_on_log" else out
    ref = _expected_pcm([src], 4, n_iter=10)[0]
    path = os.path.join(str(tmp_path), "m", "synth", "e2", "LJ001-0004_m_gl.wav")
    fs, pcm = scipy.io.wavfile.read(path)
    expect = np.clip(ref * 32768.0, -32768, 32767).astype(np.int16)
    assert len(pcm) == len(expect)
    # float32 state: the kernel equals the complex64 restatement to ~1e-6, a few samples may round across
    assert np.abs(pcm.astype(np.int32) - expect).max() <= 2
