"""CPU checks of Griffin-Lim: the numpy restatement (tests/griffinlim_spec.py) reconstructs exactly and lowers the
spectral convergence without momentum, the host draws librosa's initial phases, and every argument refusal happens
before any device work."""
import os

import numpy as np
import pytest

import griffinlim_spec as gl
import stft_spec
from idiaptts_amd import world
from idiaptts_amd.synthetic_audio import make_audio


def _case(name, golden_dir):
    from idiaptts_amd.src.data_preparation.audio.AudioProcessing import AudioProcessing
    if name == "synthetic22050":
        return make_audio(22050, 1.0, 5), 22050
    raw, fs = AudioProcessing.get_raw(os.path.join(golden_dir, name + ".wav"))
    return raw, fs


CASES = [("LJ001-0001", 1024, 80), ("LJ001-0001", 1024, 110), ("p225_001", 2048, 240)]


@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
@pytest.mark.parametrize("name,n_fft,hop", CASES)
def test_istft_inverts_stft(name, n_fft, hop, pad_mode, golden_dir):
    x, _ = _case(name, golden_dir)
    X = gl.stft(x, hop, n_fft, pad_mode=pad_mode)
    T = X.shape[0]
    assert T == 1 + len(x) // hop
    y = gl.istft(X, hop, n_fft)
    assert len(y) == hop * (T - 1)
    assert np.abs(y - x[:len(y)]).max() <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("name,n_fft,hop", CASES)
def test_spectral_convergence_does_not_increase_without_momentum(name, n_fft, hop, golden_dir):
    x, _ = _case(name, golden_dir)
    x = x[:int(0.8 * len(x))] if len(x) > 40000 else x
    S = np.abs(gl.stft(x, hop, n_fft))
    a0 = gl.init_phases(S.shape, 3)
    sc = [gl.spectral_convergence(S, gl.griffinlim(S, a0, n, hop, momentum=0.0), hop) for n in range(1, 11)]
    assert all(b <= a for a, b in zip(sc[:-1], sc[1:])), sc
    assert sc[-1] < sc[0] - 0.02, sc


def test_window_sumsquare_matches_frames():
    win = stft_spec.window(1024)
    wss = gl.window_sumsquare(win, 5, 80, 1024)
    assert len(wss) == 1024 + 4 * 80
    assert wss[500] == pytest.approx(sum(win[500 - t * 80] ** 2 for t in range(5)), rel=1e-15)


def test_initial_phases_match_librosa_draws():
    shapes = [(7, 513), (3, 513), (11, 513)]
    got = world.griffinlim_init_phases(shapes, "random", np.random.RandomState(5))
    rng = np.random.RandomState(5)
    for (T, K), g in zip(shapes, got):
        ref = np.exp(2j * np.pi * rng.rand(K, T)).T
        assert g.shape == (T, K) and np.array_equal(g, ref)
    single = world.griffinlim_init_phases([(7, 513)], "random", np.random.RandomState(5))[0]
    assert np.array_equal(single, np.exp(2j * np.pi * np.random.RandomState(5).rand(513, 7)).T)
    c64 = world.griffinlim_init_phases([(7, 513)], "random", np.random.RandomState(5), np.complex64)[0]
    assert c64.dtype == np.complex64 and np.array_equal(c64, single.astype(np.complex64))
    ones = world.griffinlim_init_phases([(4, 513)], None, None)[0]
    assert np.array_equal(ones, np.ones((4, 513)))
    # the rng of random_state: np.random for None, a fresh RandomState for an int, the given one otherwise
    assert world.griffinlim_args(513, [4], random_state=None)[3] is np.random
    rs = np.random.RandomState(1)
    assert world.griffinlim_args(513, [4], random_state=rs)[3] is rs
    assert world.griffinlim_args(513, [4], random_state=9)[3].rand() == np.random.RandomState(9).rand()
    assert world.griffinlim_args(513, [4])[:3] == (1024, 256, 1024)
    assert world.griffinlim_args(1025, [4], hop_length=240, win_length=1200)[:3] == (2048, 240, 1200)


@pytest.mark.parametrize("K", [257, 2049])
def test_refuses_other_fft_sizes(K, monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError, match=str(2 * (K - 1))):
        world.griffinlim(np.ones((K, 10)))


def _no_device(monkeypatch):
    def fail(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(world, "_device", fail)
    monkeypatch.setattr(world.ops, "griffinlim", fail)


@pytest.mark.parametrize("kwargs,exc", [(dict(window="hamming"), NotImplementedError),
                                        (dict(center=False), NotImplementedError),
                                        (dict(length=1000), NotImplementedError),
                                        (dict(pad_mode="edge"), NotImplementedError),
                                        (dict(momentum=-0.1), ValueError),
                                        (dict(init="foo"), ValueError),
                                        (dict(random_state="seed"), ValueError)])
def test_refusals_before_device_work(kwargs, exc, monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(exc):
        world.griffinlim(np.ones((513, 10)), **kwargs)


def test_one_frame_raises_and_momentum_above_one_warns(monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        world.griffinlim(np.ones((513, 1)))
    with pytest.raises(ValueError):
        world.griffinlim_batch([np.ones((10, 513)), np.ones((1, 513))])
    with pytest.warns(UserWarning):
        world.griffinlim_args(513, [4], momentum=1.5)
