"""Corpus audio preparation without a GPU: the numpy restatements (tests/audio_prep_spec.py) against scipy, the trim
arithmetic of SilenceRemover on hand-made RMS tracks, the class and command-line signatures of the reference, the
refusals of the C boundary (ITTS_E_INVALID naming the value before any device work: the pointers handed in are null
or bogus) and the ValueErrors of the Python surface."""
import ctypes
import inspect
import logging
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.signal
from scipy.io import wavfile

from idiaptts_amd import lib
from tests import audio_prep_spec as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(64)       # never dereferenced: every call below is refused or empty
SYMBOLS = ("itts_fir_filtfilt_workspace_bytes", "itts_fir_filtfilt_batch", "itts_resample_poly_batch",
           "itts_loudness_normalise_batch", "itts_frame_rms_batch")


def _off(*values):
    return (ctypes.c_int64 * len(values))(*values)


# ------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("numtaps,n", [(11, 34), (11, 35), (101, 1000), (1001, 3004), (1001, 3500), (1001, 20000)])
def test_filtfilt_restatement_equals_scipy(numtaps, n):
    rng = np.random.default_rng(numtaps + n)
    b = scipy.signal.firls(numtaps, (0, 70, 100, 8000), (0, 0, 1, 1), fs=16000)
    x = rng.standard_normal(n) * 0.1 + 0.05
    got, ref = spec.filtfilt_spec(b, x), scipy.signal.filtfilt(b, [1], x)
    err, bound = np.abs(got - ref).max(), spec.filtfilt_bound(b, x)
    print("numtaps {} n {}: max abs {:.3g}, bound {:.3g}, identical bits: {}".format(
        numtaps, n, err, bound, np.array_equal(got, ref)))
    assert got.shape == ref.shape and err <= bound


def test_filtfilt_restatement_refuses_as_scipy_does():
    b = np.ones(11) / 11
    with pytest.raises(ValueError) as ours:
        spec.filtfilt_spec(b, np.zeros(33))
    with pytest.raises(ValueError) as theirs:
        scipy.signal.filtfilt(b, [1], np.zeros(33))
    assert str(ours.value) == str(theirs.value)


@pytest.mark.parametrize("up,down", [(1, 3), (160, 441), (320, 441), (147, 320), (2, 1)])
@pytest.mark.parametrize("n", [1, 700])
def test_resampling_restatement_equals_scipy(up, down, n):
    x = np.random.default_rng(up + n).standard_normal(n)
    got, ref = spec.resample_spec(x, up, down), scipy.signal.resample_poly(x, up, down)
    err, bound = np.abs(got - ref).max(), spec.resample_bound(x, up, down)
    print("{}/{} n {}: {} outputs, max abs {:.3g}, bound {:.3g}".format(up, down, n, len(got), err, bound))
    assert len(got) == len(ref) == -(-n * up // down)
    assert err <= bound


def test_resampling_filter_is_reduced_by_the_gcd():
    assert spec.resample_filter(16000, 48000)[:2] == (1, 3)
    assert spec.resample_filter(16000, 44100)[:2] == (160, 441)
    from idiaptts_amd.src.data_preparation.audio import down_sampling
    assert down_sampling.resample_ratio(44100, 16000) == (160, 441)
    assert np.array_equal(down_sampling.resample_filter(160, 441), spec.resample_filter(160, 441)[2])
    with pytest.raises(ValueError, match="16001"):
        down_sampling.resample_ratio(16001, 16000)


def test_frame_rms_restatement_pads_as_numpy_does():
    x = np.arange(1.0, 7.0)
    r = spec.frame_rms_spec(x, 4, 2)                # padded: 0 0 1 2 3 4 5 6 0 0
    assert np.allclose(r ** 2 * 4, [1 + 4, 1 + 4 + 9 + 16, 9 + 16 + 25 + 36, 25 + 36])
    r = spec.frame_rms_spec(x, 4, 2, "reflect")     # padded: 3 2 1 2 3 4 5 6 5 4
    assert np.allclose(r ** 2 * 4, [9 + 4 + 1 + 4, 1 + 4 + 9 + 16, 9 + 16 + 25 + 36, 25 + 36 + 25 + 16])


# ------------------------------------------------------------------------------------------------ trim arithmetic
def _remover(min_silence_ms=200):
    from idiaptts_amd.src.data_preparation.audio.silence_remove import SilenceRemover
    return SilenceRemover(min_silence_ms)


def _track(n_frames, first, last, loud=0.1, quiet=1e-5):
    rms = np.full(n_frames, quiet)
    rms[first:last + 1] = loud
    return rms


@pytest.mark.parametrize("lead_frames,tail_frames,warns", [
    (2, 2, (True, True)),          # 64 ms of silence on both sides: shorter than min_silence_ms, kept whole
    (10, 2, (False, True)),        # 320 ms in front: cut down to 200 ms
    (2, 10, (True, False)),
    (10, 12, (False, False)),
])
def test_trim_arithmetic_on_hand_made_tracks(lead_frames, tail_frames, warns, caplog):
    from idiaptts_amd.src.data_preparation.audio.silence_remove import trim_indices
    fs, hop = 16000, 512            # 32 ms
    n_frames = 60
    n = (n_frames - 1) * hop + 100
    rms = _track(n_frames, lead_frames, n_frames - 1 - tail_frames)
    indices = trim_indices(rms, n, hop, 50)
    assert indices == spec.trim_indices_spec(rms, n, hop, 50)
    assert indices == (lead_frames * hop, (n_frames - tail_frames) * hop)
    with caplog.at_level(logging.WARNING):
        got = _remover().keep_slice("a.wav", n, fs, indices)
    start, end, warn_start, warn_end = spec.keep_slice_spec(n, fs, indices, 200)
    assert got == (start, end) and (warn_start, warn_end) == warns
    assert ("in the beginning" in caplog.text) == warn_start and ("in the end" in caplog.text) == warn_end
    # by hand: 200 ms = 3200 samples stay in front of the first loud frame and behind the last
    assert start == (0 if warn_start else lead_frames * hop - 3200)
    trailing = n - (n_frames - tail_frames) * hop
    assert end == (-1 if warn_end else -(trailing - 3200) - 1)
    kept = np.arange(n)[start:end]
    assert kept[-1] == (n - 2 if warn_end else (n_frames - tail_frames) * hop + 3200 - 2)   # the last sample goes


def test_trim_of_an_all_silent_file_and_the_dropped_last_sample(caplog):
    from idiaptts_amd.src.data_preparation.audio.silence_remove import trim_indices
    fs, hop, n = 16000, 512, 16000
    rms = np.zeros(1 + n // hop)
    # every frame equals the loudest one: 0 dB > -50 dB, nothing is silent (librosa's answer for digital silence)
    assert trim_indices(rms, n, hop, 50) == spec.trim_indices_spec(rms, n, hop, 50) == (0, n)
    # no frame above the threshold: (0, 0), and the reference's bookkeeping keeps the first 200 ms less one sample
    assert trim_indices(np.array([np.nan, np.nan]), n, hop, 50) == (0, 0)
    with caplog.at_level(logging.WARNING):
        start, end = _remover().keep_slice("a.wav", n, fs, (0, 0))
    assert (start, end) == spec.keep_slice_spec(n, fs, (0, 0), 200)[:2] == (0, -(n - 3200) - 1)
    assert len(np.arange(n)[start:end]) == 3199
    # a file without any silence: everything but the last sample
    assert _remover().keep_slice("a.wav", n, fs, (0, n)) == (0, -1)
    # the threshold is relative to the loudest frame and its sign does not matter
    rms = np.array([1e-4, 1.0, 1.0, 10 ** -2.4, 10 ** -2.6])
    assert trim_indices(rms, 5 * hop, hop, 50) == (hop, 4 * hop)
    assert trim_indices(rms, 5 * hop, hop, abs(-90)) == (0, 5 * hop)


def test_hop_arithmetic_of_the_reference(monkeypatch):
    """frame_length = fs_to_frame_length(fs), hop_size_ms = min(min_silence_ms, 32) when None, process_list passes its
    chunk_size_ms in that position, hop_length = int(fs / 1000 * hop_size_ms)."""
    from idiaptts_amd.src.data_preparation.audio import silence_remove
    seen = []

    def fake_rms(x, offsets, frame_length, hop, pad_mode):
        seen.append((frame_length, hop, pad_mode))
        raise RuntimeError("stop")

    monkeypatch.setattr(silence_remove.ops, "frame_rms", fake_rms)
    monkeypatch.setattr(silence_remove.audio_batch, "to_device", lambda x: x)
    x, off = np.zeros(100), np.array([0, 100])
    for remover, fs, kwargs in [(_remover(), 22050, {}), (_remover(20), 48000, {}),
                                (_remover(), 44100, dict(hop_size_ms=10))]:
        with pytest.raises(RuntimeError, match="stop"):
            remover.trim_slices(x, off, fs, ["a"], **kwargs)
    assert seen == [(1024, 705, "constant"), (2048, 960, "constant"), (2048, 441, "constant")]
    sig = inspect.signature(silence_remove.SilenceRemover.process_list)
    assert sig.parameters["chunk_size_ms"].default == 10


# ------------------------------------------------------------------------------------------------ signatures
def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


E = inspect.Parameter.empty


def test_class_signatures_equal_the_reference():
    from idiaptts_amd.src.data_preparation.audio.high_pass_filter import HighPassFilter
    from idiaptts_amd.src.data_preparation.audio.normalize_loudness import LoudnessNormalizer
    from idiaptts_amd.src.data_preparation.audio.silence_remove import SilenceRemover
    from idiaptts_amd.src.data_preparation.audio import down_sampling
    lst = [("self", E), ("id_list", E), ("dir_audio", E), ("dir_out", E), ("format", "wav")]
    one = [("self", E), ("file", E), ("dir_audio", E), ("dir_out", E)]
    assert _params(HighPassFilter.__init__) == [("self", E), ("stop_freq_Hz", 70), ("pass_freq_Hz", 100),
                                                ("filter_order", 1001)]
    assert _params(HighPassFilter.process_list) == lst and _params(HighPassFilter.process_file) == one
    assert _params(HighPassFilter.highpass_filter) == [("self", E), ("raw", E), ("fs", E)]
    assert _params(LoudnessNormalizer.__init__) == [("self", E), ("ref_rms", 0.1)]
    assert _params(LoudnessNormalizer.process_list) == lst and _params(LoudnessNormalizer.process_file) == one
    assert _params(SilenceRemover.__init__) == [("self", E), ("min_silence_ms", 200)]
    assert _params(SilenceRemover.process_list) == lst + [("silence_threshold_db", -50), ("chunk_size_ms", 10)]
    assert _params(SilenceRemover.process_file) == one + [("silence_threshold_db", -50), ("hop_size_ms", None)]
    assert not hasattr(SilenceRemover, "_detect_leading_silence")
    assert _params(down_sampling.downsample_list) == [("id_list", E), ("dir_audio", E), ("dir_out", E),
                                                      ("target_sampling_rate", E)]


CLI_COMMON = {"-w/--dir_wav": ("dir_wav", str, True, None), "-o/--dir_out": ("dir_out", str, True, None),
              "-f/--file_id_list": ("file_id_list", str, True, None), "--format": ("format", str, False, "wav")}


@pytest.mark.parametrize("module,extra", [
    ("high_pass_filter", {"--stop_freq_Hz": ("stop_freq_Hz", float, False, 70),
                          "--pass_freq_Hz": ("pass_freq_Hz", float, False, 100),
                          "--filter_order": ("filter_order", int, False, 1001)}),
    ("normalize_loudness", {"--ref_rms": ("ref_rms", float, False, 0.1)}),
    ("silence_remove", {"--silence_db": ("silence_threshold_db", int, False, -50),
                        "--chunk_size": ("chunk_size_ms", int, False, 10),
                        "--min_silence_ms": ("min_silence_ms", int, False, 200)}),
])
def test_command_lines_equal_the_reference(module, extra, monkeypatch):
    import argparse
    import importlib
    mod = importlib.import_module("idiaptts_amd.src.data_preparation.audio." + module)
    captured = {}

    def parse_args(self, *args, **kwargs):
        captured["parser"] = self
        raise SystemExit(0)

    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse_args)
    with pytest.raises(SystemExit):
        mod.main()
    got = {"/".join(a.option_strings): (a.dest, a.type, a.required, a.default)
           for a in captured["parser"]._actions if a.dest != "help"}
    assert got == dict(CLI_COMMON, **extra)


def test_importing_down_sampling_has_no_effect(tmp_path):
    """The reference's module reads sys.argv and converts files at import."""
    code = ("import sys, os; sys.argv = ['x', {0!r}, {1!r}, {2!r}, '16000']; before = set(os.listdir({0!r}));"
            "import idiaptts_amd.src.data_preparation.audio.down_sampling as d;"
            "assert set(os.listdir({0!r})) == before and not os.path.exists({1!r});"
            "assert callable(d.main) and callable(d.downsample_list); print('quiet')"
            ).format(str(tmp_path), str(tmp_path / "out"), str(tmp_path / "missing_id_list"))
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert res.stdout.strip() == "quiet"


# ------------------------------------------------------------------------------------------------ C boundary
def test_header_binding_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "idiaptts_amd.h")).read()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in SYMBOLS:
        proto = re.search(r"\bint(?:64_t)? " + name + r"\s*\(([^)]*)\)", text)
        assert proto, name + " is not declared in the header"
        assert hasattr(cdll, name), "missing export " + name
        assert len(lib._SIGNATURES[name][1]) == len(proto.group(1).split(",")), name + ": arity differs"
    for cite in ("high_pass_filter.py:57", "down_sampling.py:43", "normalize_loudness.py:41-42",
                 "silence_remove.py:75-79"):
        assert cite in text


def _filtfilt(L, off=(0, 4000), numtaps=11, x=P, taps=P, y=P, ws=P, n=None):
    return L.itts_fir_filtfilt_batch(x, _off(*off) if off is not None else None, len(off) - 1 if n is None else n,
                                     taps, numtaps, y, ws, None)


def _resample(L, off=(0, 100), out=(0, 34), up=1, down=3, numtaps=61, x=P, taps=P, y=P, n=None):
    return L.itts_resample_poly_batch(x, _off(*off) if off is not None else None,
                                      _off(*out) if out is not None else None, len(off) - 1 if n is None else n,
                                      up, down, taps, numtaps, y, None)


def _loud(L, off=(0, 100), ref=0.1, x=P, y=P, n=None):
    return L.itts_loudness_normalise_batch(x, _off(*off) if off is not None else None,
                                           len(off) - 1 if n is None else n, ref, y, None)


def _rms(L, off=(0, 1000), f_off=(0, 7), frame=1024, hop=160, pad=0, x=P, out=P, n=None):
    return L.itts_frame_rms_batch(x, _off(*off) if off is not None else None,
                                  _off(*f_off) if f_off is not None else None, len(off) - 1 if n is None else n,
                                  frame, hop, pad, out, None)


@pytest.mark.parametrize("call,kwargs,needle", [
    (_filtfilt, dict(numtaps=10), "numtaps = 10"),
    (_filtfilt, dict(numtaps=0), "numtaps = 0"),
    (_filtfilt, dict(numtaps=-5), "numtaps = -5"),
    (_filtfilt, dict(numtaps=2049), "numtaps = 2049"),
    (_filtfilt, dict(off=(0, 33)), "33 samples"),
    (_filtfilt, dict(off=(0, 4000, 4033)), "signal 1 has 33 samples"),
    (_filtfilt, dict(off=(0, 33)), "greater than padlen, which is 33"),
    (_filtfilt, dict(x=None), "null pointer"),
    (_filtfilt, dict(taps=None), "null pointer"),
    (_filtfilt, dict(y=None), "null pointer"),
    (_filtfilt, dict(ws=None), "null pointer"),
    (_filtfilt, dict(off=None, n=1), "null pointer"),
    (_filtfilt, dict(n=-1), "n_signals = -1"),
    (_resample, dict(up=0), "up = 0"),
    (_resample, dict(down=0), "down = 0"),
    (_resample, dict(up=1025), "up = 1025"),
    (_resample, dict(down=1025), "down = 1025"),
    (_resample, dict(numtaps=60), "numtaps = 60"),
    (_resample, dict(out=(0, 33)), "33 output samples"),
    (_resample, dict(x=None), "null pointer"),
    (_resample, dict(y=None), "null pointer"),
    (_resample, dict(taps=None), "null pointer"),
    (_resample, dict(out=None, n=1), "null pointer"),
    (_loud, dict(ref=0.0), "ref_rms = 0.0"),
    (_loud, dict(x=None), "null pointer"),
    (_loud, dict(y=None), "null pointer"),
    (_loud, dict(off=(5, 100)), "offsets must start at 0"),
    (_rms, dict(hop=0), "hop = 0"),
    (_rms, dict(hop=-3), "hop = -3"),
    (_rms, dict(pad=2), "pad_mode = 2"),
    (_rms, dict(pad=-1), "pad_mode = -1"),
    (_rms, dict(frame=0), "frame_length = 0"),
    (_rms, dict(f_off=(0, 6)), "6 frames"),
    (_rms, dict(x=None), "null pointer"),
    (_rms, dict(out=None), "null pointer"),
    (_rms, dict(off=(0, 0), f_off=(0, 1)), "signal 0 is empty"),
    (_rms, dict(off=(0, 1 << 25), f_off=(0, (1 << 25) + 1), frame=2, hop=1), "33554433 frames"),
    (_resample, dict(off=(0, 1 << 36), out=(0, 1 << 26), up=1, down=1024, numtaps=20481), "16777216 workgroups"),
])
def test_refusals_name_the_value(call, kwargs, needle):
    L = lib.load()
    assert call(L, **kwargs) == -1
    msg = L.itts_last_error().decode()
    assert msg.startswith("itts_"), msg
    assert needle in msg, msg


def test_empty_batches_succeed_and_limits_are_inclusive():
    L = lib.load()
    assert _filtfilt(L, off=(0,), x=None, taps=None, y=None, ws=None) == 0
    assert _resample(L, off=(0,), out=(0,), x=None, taps=None, y=None) == 0
    assert _loud(L, off=(0,), x=None, y=None) == 0
    assert _rms(L, off=(0,), f_off=(0,), x=None, out=None) == 0
    # the arguments of an empty batch are still checked
    assert _filtfilt(L, off=(0,), numtaps=12) == -1
    assert _resample(L, off=(0,), out=(0,), down=1025) == -1
    assert _resample(L, off=(0,), out=(0,), up=1024, down=1024, numtaps=20481) == 0
    assert _filtfilt(L, off=(0,), numtaps=2047) == 0
    assert L.itts_fir_filtfilt_workspace_bytes(1000, 2, 11) == (1000 + 2 * 33) * 8
    assert L.itts_fir_filtfilt_workspace_bytes(0, 0, 11) == 0


# ------------------------------------------------------------------------------------------------ Python surface
def _write(path, data, fs=16000):
    wavfile.write(str(path), fs, data)
    return os.path.basename(str(path))


def test_multi_channel_input_raises_naming_the_file(tmp_path):
    from idiaptts_amd.src.data_preparation.audio.high_pass_filter import HighPassFilter
    from idiaptts_amd.src.data_preparation.audio.normalize_loudness import LoudnessNormalizer
    from idiaptts_amd.src.data_preparation.audio.silence_remove import SilenceRemover
    rng = np.random.default_rng(0)
    _write(tmp_path / "mono.wav", (rng.normal(size=5000) * 3000).astype(np.int16))
    _write(tmp_path / "stereo.wav", (rng.normal(size=(5000, 2)) * 3000).astype(np.int16))
    out = tmp_path / "out"
    for step in (HighPassFilter(filter_order=11), LoudnessNormalizer(), SilenceRemover()):
        with pytest.raises(ValueError, match=r"stereo\.wav.*2 channels"):
            step.process_file("stereo.wav", str(tmp_path), str(out))
        with pytest.raises(ValueError, match=r"stereo\.wav"):
            step.process_list(["mono", "stereo"], str(tmp_path), str(out))
    assert not out.exists()        # refused before anything was written


def test_too_short_a_file_raises_scipys_text_with_the_name(tmp_path):
    from idiaptts_amd.src.data_preparation.audio.high_pass_filter import HighPassFilter
    _write(tmp_path / "short.wav", np.zeros(3003, dtype=np.int16))
    with pytest.raises(ValueError) as theirs:
        scipy.signal.filtfilt(np.ones(1001), [1], np.zeros(3003))
    with pytest.raises(ValueError) as ours:
        HighPassFilter().process_file("short.wav", str(tmp_path), str(tmp_path / "out"))
    assert str(theirs.value) in str(ours.value) and "short.wav" in str(ours.value)
    assert not (tmp_path / "out").exists()
    with pytest.raises(ValueError) as ours:
        HighPassFilter(filter_order=11).highpass_filter(np.zeros(33), 16000)
    assert str(ours.value) == "The length of the input vector x must be greater than padlen, which is 33."


def test_an_all_zero_file_is_refused_by_the_loudness_normaliser(tmp_path):
    from idiaptts_amd.src.data_preparation.audio.normalize_loudness import LoudnessNormalizer
    _write(tmp_path / "zeros.wav", np.zeros(4000, dtype=np.int16))
    with pytest.raises(ValueError, match=r"zeros\.wav"):
        LoudnessNormalizer().process_file("zeros.wav", str(tmp_path), str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()


def test_an_all_zero_file_in_a_later_batch_is_refused_before_the_first_write(tmp_path):
    """Two sampling rates make two batches; the silent file sits in the second."""
    from idiaptts_amd.src.data_preparation.audio import audio_batch
    from idiaptts_amd.src.data_preparation.audio.normalize_loudness import LoudnessNormalizer
    rng = np.random.default_rng(1)
    _write(tmp_path / "loud.wav", (rng.normal(size=4000) * 3000).astype(np.int16), 16000)
    _write(tmp_path / "zeros.wav", np.zeros(4000, dtype=np.int16), 48000)
    assert len(audio_batch.plan_batches(["loud.wav", "zeros.wav"], str(tmp_path))) == 2
    with pytest.raises(ValueError, match=r"zeros\.wav"):
        LoudnessNormalizer().process_list(["loud", "zeros"], str(tmp_path), str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()


def test_the_shared_writer_is_the_synthesisers_conversion(tmp_path):
    from idiaptts_amd.src.data_preparation.audio import audio_batch
    y = np.array([0.0, 0.5, -1.0, 1.0, 1.5, -2.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, 1e-9])
    want = np.array([0, 16384, -32768, 32767, 32767, -32768, 0, 2, 2, 0], dtype=np.int16)
    assert np.array_equal(audio_batch.float_to_pcm16(y), want)
    assert np.array_equal(spec.pcm16_spec(y), want)
    with pytest.raises(FileNotFoundError):          # the writer creates no directory
        audio_batch.write_pcm16(str(tmp_path / "sub" / "a.wav"), y, 22050)
    audio_batch.write_pcm16(str(tmp_path / "a.wav"), y, 22050)
    fs, data = wavfile.read(str(tmp_path / "a.wav"))
    assert fs == 22050 and data.dtype == np.int16 and np.array_equal(data, want)
    assert audio_batch.wav_header(str(tmp_path / "a.wav")) == (22050, 1, 10)
    assert audio_batch.wav_layout(str(tmp_path / "a.wav")) == (22050, 1, 10)


def test_layout_of_files_the_native_reader_does_not_take(tmp_path):
    from idiaptts_amd.src.data_preparation.audio import audio_batch
    _write(tmp_path / "stereo.wav", np.zeros((7, 2), dtype=np.int16), 44100)
    assert audio_batch.wav_layout(str(tmp_path / "stereo.wav")) == (44100, 2, 7)
    # a data chunk that claims more than the file holds counts what is there
    raw = bytearray((tmp_path / "stereo.wav").read_bytes())
    at = raw.index(b"data") + 4
    raw[at:at + 4] = (4000).to_bytes(4, "little")
    (tmp_path / "lying.wav").write_bytes(bytes(raw))
    assert audio_batch.wav_header(str(tmp_path / "lying.wav")) == (44100, 2, 7)
    (tmp_path / "junk.wav").write_bytes(b"not a wav file at all")
    with pytest.raises(ValueError, match=r"junk\.wav"):
        audio_batch.wav_header(str(tmp_path / "junk.wav"))


def test_an_empty_file_is_refused_by_name(tmp_path):
    from idiaptts_amd.src.data_preparation.audio.normalize_loudness import LoudnessNormalizer
    from idiaptts_amd.src.data_preparation.audio.silence_remove import SilenceRemover
    _write(tmp_path / "empty.wav", np.zeros(0, dtype=np.int16))
    for step in (LoudnessNormalizer(), SilenceRemover()):
        with pytest.raises(ValueError, match=r"empty\.wav holds no samples"):
            step.process_file("empty.wav", str(tmp_path), str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()


def test_batches_are_planned_by_rate_and_size(tmp_path):
    from idiaptts_amd.src.data_preparation.audio import audio_batch
    for name, fs, n in [("a", 16000, 100), ("b", 16000, 200), ("c", 48000, 50), ("d", 16000, 300), ("e", 16000, 300)]:
        _write(tmp_path / (name + ".wav"), np.zeros(n, dtype=np.int16), fs)
    files = [n + ".wav" for n in "abcde"]
    assert audio_batch.plan_batches(files, str(tmp_path)) == [(["a.wav", "b.wav"], 16000), (["c.wav"], 48000),
                                                              (["d.wav", "e.wav"], 16000)]
    assert audio_batch.plan_batches(files, str(tmp_path), max_samples=500) == [
        (["a.wav", "b.wav"], 16000), (["c.wav"], 48000), (["d.wav"], 16000), (["e.wav"], 16000)]
