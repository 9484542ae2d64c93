"""Every family of entry points that takes scratch hands all of it back: a second call with the same arguments
finds every block of the first one free.

Each family is called once at a small size, the pool's figures are read (itts_scratch_pool_stats), and it is
called again: the bytes in use must be what they were, and the pool must not have grown.  A block that an entry point
loses -- taken through a ScratchScope that outlives the call, or through none -- stays busy: the second call cannot
reuse it, takes a fresh one, and both figures go up.

The audio is two utterances of 0.25 s and 0.4 s at 16 kHz; the layer ops run at the smallest shapes of their own
tests.  All inputs are made once (`Inputs`) and only read."""
import ctypes

import numpy as np
import pytest
import torch

import wavenet_spec as ws

pytestmark = pytest.mark.gpu
FS = 16000


def _synthetic(fs, seconds, seed):
    rng = np.random.default_rng(4321 + seed)
    n = int(fs * seconds)
    f0 = np.clip(140 + 30 * seed + np.cumsum(rng.normal(0, 0.02, n)) * 20, 80, 400)
    voiced = (np.sin(2 * np.pi * np.arange(n) / fs * 1.7 + seed) > -0.2).astype(float)
    phase = 2 * np.pi * np.cumsum(f0) / fs
    src = sum(np.sin(k * phase) / k for k in range(1, 10)) * voiced
    return 0.3 * src / np.abs(src).max() + 10 ** (-45 / 20) * rng.normal(size=n)


def _pool():
    from idiaptts_amd import lib as _lib
    L = _lib.load()
    r, u, k = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _lib.check(L.itts_scratch_pool_stats(ctypes.byref(r), ctypes.byref(u), ctypes.byref(k)), "stats")
    return r.value, u.value


class Inputs(object):
    """what the families read: the audio, one analysis of it, and the small layer operands"""
    _made = None

    @classmethod
    def get(cls, gpu):
        if cls._made is None:
            cls._made = cls(gpu)
        return cls._made

    def __init__(self, gpu):
        from idiaptts_amd import lib as _lib, ops
        L = _lib.load()
        gen = torch.Generator().manual_seed(77)
        xs = [_synthetic(FS, 0.25, 0), _synthetic(FS, 0.4, 1)]
        self.gpu = gpu
        self.x = torch.from_numpy(np.concatenate(xs)).to(gpu)
        self.x_off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).tolist()
        frames = [int(L.itts_world_num_frames(len(x), FS, 5.0)) for x in xs]
        self.f_off = np.concatenate([[0], np.cumsum(frames)]).tolist()
        self.hf_off = np.concatenate([[0], np.cumsum([ops.harvest_num_frames(len(x), FS) for x in xs])]).tolist()
        self.f0, self.sp, self.ap = ops.wav2world(self.x, self.x_off, self.f_off, FS)
        self.amp = self.sp.sqrt()
        self.mc = ops.mcep(self.amp, 24, 0.42, dtype=torch.float64)
        self.mc79 = 0.01 * torch.randn((self.amp.shape[0], 80), generator=gen, dtype=torch.float64).to(gpu)
        self.mgc = ops.mgcep(self.amp, 24, 0.42, -1.0 / 3.0, dtype=torch.float64)
        T = self.f_off[-1]
        self.lf0, self.vuv = ops.lf0_vuv(self.f0, self.f_off)
        self.sp32 = torch.randn((T, 5), generator=gen).to(gpu)
        self.bap32 = torch.randn((T, 1), generator=gen).to(gpu)
        # STFT / Griffin-Lim: 1024-point frames every 80 samples, centred
        self.window = torch.hann_window(1024, periodic=True, dtype=torch.float64).to(gpu)
        self.s_off = np.concatenate([[0], np.cumsum([1 + len(x) // 80 for x in xs])]).tolist()
        self.S = ops.stft_amp(self.x, self.x_off, self.s_off, [0, 0], 1024, 80, "reflect", self.window)
        self.angles = torch.polar(torch.ones_like(self.S),
                                  (6.28 * torch.rand(self.S.shape, generator=gen)).to(gpu)).contiguous()
        # audio preparation
        taps = np.hanning(33)[1:-1]
        self.taps = torch.from_numpy(taps / taps.sum()).to(gpu)
        # raw-waveform targets
        self.mol_x = torch.randn((2, 6, 9), generator=gen).to(gpu)
        self.mol_y = (2 * torch.rand((2, 1, 9), generator=gen) - 1).to(gpu)
        self.mol_w = torch.ones((2, 9)).to(gpu)
        self.rows = torch.randn((12, 3), generator=gen).to(gpu)
        # Conv1d: three rows of 12 steps, 12 -> 10 channels, 5 taps, no padding (conv_cases "pad0")
        self.conv_x = torch.randn((12, 3, 12), generator=gen).to(gpu)
        self.conv_w = torch.randn((10, 12, 5), generator=gen).to(gpu)
        self.conv_b = torch.randn((10,), generator=gen).to(gpu)
        self.conv_dz = torch.randn((8, 3, 10), generator=gen).to(gpu)
        # WaveNet generation: the small k = 2 class model of tests/wavenet_spec.py, two rows
        from idiaptts_amd.src.neural_networks.pytorch.models.WaveNetWrapper import WaveNetWrapper
        net = ws.small(k=2, mol=False)
        sd = ws.random_state(net, seed=33, scale=1.5)
        self.wavenet = WaveNetWrapper.Config(
            layers=net.layers, stacks=net.stacks, residual_channels=net.R, gate_channels=net.G,
            skip_out_channels=net.S, kernel_size=net.k, cin_channels=net.cin, out_channels=net.C,
            scalar_input=net.scalar, dropout=0.0, weight_normalization=True).create_model()
        self.wavenet.load_state_dict({k: torch.from_numpy(np.asarray(v)).float() for k, v in sd.items()})
        self.wavenet = self.wavenet.to(gpu).eval()
        self.wn_c = torch.randn((2, net.cin, 7), generator=gen).to(gpu)
        self.wn_u = (0.001 + 0.998 * torch.rand((2, 7), generator=gen)).to(gpu)
        # one bidirectional H = 512 LSTM layer, rows of 3, 2 and 1 steps (rnn_cases: H = 512 is the persistent kernels')
        from idiaptts_amd import nn as inn
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(5)
            self.lstm = inn.LSTM(24, 512, 1, bidirectional=True).to(gpu)
        self.lstm_x = torch.randn((3, 3, 24), generator=gen).to(gpu)
        self.lstm_lens = torch.tensor([3, 2, 1], dtype=torch.int64)
        # MLPG: 3 dimensions, utterances of 194 frames (the shortest the stream form takes: MLPG_SEQ_BELOW) and 40
        self.mlpg_off = [0, 194, 234]
        self.mlpg_feat = torch.randn((234, 9), generator=gen, dtype=torch.float64).to(gpu)
        self.mlpg_var = (0.5 + torch.rand((9,), generator=gen, dtype=torch.float64)).to(gpu)
        self.mlpg_gout = torch.randn((234, 3), generator=gen, dtype=torch.float64).to(gpu)


def _lstm(i):
    x = i.lstm_x.clone().requires_grad_(True)
    out, _ = i.lstm(x, None, i.lstm_lens)
    out.sum().backward()


def _mlpg_stream(i):
    from idiaptts_amd import ops
    with ops.mlpg_forced(solve="stream"):
        ops.mlpg_generation(i.mlpg_feat, i.mlpg_var, 3, i.mlpg_off)
        assert ops.mlpg_last_form() & ops.MLPG_SOLVE_MASK == ops.MLPG_STREAM
    with ops.mlpg_adjoint_forced("stream"):
        ops.mlpg_adjoint(i.mlpg_gout, i.mlpg_var, 3, i.mlpg_off)
        assert ops.mlpg_adjoint_last_form() == ops.MLPG_STREAM


def _families():
    from idiaptts_amd import ops
    return {
        "dio": lambda i: ops.dio(i.x, i.x_off, i.f_off, FS),
        "stonemask": lambda i: ops.stonemask(i.x, i.x_off, i.f0, i.f_off, FS),
        "d4c": lambda i: ops.d4c(i.x, i.x_off, i.f0, i.f_off, FS),
        "cheaptrick_mcep": lambda i: ops.cheaptrick_mcep(i.x, i.x_off, i.f0, i.f_off, FS, order=24, alpha=0.42),
        "cheaptrick_mcep_no_sp": lambda i: ops.cheaptrick_mcep(i.x, i.x_off, i.f0, i.f_off, FS, want_sp=False,
                                                              order=24, alpha=0.42),
        "mcep": lambda i: ops.mcep(i.amp, 24, 0.42),
        "mcep_order_79": lambda i: ops.mcep(i.amp, 79, 0.42),
        "mgc2sp": lambda i: ops.mgc2sp(i.mc, 0.42, 1024),
        "mgc2sp_order_79": lambda i: ops.mgc2sp(i.mc79, 0.42, 1024),
        "mgcep": lambda i: ops.mgcep(i.amp, 24, 0.42, -1.0 / 3.0),
        "mgc2sp_gamma": lambda i: ops.mgc2sp_gamma(i.mgc, 0.42, -1.0 / 3.0, 1024),
        "harvest": lambda i: ops.harvest(i.x, i.x_off, i.hf_off, FS),
        "world_synthesize": lambda i: ops.world_synthesize(i.f0, i.sp, i.ap, i.f_off, FS),
        "wav2world": lambda i: ops.wav2world(i.x, i.x_off, i.f_off, FS),
        "lf0_vuv": lambda i: ops.lf0_vuv(i.f0, i.f_off),
        "interpolate_lin_f32": lambda i: ops.interpolate_lin_f32(i.lf0 * i.vuv, i.f_off),
        "assemble_cmp": lambda i: ops.assemble_cmp(i.sp32, i.lf0, i.vuv, i.bap32, i.f_off),
        "stft_amp": lambda i: ops.stft_amp(i.x, i.x_off, i.s_off, [0, 0], 1024, 80, "reflect", i.window),
        "griffinlim": lambda i: ops.griffinlim(i.S, i.angles.clone(), i.s_off, 1024, 80, "reflect", i.window, 2, 0.99),
        "fir_filtfilt": lambda i: ops.fir_filtfilt(i.x, i.x_off, i.taps),
        "resample_poly": lambda i: ops.resample_poly(i.x, i.x_off, 1, 2, i.taps),
        "loudness_normalise": lambda i: ops.loudness_normalise(i.x, i.x_off),
        "frame_rms": lambda i: ops.frame_rms(i.x, i.x_off, 1024, 160),
        "mol_loss": lambda i: ops.mol_loss(i.mol_x, i.mol_y, i.mol_w),
        "mulaw_encode": lambda i: ops.mulaw_encode(i.x, i.x_off),
        "mulaw_onehot": lambda i: ops.mulaw_onehot(i.x, [0, 4100], [64, 33]),
        "sample_linearly": lambda i: ops.sample_linearly(i.rows, [0, 7, 12], 2),
        "conv1d_fwd": lambda i: ops.conv1d_fwd(i.conv_x, i.conv_w, i.conv_b, 0, 1, False),
        "conv1d_bwd_input": lambda i: ops.conv1d_bwd_input(i.conv_dz, i.conv_w, 12, 0, 1, False),
        "wavenet_generate": lambda i: i.wavenet.model.generate(i.wn_c, [7, 4], uniforms=i.wn_u),
        "lstm_512_fwd_bwd": _lstm,
        "mlpg_stream": _mlpg_stream,
    }


FAMILIES = ["dio", "stonemask", "d4c", "cheaptrick_mcep", "cheaptrick_mcep_no_sp", "mcep", "mcep_order_79", "mgc2sp",
            "mgc2sp_order_79", "mgcep", "mgc2sp_gamma", "harvest", "world_synthesize", "wav2world", "lf0_vuv",
            "interpolate_lin_f32", "assemble_cmp", "stft_amp", "griffinlim", "fir_filtfilt", "resample_poly",
            "loudness_normalise", "frame_rms", "mol_loss", "mulaw_encode", "mulaw_onehot", "sample_linearly",
            "conv1d_fwd", "conv1d_bwd_input", "wavenet_generate", "lstm_512_fwd_bwd", "mlpg_stream"]


def test_the_family_list_is_the_table():
    assert sorted(FAMILIES) == sorted(_families())


@pytest.mark.parametrize("family", FAMILIES)
def test_a_second_call_finds_every_block_of_the_first_one_free(gpu, family):
    inputs = Inputs.get(gpu)
    call = _families()[family]
    call(inputs)
    torch.cuda.synchronize()
    reserved, used = _pool()
    call(inputs)
    torch.cuda.synchronize()
    reserved2, used2 = _pool()
    print("{}: reserved {} -> {}, used {} -> {}".format(family, reserved, reserved2, used, used2))
    assert used2 == used
    assert reserved2 <= reserved
