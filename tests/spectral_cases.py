"""The case tables and seeded inputs of tests/test_gpu_spectral_edges.py: the four spectral kernels (stft_wave_kernel
and mel_project_kernel of csrc/stft.hip, griffinlim_kernel, mel_inverse_kernel) at the lengths, hops, band counts and tile
counts where their code takes another path than at the working point of the fixture audio.

tests/test_spectral_cases.py proves on the CPU, from the host formulas restated here, that every case reaches the
branch it is named for (how often the centre padding reflects, how many Griffin-Lim tiles an utterance has and how
short the shortest is, how many mel filters have no bin, which of a lane's four filter slots the last band falls in,
whether the utterance lookup searches, whether mel_project's grid strides), and checks the three restatements
(stft_spec, griffinlim_spec, mel_inverse_spec) at the new cases against independent evaluations.

Every input is make_audio or numpy's default_rng with a fixed seed; nothing is read from a file."""
import functools

import numpy as np

import stft_spec

PAD_MODES = ("reflect", "constant")
KINDS = ("amp_sp", "amp_sp_f64", "log_amp_sp", "mfbanks")
FS_OF = {1024: 16000, 2048: 48000}          # the sampling rate whose mel basis a transform size is tested with

# ------------------------------------------------------------------------------------------------ signals
@functools.lru_cache(maxsize=None)
def _voice(seed):
    from idiaptts_amd.synthetic_audio import make_audio
    return make_audio(16000, 0.6, seed)


def signal(n, seed):
    """n samples: a stretch of synthetic voice plus white noise (no sample is exactly 0, whatever the stretch holds)"""
    rng = np.random.default_rng(seed)
    base = _voice(seed % 3)
    assert n <= len(base) - 1000
    return base[1000:1000 + n] + 0.05 * rng.standard_normal(n)


# ------------------------------------------------------------------------------------------------ STFT
STFT_POINTS = ((1024, 80), (2048, 240))      # (n_fft, hop) of the length cases
STFT_LENGTHS = {1024: (1, 2, 3, 79, 80, 81, 511, 512, 513, 1023, 1024, 1025),
                2048: (1, 1023, 1024, 1025, 2047, 2048, 2049)}
SHORT_LENGTHS = {1024: (2, 3, 79, 80, 81, 511, 512), 2048: (1023, 1024)}     # the padding reflects at least twice
WIN_LENGTHS = {1024: (400, 1), 2048: (1101, 2047)}
HOP_CASES = ((1, 40), (80, 3000), (1024, 4100), (1500, 4100))  # (hop, samples) at 1024
FIRST = (0, 3, 1, 0, 2)
MEL_BANDS = {(16000, 1024): (1, 2, 63, 64, 65, 128, 129, 513), (48000, 2048): (1, 64, 65, 513)}
MEL_PROJECT_ROWS = (1, 3, 4, 5, 16389)
MEL_PROJECT_WAVES, MEL_PROJECT_MAX_BLOCKS = 4, 4096            # rows per workgroup and the grid cap of itts_mel_project
BALLOT_MAX_UTTS = 1024                                         # find_utt_wave searches beyond this many utterances
N_MANY, N_PREFIX = 1030, 1024
MANY_ZERO_FRAME_UTTS = (0, 1, 515, 516, 1023, 1029)            # start, middle, the prefix's end, the end


def stft_modes(n_fft, n):
    """(center, pad_mode) pairs a length is run with: both paddings, and center=False where a frame fits"""
    return [(True, "reflect"), (True, "constant")] + ([(False, "reflect")] if n >= n_fft else [])


def reflections(n, n_fft):
    """How many times np.pad reflects an n-sample signal to pad n_fft // 2 on a side: each reflection adds at most
    n - 1 samples.  0 for one sample (np.pad repeats it: padded_sample's xl == 1 branch)."""
    return 0 if n == 1 else -(-(n_fft // 2) // (n - 1))


def reflect_index(j, n):
    """padded_sample's index arithmetic: position j of the reflected signal, period 2 (n - 1)"""
    if n == 1:
        return 0
    p = 2 * (n - 1)
    j %= p
    return p - j if j >= n else j


def mel_project_strides(T):
    return -(-T // MEL_PROJECT_WAVES) > MEL_PROJECT_MAX_BLOCKS


def direct_amp_sp(x, n_fft, hop, win_length=None, center=True, pad_mode="reflect"):
    """|rfft| / sqrt(K) frame by frame on np.pad's signal and scipy's window: no index tables, no restated window"""
    import scipy.signal
    win_length = n_fft if win_length is None else win_length
    w = np.zeros(n_fft)
    lpad = (n_fft - win_length) // 2
    w[lpad:lpad + win_length] = scipy.signal.get_window("hann", win_length, fftbins=True)
    y = np.pad(np.asarray(x, np.float64), n_fft // 2, mode=pad_mode) if center else np.asarray(x, np.float64)
    rows = [np.abs(np.fft.rfft(y[t * hop:t * hop + n_fft] * w)) for t in range(1 + (len(y) - n_fft) // hop)]
    return np.asarray(rows) / np.sqrt(n_fft // 2 + 1)


def stft_frames(n, n_fft, hop, center=True):
    return 1 + n // hop if center else 1 + (n - n_fft) // hop


def first_batch(n_fft, hop, center):
    """the ragged batch of the `first` cases: (signals, first, rows kept per utterance)"""
    lengths = [n_fft + 7 * hop + 3, 2 * n_fft + 1, n_fft + 2 * hop, n_fft + 3 * hop - 1, 3 * n_fft]
    raws = [signal(n, 20 + u) for u, n in enumerate(lengths)]
    keep = [stft_frames(n, n_fft, hop, center) - f - (u % 2) for u, (n, f) in enumerate(zip(lengths, FIRST))]
    assert min(keep) >= 1
    return raws, list(FIRST), keep


@functools.lru_cache(maxsize=None)
def many_utterances():
    """1 030 utterances of 90 to 400 samples at 1024 / hop 80: (samples back to back, lengths, rows per utterance);
    the utterances of MANY_ZERO_FRAME_UTTS keep no row"""
    from idiaptts_amd.synthetic_audio import make_audio
    rng = np.random.default_rng(1030)
    lengths = rng.integers(90, 401, N_MANY)
    total = int(lengths.sum())
    x = make_audio(16000, total / 16000.0 + 0.01, 3)[:total] + 0.01 * rng.standard_normal(total)
    rows = 1 + lengths // 80
    rows[list(MANY_ZERO_FRAME_UTTS)] = 0
    return x, [int(n) for n in lengths], [int(r) for r in rows]


@functools.lru_cache(maxsize=None)
def sweep_draws(seed=2024, count=24):
    """The random sweep: `count` argument sets from default_rng(seed).  A draw the entry point must refuse
    (center=False with an utterance shorter than n_fft) is drawn again, so all `count` run."""
    rng = np.random.default_rng(seed)
    draws = []
    while len(draws) < count:
        n_fft = int(rng.choice((1024, 2048)))
        d = dict(n_fft=n_fft, hop=int(rng.integers(1, n_fft * 3 // 2 + 1)), win_length=int(rng.integers(1, n_fft + 1)),
                 center=bool(rng.integers(2)), pad_mode=PAD_MODES[rng.integers(2)], kind=KINDS[rng.integers(4)],
                 n_mels=int(rng.integers(1, 514)), seed=int(rng.integers(1 << 30)))
        d["lengths"] = [int(n) for n in rng.integers(1, 3 * n_fft + 1, int(rng.integers(1, 7)))]
        if not d["center"] and min(d["lengths"]) < n_fft:
            continue
        frames = [stft_frames(n, n_fft, d["hop"], d["center"]) for n in d["lengths"]]
        d["first"] = [int(rng.integers(0, f)) for f in frames]
        d["rows"] = [int(rng.integers(1, f - a + 1)) for f, a in zip(frames, d["first"])]
        draws.append(d)
    return tuple(draws)


def sweep_signals(d):
    rng = np.random.default_rng(d["seed"])
    return [signal(n, int(rng.integers(1 << 20))) for n in d["lengths"]]


# ------------------------------------------------------------------------------------------------ Griffin-Lim
GL_CASES = ((1024, 256, None), (1024, 512, None), (1024, 64, None), (1024, 80, 400),
            (2048, 512, None), (2048, 1024, None), (2048, 240, None), (2048, 240, 1200))    # n_fft, hop, win_length
GL_BOTH_PADS = ((1024, 512), (2048, 1024))          # the two-frame tiles
GL_BOTH_DTYPES = ((1024, 256), (2048, 512))
GL_ITERS = 5
# griffinlim.hip's LDS plan: the budget, and per transform size (waves, twiddle table bytes, exchange bytes per wave)
GL_LDS_BUDGET = 160 * 1024
GL_LDS_PLAN = {1024: (12, 12288, 8704), 2048: (6, 24448, 16896)}


def gl_tile_frames(n_fft, hop):
    """tile_frames of griffinlim.hip restated: the largest tile whose segment of (F - 1) hop + n_fft doubles fits
    beside the table and the waves' exchange rows, a multiple of the wave count when it is at least that"""
    waves, table, rows = GL_LDS_PLAN[n_fft]
    samples = (GL_LDS_BUDGET - table - waves * rows) // 8
    if samples < n_fft:
        return 0
    F = (samples - n_fft) // hop + 1
    if F >= waves:
        F -= F % waves
    return 0 if F < 2 or F * hop <= n_fft else F


def gl_tiles(T, F):
    """the host's split of T frames into ceil(T / F) tiles of near-equal size: [(first frame, end frame)]"""
    nt = -(-T // F)
    return [(k * T // nt, (k + 1) * T // nt) for k in range(nt)]


def gl_frame_counts(n_fft, hop):
    F = gl_tile_frames(n_fft, hop)
    return (2, 3, F, F + 1, 2 * F + 1)


def gl_spectra(n_fft, counts, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return [(rng.random((t, n_fft // 2 + 1)) ** 3).astype(dtype) for t in counts]


# ------------------------------------------------------------------------------------------------ mel inversion
MI_BANDS = {(16000, 1024): (1, 2, 63, 64, 65, 128, 129, 192, 193, 256), (48000, 2048): (1, 65, 256)}
MI_NNLS_BANDS = (65, 129)
MI_FRAME_COUNTS = (1, 2, 3, 5)
MI_WAVES = 4                      # frames per workgroup of mel_inverse_kernel


def lane_slot(n_mels):
    """the slot s of filter l + 64 s that the last band occupies"""
    return (n_mels - 1) // 64


@functools.lru_cache(maxsize=None)
def mel_bands(fs, n_fft, n_mels):
    """mel filter banks of 2 s of synthetic voice, every 5th frame: float32 [81, n_mels], read-only"""
    from idiaptts_amd.synthetic_audio import make_audio
    B = np.ascontiguousarray(stft_spec.mfbanks(make_audio(fs, 2.0, 5), fs, n_fft, fs // 200, n_mels)[::5])
    B.setflags(write=False)
    return B
