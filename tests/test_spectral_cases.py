"""The case tables of tests/spectral_cases.py reach the branches they are named for -- worked out from the host
formulas alone, no GPU -- and the three restatements the GPU tests compare with (stft_spec, griffinlim_spec,
mel_inverse_spec) hold at the new cases against evaluations that share no code with them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import griffinlim_spec as gl  # noqa: E402
import mel_inverse_spec as mi  # noqa: E402
import spectral_cases as sc  # noqa: E402
import stft_spec  # noqa: E402


# ------------------------------------------------------------------------------------------------ reach
def test_short_lengths_reflect_at_least_twice_and_one_sample_repeats():
    for n_fft, _ in sc.STFT_POINTS:
        lengths = sc.STFT_LENGTHS[n_fft]
        assert 1 in lengths and sc.reflections(1, n_fft) == 0
        assert set(sc.SHORT_LENGTHS[n_fft]) == {n for n in lengths if sc.reflections(n, n_fft) >= 2}
        assert len(sc.SHORT_LENGTHS[n_fft]) >= 2
        # both sides of every threshold: one reflection, and signals at least one frame long for center=False
        assert any(sc.reflections(n, n_fft) == 1 and n < n_fft for n in lengths)
        assert {n_fft - 1, n_fft, n_fft + 1} <= set(lengths)
    assert max(sc.reflections(n, 1024) for n in sc.STFT_LENGTHS[1024]) == 512      # two samples: 512 reflections


def test_reflect_index_is_np_pad():
    """the period-2 (n - 1) index arithmetic of the kernels is np.pad's repeated reflection, one sample included"""
    for n_fft, _ in sc.STFT_POINTS:
        for n in sc.STFT_LENGTHS[n_fft]:
            x = np.arange(n, dtype=np.float64)
            ref = np.pad(x, n_fft // 2, mode="reflect")
            got = np.array([x[sc.reflect_index(j, n)] for j in range(-(n_fft // 2), n + n_fft // 2)])
            assert np.array_equal(got, ref), (n_fft, n)


def test_hops_window_lengths_and_first_batches():
    assert [h for h, _ in sc.HOP_CASES] == [1, 80, 1024, 1500] and sc.HOP_CASES[0][1] == 40
    assert max(h for h, _ in sc.HOP_CASES) > 1024                # frames that skip samples
    for n_fft in (1024, 2048):
        assert all(0 < w < n_fft for w in sc.WIN_LENGTHS[n_fft])
        assert any(w % 2 for w in sc.WIN_LENGTHS[n_fft])         # an odd length: uneven zero padding of the window
    for n_fft, hop, center in ((1024, 80, True), (2048, 240, True), (2048, 240, False)):
        raws, first, keep = sc.first_batch(n_fft, hop, center)
        assert tuple(first) == (0, 3, 1, 0, 2) and len(raws) == 5
        for r, f, k in zip(raws, first, keep):
            assert 1 <= k and f + k <= sc.stft_frames(len(r), n_fft, hop, center)
        assert len({len(r) for r in raws}) == 5                  # ragged


def test_many_utterances_search_and_the_prefix_ballots():
    x, lengths, rows = sc.many_utterances()
    assert len(lengths) == sc.N_MANY == 1030 > sc.BALLOT_MAX_UTTS >= sc.N_PREFIX == 1024
    assert len(x) == sum(lengths) and 90 <= min(lengths) and max(lengths) <= 400
    zero = [u for u, r in enumerate(rows) if r == 0]
    assert tuple(zero) == sc.MANY_ZERO_FRAME_UTTS
    assert zero[0] == 0 and zero[-1] == sc.N_MANY - 1 and sc.N_PREFIX - 1 in zero      # start, end, the prefix's end
    assert any(0 < u < sc.N_PREFIX - 1 and rows[u - 1] > 0 and rows[u + 2] > 0 and rows[u + 1] == 0 for u in zero)
    assert all(r == 1 + n // 80 for n, r in zip(lengths, rows) if r)
    assert all(sc.reflections(n, 1024) >= 2 for n in lengths)                         # every one shorter than n_fft / 2


def test_mel_band_counts_passes_and_empty_filters():
    from idiaptts_amd import world
    for (fs, n_fft), bands in sc.MEL_BANDS.items():
        passes = {-(-m // 64) for m in bands}                    # trips of `for (m = l; m < n_mels; m += 64)` in lane 0
        assert {1, 2} <= passes and max(passes) == 9
        assert {1, 64, 65, 513} <= set(bands)
        for m in bands:
            tab, w = world.mel_tables(fs, n_fft, m)
            tab = tab.reshape(-1, 3)
            empty = int((tab[:, 1] == 0).sum())
            assert (empty > 0) == (m == 513), (fs, n_fft, m, empty)
            assert len(w) == tab[:, 1].sum() and np.all(tab[:, 0] + tab[:, 1] <= n_fft // 2 + 1)
            # the spec's basis has the same empty rows, so the kernel's zeros are compared with zeros
            assert np.array_equal(tab[:, 1] == 0, ~stft_spec.mel_basis(fs, n_fft, m).any(axis=1))
    empty = lambda fs, n_fft: int((world.mel_tables(fs, n_fft, 513)[0].reshape(-1, 3)[:, 1] == 0).sum())  # noqa: E731
    assert (empty(16000, 1024), empty(22050, 1024), empty(48000, 2048)) == (48, 77, 48)


def test_mel_project_rows_stride_the_grid_once():
    assert sc.MEL_PROJECT_ROWS == (1, 3, 4, 5, 16389)
    assert [sc.mel_project_strides(t) for t in sc.MEL_PROJECT_ROWS] == [False, False, False, False, True]
    assert not sc.mel_project_strides(4 * 4096) and sc.mel_project_strides(4 * 4096 + 1)
    assert {t % 4 for t in sc.MEL_PROJECT_ROWS} == {0, 1, 3}


def test_sweep_draws_are_24_and_all_accepted():
    draws = sc.sweep_draws()
    assert len(draws) == 24 and draws is sc.sweep_draws()
    for d in draws:
        assert d["n_fft"] in (1024, 2048) and 1 <= d["hop"] <= d["n_fft"] * 3 // 2
        assert 1 <= d["win_length"] <= d["n_fft"] and 1 <= d["n_mels"] <= 513
        assert 1 <= len(d["lengths"]) <= 6 and 1 <= min(d["lengths"]) and max(d["lengths"]) <= 3 * d["n_fft"]
        assert d["center"] or min(d["lengths"]) >= d["n_fft"]
        for n, a, r in zip(d["lengths"], d["first"], d["rows"]):
            assert r >= 1 and a >= 0 and a + r <= sc.stft_frames(n, d["n_fft"], d["hop"], d["center"])
    assert {d["kind"] for d in draws} == set(sc.KINDS)
    assert {d["center"] for d in draws} == {True, False} and {d["pad_mode"] for d in draws} == set(sc.PAD_MODES)
    assert {d["n_fft"] for d in draws} == {1024, 2048}
    assert any(d["hop"] > d["n_fft"] for d in draws) and any(max(d["first"]) > 0 for d in draws)
    assert any(d["center"] and sc.reflections(min(d["lengths"]), d["n_fft"]) >= 2 for d in draws)


def test_griffinlim_tile_counts_and_the_two_frame_tiles():
    F = {(n_fft, hop): sc.gl_tile_frames(n_fft, hop) for n_fft, hop, _ in sc.GL_CASES}
    assert F == {(1024, 256): 12, (1024, 512): 10, (1024, 64): 72, (1024, 80): 60,
                 (2048, 512): 6, (2048, 1024): 3, (2048, 240): 12}
    smallest = {}
    for (n_fft, hop), f in F.items():
        counts = sc.gl_frame_counts(n_fft, hop)
        assert counts == (2, 3, f, f + 1, 2 * f + 1)
        tiles = [sc.gl_tiles(t, f) for t in counts]
        assert [len(t) for t in tiles] == [1, 1, 1, 2, 3]
        for t, tl in zip(counts, tiles):
            assert tl[0][0] == 0 and tl[-1][1] == t and all(a[1] == b[0] for a, b in zip(tl[:-1], tl[1:]))
            assert all(2 <= b - a <= f for a, b in tl)
        smallest[(n_fft, hop)] = min(b - a for tl in tiles[3:] for a, b in tl)
        # the halo: frames of the neighbouring tiles that overlap a tile's segment
        halo = -(-n_fft // hop) - 1
        assert halo == {64: 15, 80: 12, 240: 8, 256: 3, 512: {1024: 1, 2048: 3}[n_fft], 1024: 1}[hop]
    assert smallest[(2048, 1024)] == 2                           # every tile of the seven-frame utterance but the last
    assert smallest[(1024, 512)] == 5
    assert set(sc.GL_BOTH_PADS) == {(1024, 512), (2048, 1024)} == {k for k in F if k[1] == k[0] // 2}
    assert all(k in F for k in sc.GL_BOTH_DTYPES)
    # default hops (win_length // 4) and zero-padded windows are in the table
    assert {(1024, 256, None), (2048, 512, None)} <= set(sc.GL_CASES)
    assert {w for _, _, w in sc.GL_CASES if w} == {400, 1200}


def test_zero_padded_window_leaves_positions_without_window_sum():
    """win_length < n_fft: untrimmed positions that no frame's window covers (the `wss > FLT_MIN` branch not taken)"""
    for n_fft, hop, win_length in sc.GL_CASES:
        if win_length:
            w = stft_spec.window(n_fft, win_length)
            wss = gl.window_sumsquare(w, 3, hop, n_fft)
            assert (wss <= np.finfo(np.float32).tiny).sum() >= n_fft - win_length
            assert (wss > np.finfo(np.float32).tiny).any()


def test_mel_inverse_band_counts_fill_every_lane_slot_edge():
    from idiaptts_amd import world
    slots = {m: sc.lane_slot(m) for m in sc.MI_BANDS[(16000, 1024)]}
    assert slots == {1: 0, 2: 0, 63: 0, 64: 0, 65: 1, 128: 1, 129: 2, 192: 2, 193: 3, 256: 3}
    assert {sc.lane_slot(m) for m in sc.MI_BANDS[(48000, 2048)]} == {0, 1, 3}
    assert max(sc.MI_BANDS[(16000, 1024)]) == world.MEL_INVERSE_MAX_MELS
    assert all(0 <= s <= 3 for s in slots.values())
    # frame counts that leave 3, 2, 1 and (with 5) 3 waves of the last workgroup idle
    assert sc.MI_FRAME_COUNTS == (1, 2, 3, 5) and all(f % sc.MI_WAVES for f in sc.MI_FRAME_COUNTS)
    for key, bands in sc.MI_BANDS.items():
        for m in bands:
            B = sc.mel_bands(*key, m)
            assert B.shape == (81, m) and B.dtype == np.float32 and np.isfinite(B).all() and B.max() > 0


def test_pinv_table_is_zero_where_no_filter_reaches():
    """a bin in no filter (0 Hz, the Nyquist bin) has a zero column in A, so its row of pinv(A) is zero: the table
    must hold exact zeros there, or the start leaves rounding noise of the SVD in bins no iteration ever moves"""
    from idiaptts_amd import world
    for fs, n_fft, m in ((16000, 1024, 80), (16000, 1024, 256), (48000, 2048, 65)):
        for dtype in (np.float32, np.float64):
            A = world.mel_basis_plain(fs, n_fft, m, dtype)
            dead = np.flatnonzero(~A.any(axis=0))
            assert len(dead) >= 1 and dead[0] == 0
            pinv_t = world.mel_inverse_tables(fs, n_fft, m, dtype)[3]
            assert not pinv_t[:, dead].any(), np.abs(pinv_t[:, dead]).max()


# ------------------------------------------------------------------------------------------------ restatements
def _rel(got, ref):
    assert got.shape == ref.shape
    return np.abs(got - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("pad_mode", sc.PAD_MODES)
def test_amp_sp_restatement_at_short_lengths(pad_mode):
    for n_fft, hop in sc.STFT_POINTS:
        for n in (1,) + sc.SHORT_LENGTHS[n_fft]:
            x = sc.signal(n, n)
            got = stft_spec.amp_sp(x, n_fft, hop, pad_mode=pad_mode)
            assert got.shape == (1 + n // hop, n_fft // 2 + 1)
            assert _rel(got, sc.direct_amp_sp(x, n_fft, hop, pad_mode=pad_mode)) <= 1e-13, (n_fft, n)
    # one sample, reflected: the signal is constant, every frame is the window's spectrum times the sample
    x = sc.signal(1, 1)
    w = np.abs(np.fft.rfft(stft_spec.window(1024))) / np.sqrt(513)
    assert _rel(stft_spec.amp_sp(x, 1024, 80)[0], abs(x[0]) * w) <= 1e-13


def test_amp_sp_restatement_at_the_window_lengths():
    for n_fft, hop in sc.STFT_POINTS:
        x = sc.signal(3 * n_fft, 7)
        for win_length in sc.WIN_LENGTHS[n_fft]:
            got = stft_spec.amp_sp(x, n_fft, hop, win_length=win_length)
            assert _rel(got, sc.direct_amp_sp(x, n_fft, hop, win_length)) <= 1e-13, (n_fft, win_length)
    # a window of one point (at index (n_fft - 1) // 2) picks one sample per frame: a flat spectrum
    x = sc.signal(3000, 8)
    got = stft_spec.amp_sp(x, 1024, 80, win_length=1)
    picked = np.abs(x[np.abs(np.arange(38) * 80 - 1)])
    assert _rel(got, np.repeat(picked[:, None], 513, axis=1) / np.sqrt(513)) <= 1e-13


@pytest.mark.parametrize("n_fft,hop,win_length", sc.GL_CASES)
def test_istft_of_stft_reconstructs_at_the_new_hops(n_fft, hop, win_length):
    for T in sc.gl_frame_counts(n_fft, hop)[:4]:
        x = np.random.default_rng(T).standard_normal(hop * (T - 1))
        for pad_mode in sc.PAD_MODES:
            X = gl.stft(x, hop, n_fft, win_length, pad_mode)
            assert X.shape == (T, n_fft // 2 + 1)
            y = gl.istft(X, hop, n_fft, win_length)
            assert _rel(y, x) <= 1e-12, (T, pad_mode)


@pytest.mark.parametrize("n_mels", [1, 2, 64, 65])
def test_solve_reaches_scipy_nnls(n_mels):
    import scipy.optimize
    A = mi.basis(16000, 1024, n_mels, np.float64)
    B = sc.mel_bands(16000, 1024, n_mels)[::8].astype(np.float64)
    X, n = mi.solve(A, B)
    assert (X >= 0).all() and n.max() <= mi.CAP
    for b, x in zip(B, X):
        xs, _ = scipy.optimize.nnls(A, b)
        gap = (np.sum((A @ x - b) ** 2) - np.sum((A @ xs - b) ** 2)) / np.sum(b ** 2)
        assert gap <= 1e-9, (n_mels, gap)
