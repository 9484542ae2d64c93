"""Float64 numpy restatement of the DTW the package scores with (csrc/dtw.hip, ops.dtw_align, Metrics.get_metrics_dtw):

    d(i, j) = sqrt(sum_k (x[i, k] - y[j, k])^2)
    C(0, 0) = d(0, 0);  C(i, j) = d(i, j) + min(C(i-1, j-1), C(i-1, j), C(i, j-1))

a predecessor outside the grid or the band counting as +inf; on equal values the diagonal wins, then (i-1, j), then
(i, j-1).  The table is filled one anti-diagonal at a time (every cell of a diagonal depends on the two before it only),
the path is the backtrack of the choices from (T1-1, T2-1), reported from (0, 0) on."""
import math

import numpy as np

MELCD_CONST = 10.0 / math.log(10.0) * math.sqrt(2.0)


def band_centre(i, T1, T2):
    """round-half-up of i (T2-1) / (T1-1) in integers (T1 >= 2)"""
    den = T1 - 1
    return (2 * i * (T2 - 1) + den) // (2 * den)


def admissible(i, j, T1, T2, band):
    """Cell (i, j) lies in the band: |j - centre(i)| <= band; no band (None) and T1 == 1 (one path: the whole row) admit
    every cell."""
    if band is None or band < 0 or T1 == 1:
        return True
    return abs(j - band_centre(i, T1, T2)) <= band


def distances(x, y):
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    out = np.empty((len(x), len(y)), dtype=np.float64)
    for r0 in range(0, len(x), 64):
        out[r0:r0 + 64] = np.sqrt(((x[r0:r0 + 64, None, :] - y[None, :, :]) ** 2).sum(-1))
    return out


def fill(x, y, band=None):
    """(C [T1, T2] with +inf outside the band, choices [T1, T2] uint8 (0 diagonal, 1 up, 2 left; 255 outside the band),
    the smallest gap between the chosen predecessor and the runner-up over all cells that have two finite ones)"""
    d = distances(x, y)
    T1, T2 = d.shape
    Cp = np.full((T1 + 1, T2 + 1), np.inf)              # Cp[i + 1, j + 1] = C(i, j): a border of +inf
    dec = np.full((T1, T2), 255, dtype=np.uint8)
    gap = np.inf
    for s in range(T1 + T2 - 1):
        i = np.arange(max(0, s - T2 + 1), min(T1 - 1, s) + 1)
        j = s - i
        if band is not None and band >= 0 and T1 > 1:
            ok = np.abs(j - (2 * i * (T2 - 1) + (T1 - 1)) // (2 * (T1 - 1))) <= band
            i, j = i[ok], j[ok]
            if len(i) == 0:
                continue
        diag, up, left = Cp[i, j], Cp[i, j + 1], Cp[i + 1, j]
        best, ch = diag.copy(), np.zeros(len(i), dtype=np.uint8)
        m = up < best
        best[m], ch[m] = up[m], 1
        m = left < best
        best[m], ch[m] = left[m], 2
        three = np.sort(np.stack([diag, up, left]), axis=0)
        two = np.isfinite(three[1])
        if two.any():
            gap = min(gap, float((three[1] - three[0])[two].min()))
        if s == 0:
            best[:] = 0.0
        Cp[i + 1, j + 1] = d[i, j] + best
        dec[i, j] = ch
    return Cp[1:, 1:], dec, gap


def backtrack(dec):
    T1, T2 = dec.shape
    i, j, path = T1 - 1, T2 - 1, []
    while True:
        path.append((i, j))
        if i == 0 and j == 0:
            break
        ch = 2 if i == 0 else 1 if j == 0 else int(dec[i, j])
        assert ch in (0, 1, 2), "the path left the band at ({}, {})".format(i, j)
        if ch == 0:
            i, j = i - 1, j - 1
        elif ch == 1:
            i -= 1
        else:
            j -= 1
    return np.array(path[::-1], dtype=np.int32)


def dtw(x, y, band=None):
    """-> (cost, path int32 [L, 2]); (inf, empty path) when the band does not connect the corners"""
    C, dec, _ = fill(x, y, band)
    cost = float(C[-1, -1])
    if not np.isfinite(cost):
        return cost, np.zeros((0, 2), dtype=np.int32)
    return cost, backtrack(dec)


def decision_margin(x, y, band=None):
    """The smallest gap, over all cells, between the chosen predecessor and the runner-up, relative to the total cost:
    above the rounding of any float64 evaluation order, every such evaluation makes the same choices.  A band that does
    not connect the corners leaves no path to compare (which cells can be reached does not hang on rounding): inf."""
    C, _, gap = fill(x, y, band)
    return gap / float(C[-1, -1]) if np.isfinite(C[-1, -1]) else np.inf


def exhaustive_cost(x, y):
    """The minimum over EVERY monotone path from (0, 0) to (T1-1, T2-1) (steps (1,1), (1,0), (0,1)) of the summed
    distances, by enumeration; for T1, T2 <= 6."""
    d = distances(x, y)
    T1, T2 = d.shape
    assert T1 <= 6 and T2 <= 6
    best = [np.inf]

    def walk(i, j, total):
        total += d[i, j]
        if i == T1 - 1 and j == T2 - 1:
            best[0] = min(best[0], total)
            return
        if i + 1 < T1 and j + 1 < T2:
            walk(i + 1, j + 1, total)
        if i + 1 < T1:
            walk(i + 1, j, total)
        if j + 1 < T2:
            walk(i, j + 1, total)

    walk(0, 0, 0.0)
    return best[0]


def scores(org, out, band=None, path=None):
    """[MCD, F0 RMSE, VDE, BAP distortion] of (coded_sp, lf0, vuv, bap) tuples along the DTW path of the coded spectra
    without bin 0: Metrics.get_metrics' formulas over the aligned pairs (i, j)."""
    o_sp, o_lf0, o_vuv, o_bap = (np.asarray(a, dtype=np.float64) for a in org)
    p_sp, p_lf0, p_vuv, p_bap = (np.asarray(a, dtype=np.float64) for a in out)
    if path is None:
        cost, path = dtw(o_sp[:, 1:], p_sp[:, 1:], band)
    pi, pj = path[:, 0], path[:, 1]
    L = len(path)
    mcd = MELCD_CONST * np.sqrt(((o_sp[pi, 1:] - p_sp[pj, 1:]) ** 2).sum(-1)).sum() / L
    v = o_vuv.reshape(-1)[pi]
    se = (np.exp(o_lf0.reshape(-1)[pi]) - np.exp(p_lf0.reshape(-1)[pj])) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        f0 = float(np.sqrt(np.float64((se * v).sum()) / np.float64(v.sum())))
    vde = float((v != p_vuv.reshape(-1)[pj]).sum()) / L
    if p_bap.ndim > 1 and p_bap.shape[1] > 1:
        bap = MELCD_CONST * np.sqrt(((o_bap[pi, 1:] - p_bap[pj, 1:]) ** 2).sum(-1)).mean()
    else:
        bap = MELCD_CONST * math.sqrt(((o_bap.reshape(-1)[pi] - p_bap.reshape(-1)[pj]) ** 2).mean())
    return [float(mcd), f0, vde, float(bap)]
