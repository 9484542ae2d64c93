"""float64 numpy restatement of the mel filter-bank inversion (the test oracle of csrc/mel_inverse.hip).

The reference decodes mel filter banks with (AudioProcessing.py:291-301, decode_sp :321-322)
  amp_sp = librosa.feature.inverse.mel_to_stft(coded_sp.T, sr=fs, n_fft=n_fft, power=1.0, norm=None).T * K
with n_fft = fs_to_frame_length(fs) when not given and K = n_fft // 2 + 1.  librosa builds
  A = librosa.filters.mel(sr=fs, n_fft=n_fft, n_mels=n_mels, dtype=coded_sp.dtype, norm=None)
-- the Slaney-scale triangles computed in float64 and stored in the input's dtype, without the Slaney factors
2 / (f[i+2] - f[i]) that extraction (norm="slaney") applies -- and solves the non-negative least-squares problem
  min_X 0.5 / B.size ||A X - B||^2   subject to   X >= 0
with librosa.util.nnls: X starts at clip(pinv(A) @ B, 0) and scipy.optimize.fmin_l_bfgs_b (m = K, default pgtol
and factr) refines it in column blocks; power 1.0 makes the final X ** (1 / power) the identity.  The stopping rule
of L-BFGS-B is loose and the minimiser is not unique (A is n_mels x K with K > n_mels), so librosa's exact output
is not a target: parity with librosa is unpinned (librosa is not a dependency).  The kernel's contract is the
NNLS problem itself, solved per frame by the fixed, deterministic iteration `solve` restates:

  x = clip(pinv(A) b, 0),  y = x,  t = 1                              (librosa's starting point)
  for i = 1 .. cap:
      g     = A^T (A y - b)
      x'    = max(y - g / L, 0)                                        (L = lambda_max(A A^T), float64)
      t'    = (1 + sqrt(1 + 4 t^2)) / 2
      y     = x' + (t - 1) / t' (x' - x),  x = x',  t = t'             (FISTA, no restart)
      if i % check == 0 and max_k |min(x_k, (A^T (A x - b))_k)| <= tol max_k |(A^T b)_k|: stop
  return K x

All arithmetic is float64 whatever the input dtype; only the basis values (rounded to the dtype) and the output
rounding follow the dtype.  A frame's result depends on nothing but its own mel bands."""
import numpy as np

import stft_spec

TOL = 1e-6          # the KKT stopping threshold, relative to max |A^T b|
CAP = 1024          # the iteration cap
CHECK = 16          # iterations between stopping tests


def basis(fs, n_fft, n_mels, dtype=np.float32):
    """librosa.filters.mel(sr=fs, n_fft=n_fft, n_mels=n_mels, norm=None, dtype=dtype): the triangles in float64,
    stored as `dtype`.  [n_mels, n_fft // 2 + 1]"""
    fft_f = np.fft.rfftfreq(n_fft, 1.0 / fs)
    f = stft_spec.mel_points(fs, n_mels)
    fdiff = np.diff(f)
    ramps = np.subtract.outer(f, fft_f)
    w = np.zeros((n_mels, n_fft // 2 + 1), dtype=dtype)
    for i in range(n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    return w


def slaney_factors(fs, n_mels):
    f = stft_spec.mel_points(fs, n_mels)
    return 2.0 / (f[2:] - f[:-2])


def lipschitz(A):
    """lambda_max(A A^T) in float64."""
    A = np.asarray(A, dtype=np.float64)
    return float(np.linalg.eigvalsh(A @ A.T)[-1])


def start(A, B):
    """librosa's starting point clip(pinv(A) b, 0) for the frames B [F, n_mels] -> [F, K]."""
    A = np.asarray(A, dtype=np.float64)
    return np.maximum(np.asarray(B, np.float64) @ np.linalg.pinv(A).T, 0.0)


def kkt(A, B, X):
    """max_k |min(x_k, g_k)| / max_k |(A^T b)_k| per frame, g = A^T (A x - b); 0 where A^T b = 0."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, np.float64)
    G = (X @ A.T - B) @ A
    num = np.abs(np.minimum(X, G)).max(axis=1)
    den = np.abs(B @ A).max(axis=1)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), num)


def solve(A, B, tol=TOL, cap=CAP, check=CHECK, iters=None):
    """The iteration above for frames B [F, n_mels] -> (X [F, K] float64, iterations taken [F]).  With `iters`
    ([F] ints) every frame runs exactly that many iterations instead (no stopping test)."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    inv_l = 1.0 / lipschitz(A)
    X = start(A, B)
    Y = X.copy()
    den = np.abs(B @ A).max(axis=1)
    n = np.full(len(B), cap if iters is None else 0, dtype=np.int64)
    todo = np.ones(len(B), dtype=bool) if iters is None else np.asarray(iters) > 0
    last = cap if iters is None else int(np.max(iters, initial=0))
    t = 1.0
    for i in range(1, last + 1):
        if not todo.any():
            break
        a = np.flatnonzero(todo)
        G = (Y[a] @ A.T - B[a]) @ A
        Xn = np.maximum(Y[a] - G * inv_l, 0.0)
        tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        Y[a] = Xn + (t - 1.0) / tn * (Xn - X[a])
        X[a] = Xn
        t = tn
        if iters is not None:
            done = np.asarray(iters)[a] == i
            n[a[done]] = i
            todo[a[done]] = False
        elif i % check == 0:
            R = (X[a] @ A.T - B[a]) @ A
            done = np.abs(np.minimum(X[a], R)).max(axis=1) <= tol * den[a]
            n[a[done]] = i
            todo[a[done]] = False
    return X, n


def mfbanks_to_amp_sp(coded_sp, fs, n_fft, tol=TOL, cap=CAP):
    """The reference's mfbanks_to_amp_sp on this iteration: [T, n_mels] -> [T, K] in the input's dtype (float32
    stays float32, anything else is float64)."""
    coded_sp = np.asarray(coded_sp)
    dtype = np.float32 if coded_sp.dtype == np.float32 else np.float64
    A = basis(fs, n_fft, coded_sp.shape[1], dtype)
    X, _ = solve(A, coded_sp, tol, cap)
    return (X * (n_fft // 2 + 1)).astype(dtype)
