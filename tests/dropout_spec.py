"""Restatement of the dropout rule of csrc/dropout.h in numpy (uint64 arithmetic, no device), and a float64
forward / backward of a Linear chain under given masks: what the dropout tests compare the kernels with."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two; returns the four output words (uint64 arrays
    holding 32-bit values)"""
    c = [np.asarray(v, dtype=np.uint64) & LOW for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & LOW for v in key]
    for _ in range(10):
        p0 = M0 * c[0]
        p1 = M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k[0], p1 & LOW, (p0 >> S32) ^ c[3] ^ k[1], p0 & LOW]
        k = [(k[0] + W0) & LOW, (k[1] + W1) & LOW]
    return c


def threshold(p):
    return int(min(2 ** 32 - 1, np.rint(np.float64(p) * 2.0 ** 32)))


def scale_f32(p):
    """1 / (1 - p) as torch computes it: float32 of 1 - p, then a float32 division"""
    return np.float32(1.0) / np.float32(1.0 - float(p))


def keep_mask(M, N, p, seed, salt, row_offset=0):
    """bool [M, N]: True where element (row, col) is kept"""
    seed = int(seed)
    rows = (np.arange(M, dtype=np.uint64) + np.uint64(row_offset))[:, None]
    cols = np.arange(N, dtype=np.uint64)[None, :]
    rows, cols = np.broadcast_arrays(rows, cols)
    words = philox4x32_10((rows & LOW, rows >> S32, cols >> np.uint64(2), np.uint64(salt)),
                          (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)))
    word = np.choose((cols & np.uint64(3)).astype(np.int64), words)
    return word >= np.uint64(threshold(p))


ACTS = {
    None: (lambda z: z, lambda y: np.ones_like(y)),
    "tanh": (np.tanh, lambda y: 1.0 - y * y),
    "sigmoid": (lambda z: 1.0 / (1.0 + np.exp(-z)), lambda y: y * (1.0 - y)),
    "relu": (lambda z: np.maximum(z, 0.0), lambda y: (y > 0).astype(np.float64)),
}


def chain_forward(x, layers, acts, masks, ps):
    """float64 forward of Linear (+ activation) (+ dropout) layers.  layers: [(w [N, K], b [N])], acts: names of
    ACTS, masks: keep masks (or None), ps: the probabilities.  The factor of a kept element is the float32 scale the
    kernels use.  Returns (outputs after dropout, outputs before dropout)."""
    h = np.asarray(x, dtype=np.float64)
    outs, ys = [], []
    for (w, b), act, m, p in zip(layers, acts, masks, ps):
        y = ACTS[act][0](h @ np.asarray(w, np.float64).T + np.asarray(b, np.float64))
        ys.append(y)
        h = y if m is None else y * m * np.float64(scale_f32(p))
        outs.append(h)
    return outs, ys


def chain_backward(x, layers, acts, masks, ps, dout):
    """float64 gradients of sum(out * dout) for chain_forward: (dx, [(dw, db)])"""
    outs, ys = chain_forward(x, layers, acts, masks, ps)
    d = np.asarray(dout, dtype=np.float64)
    grads = [None] * len(layers)
    for i in range(len(layers) - 1, -1, -1):
        w = np.asarray(layers[i][0], np.float64)
        if masks[i] is not None:
            d = d * masks[i] * np.float64(scale_f32(ps[i]))
        dz = d * ACTS[acts[i]][1](ys[i])
        inp = outs[i - 1] if i > 0 else np.asarray(x, np.float64)
        grads[i] = (dz.T @ inp, dz.sum(axis=0))
        d = dz @ w
    return d, grads


def masked_mse(pred, target, row_valid, n_valid):
    """(loss, d loss / d pred) of NamedLoss(MSELoss, 'mean_per_frame') in float64"""
    diff = (np.asarray(pred, np.float64) - np.asarray(target, np.float64)) * np.asarray(row_valid, np.float64)[:, None]
    scale = 1.0 / (float(n_valid) * pred.shape[1])
    return scale * np.sum(diff * diff), 2.0 * scale * diff
