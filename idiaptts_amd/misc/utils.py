"""Frame utilities with the reference's exact semantics (idiaptts/misc/utils.py:40-105).

`interpolate_lin` is sequential index logic on a few thousand frames and stays on the host (as
in the reference); it reproduces the reference's quirks bit for bit:
the output aliases the scanned array, the interpolation target is reached one frame early, and a
gap whose next voiced frame is the LAST frame is filled with the last voiced value (overwriting
that frame).  `compute_deltas` = np.gradient in float32; on the device it is part of
idiaptts_amd.ops.assemble_cmp (itts_assemble_cmp_f32: static, delta and delta-delta columns at once).
"""
import numpy as np


def interpolate_lin(data):
    """Continuous f0/lf0 + V/UV from a discontinuous contour (reference: misc/utils.py:40-86).

    :return: (interpolated [T,1] in the input dtype, vuv [T,1] float64)
    """
    data = np.reshape(np.copy(data), (data.size, 1))
    n = data.size
    vuv_vector = np.zeros((n, 1))
    vuv_vector[data > 0.0] = 1.0

    flat = data[:, 0]  # view: writes go to `data`, which is also what the scan reads (aliasing)
    last_value = 0.0
    i = 0
    while i < n:
        if flat[i] <= 0.0:
            # first voiced frame after i; if none: last index (python's for-else free `j`)
            j = i + 1
            if j < n:
                nz = np.nonzero(flat[j:] > 0.0)[0]
                j = j + int(nz[0]) if nz.size else n - 1
            if j < n - 1:
                if last_value > 0.0:
                    step = (flat[j] - flat[i - 1]) / float(j - i)
                    ks = np.arange(1, j - i + 1).astype(flat.dtype)
                    flat[i:j] = flat[i - 1] + step * ks
                else:
                    flat[i:j] = flat[j]
                # the filled frames are re-scanned by the reference; positive fills just update
                # last_value, non-positive fills would be handled again (cannot happen for j<n-1
                # because flat[j] > 0 and flat[i-1] > 0), so continue scanning from i.
                if flat[i] > 0.0:
                    last_value = flat[j - 1]
                    i = j
                    continue
                i += 1
                continue
            else:
                flat[i:] = last_value
                if last_value > 0.0:
                    break          # tail is positive: every remaining frame keeps last_value
                i += 1             # tail filled with 0: rescanned frame by frame, same result
                continue
        else:
            last_value = flat[i]
        i += 1
    return data, vuv_vector


def compute_deltas(labels):
    """np.gradient along time, float32 (reference: misc/utils.py:103-105)."""
    return np.gradient(labels, axis=0).astype(dtype=np.float32)


def _multiplier(in_to_out_multiplier):
    if in_to_out_multiplier < 1:
        raise NotImplementedError("sample_linearly with in_to_out_multiplier = {} < 1 (down-sampling) is not "
                                  "implemented, as in the reference.".format(in_to_out_multiplier))
    return int(in_to_out_multiplier)          # (truncated, as the reference's int(...))


def sample_linearly_batch(samples, in_to_out_multiplier, dtype=np.float32):
    """`sample_linearly` of a list of [T_s, D] arrays (numpy, or float32 / float64 tensors on the device) from one
    launch of itts_sample_linearly: a list of device tensors [m * T_s, D] of `dtype` (views of one buffer).  The
    conditioning features of a sample-level vocoder go through this to reach the sample rate
    (reference WaveNetVocoderTrainer.py:141-173)."""
    import torch
    from idiaptts_amd import lib, ops
    m = _multiplier(in_to_out_multiplier)
    out_dtype = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}.get(np.dtype(dtype))
    if out_dtype is None:
        raise NotImplementedError("sample_linearly to dtype {} is not implemented (float32, float64).".format(dtype))
    if len(samples) == 0:
        return []
    rows = []
    for n, s in enumerate(samples):
        t = s if torch.is_tensor(s) else torch.from_numpy(np.ascontiguousarray(s))
        if not t.is_floating_point():
            t = t.double()                    # (interp1d takes integers as float64)
        if t.dim() == 1:
            t = t.unsqueeze(-1)
        if t.dim() != 2:
            raise ValueError("sample {} must be [T, D], got {}.".format(n, tuple(t.shape)))
        if t.shape[0] < 2:
            raise ValueError("sample {} has T = {} frame(s): linear interpolation needs at least 2 (scipy's interp1d "
                             "gives NaN for a single point).".format(n, t.shape[0]))
        if t.shape[1] != (rows[0].shape[1] if rows else t.shape[1]):
            raise ValueError("sample {} has {} features, sample 0 has {}.".format(n, t.shape[1], rows[0].shape[1]))
        rows.append(t)
    lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    in_dtype = torch.float64 if any(t.dtype == torch.float64 for t in rows) else torch.float32
    x = torch.cat([t.to(device=dev, dtype=in_dtype) for t in rows], dim=0)
    offsets = [0]
    for t in rows:
        offsets.append(offsets[-1] + t.shape[0])
    if m == 1:
        y, out_off = x.to(out_dtype), offsets
    else:
        y, out_off = ops.sample_linearly(x, offsets, m, out_dtype)
    return [y[out_off[s]:out_off[s + 1]] for s in range(len(rows))]


def sample_linearly(sample, in_to_out_multiplier, dtype=np.float32):
    """[T, D] -> [m T, D] at x_new = linspace(0, T - 1, m T), m = int(in_to_out_multiplier), interpolated linearly
    in float64 and cast to dtype (reference: misc/utils.py:89-100, on scipy's interp1d); numpy in, numpy out, through
    the same kernel as `sample_linearly_batch`.  A multiplier of 1 returns the input itself, one below 1 raises
    NotImplementedError, as there.  T = 1 is refused by name: interp1d returns NaN for it."""
    m = _multiplier(in_to_out_multiplier)
    if not in_to_out_multiplier > 1:
        return sample
    if m == 1:                                  # (1 < multiplier < 2: linspace with T points is the input's own grid)
        return np.array(sample, dtype=dtype)
    sample = np.asarray(sample)
    out = sample_linearly_batch([sample], m, dtype)[0].cpu().numpy()
    return out.reshape((out.shape[0],) + sample.shape[1:])
