"""The shared cases of the discretized mixture-of-logistics loss (csrc/mol.hip; tests/test_gpu_mol.py,
tests/test_mol_cases.py, tests/golden/make_golden_mol.py): a float64 restatement of the loss and of its gradient in
numpy, written from the formulas and not from autograd, the input generator and the bounds.  Nothing here touches a
GPU."""
import math

import numpy as np

from xent_cases import ELEM_BOUND, REL_BOUND  # noqa: F401  (the dense layers' bounds: the first half of the tolerance)

NUM_CLASSES = (256, 65536)
LOG_SCALE_MINS = (-7.0, math.log(1e-14))
# the stored cases of tests/golden/mol_fixture.npz: (K, num_classes, log_scale_min, shift, hinge)
GOLDEN_B, GOLDEN_T = 2, 12
GOLDEN_CASES = [(K, nc, lsm, shift, hinge) for K in (1, 10) for nc in NUM_CLASSES for lsm in LOG_SCALE_MINS
                for shift in (None, 1, 3) for hinge in (True, False)]
# the kernel sweep
SWEEP_B = 2
SWEEP_K = (1, 2, 3, 10, 64)         # 64: the largest; 10: the usual; the workgroup is 256 lanes at all of them but 64
SWEEP_T = (2, 63, 64, 65, 257)      # around the 64 lanes of the smallest workgroup, and more than one workgroup of 256
SWEEP_SHIFT = (0, 1, 3)
HAND_Y = (-1.0, 1.0, -0.9995, 0.9995)
REDUCTIONS = ("mean_per_frame", "mean_per_sample", "mean", "sum", "none")


def case_name(K, nc, lsm, shift, hinge):
    return "K{}_nc{}_lsm{}_s{}_h{}".format(K, nc, int(round(-lsm)), shift, int(hinge))


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def branch_terms(x, y, num_classes, log_scale_min, shift):
    """float64 pieces of the frames that have a loss: dict of raw log-scales r, clamped s, inv, u, v, mid, d, delta
    [B, K, Tn] (delta as the product sigmoid(u) sigmoid(-v) (1 - e^-d): no cancellation) and the target yy [B, 1, Tn]"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    B, C, T = x.shape
    K, s0 = C // 3, shift or 0
    Tn = T - s0
    logit, mean, r = x[:, :K, :Tn], x[:, K:2 * K, :Tn], x[:, 2 * K:, :Tn]
    yy = y.reshape(B, 1, T)[:, :, s0:]
    s = np.maximum(r, log_scale_min)
    inv = np.exp(-s)
    h = 1.0 / (num_classes - 1)
    c = yy - mean
    u, v, mid = inv * (c + h), inv * (c - h), inv * c
    d = inv * (2.0 * h)
    E = -np.expm1(-d)
    delta = _sigmoid(u) * _sigmoid(-v) * E
    return dict(logit=logit, r=r, s=s, inv=inv, u=u, v=v, mid=mid, d=d, E=E, delta=delta, yy=yy, K=K, Tn=Tn)


def _quiet(fn):
    """rows of weight 0 may hold NaN and inf: numpy need not warn about them"""
    def wrapped(*args, **kwargs):
        with np.errstate(all="ignore"):
            return fn(*args, **kwargs)
    wrapped.__doc__ = fn.__doc__
    return wrapped


@_quiet
def reference64(x, y, w=None, num_classes=256, log_scale_min=-7.0, shift=None, hinge=True, as_reference=False):
    """float64 restatement: dict of elem [B, T - shift] = w l, loss = sum(elem) and grad [B, 3K, T] = d loss / d x
    (zeros in the last `shift` frames).  Rows of weight 0 give exactly 0 whatever they hold.

    cdf_delta and its derivatives come from the product form of csrc/mol.hip's header, which does not cancel, and
    softplus is the function itself.  With `as_reference` both are evaluated as the reference's torch flow does:
    sigmoid(u) - sigmoid(v) with the two chain-rule terms sigmoid'(u) / delta and -sigmoid'(v) / delta added up (even
    in float64 that loses up to 1e-16 / 2e-5 of a delta just above the switch), and torch's F.softplus, which
    returns x itself above its threshold of 20 (2e-9 off there, its derivative exactly 1).  The comparison with the
    reference's float64 fixture at 1e-12 needs this form; the exact form, held against it at 1e-8, is what the
    kernel is measured against."""
    p = branch_terms(x, y, num_classes, log_scale_min, shift)
    B, C, T = np.shape(x)
    K, Tn = p["K"], p["Tn"]
    u, v, mid, s, inv, d, E, yy = (p[k] for k in ("u", "v", "mid", "s", "inv", "d", "E", "yy"))
    with np.errstate(all="ignore"):
        su, sv, snu, snv = _sigmoid(u), _sigmoid(v), _sigmoid(-u), _sigmoid(-v)
        if as_reference:
            sp = lambda a: np.where(a > 20.0, a, _softplus(a))              # noqa: E731
            dsp = lambda a: np.where(a > 20.0, 1.0, _sigmoid(a))            # noqa: E731
        else:
            sp, dsp = _softplus, _sigmoid
        low = np.broadcast_to(yy < -0.999, u.shape)
        high = np.broadcast_to(yy > 0.999, u.shape)
        wide = p["delta"] > 1e-5
        # value, d/dmean, d/ds of the four branches
        LA, mA, sA = u - sp(u), -inv * (1.0 - dsp(u)), -u * (1.0 - dsp(u))
        LB, mB, sB = -sp(v), inv * dsp(v), v * dsp(v)
        if as_reference:
            import torch                        # (its sigmoid's own bits: one ulp of it is 5e-12 of such a delta)
            tu, tv = torch.sigmoid(torch.from_numpy(u)).numpy(), torch.sigmoid(torch.from_numpy(v)).numpy()
            delta = tu - tv
            wide = delta > 1e-5
            g_u, g_v = (1.0 - tu) * tu / delta, -(1.0 - tv) * tv / delta
            LC, mC, sC = np.log(np.maximum(delta, 1e-12)), -inv * g_u - inv * g_v, -u * g_u - v * g_v
        else:
            LC = -_softplus(-u) - _softplus(v) + np.log(E)
            mC = inv * (su - snv)
            sC = v * (su - snv) - d * snu / (snv * E)
        LD = mid - s - 2.0 * sp(mid) - math.log((num_classes - 1) / 2.0)
        mD, sD = inv * (2.0 * dsp(mid) - 1.0), mid * (2.0 * dsp(mid) - 1.0) - 1.0
        if not as_reference:                    # (1 - sigmoid(u) and u - softplus(u) without the cancellation)
            LA, mA, sA = -_softplus(-u), -inv * snu, -u * snu
    sel = lambda a, b_, c_, d_: np.where(low, a, np.where(high, b_, np.where(wide, c_, d_)))  # noqa: E731
    L, gm, gs = sel(LA, LB, LC, LD), sel(mA, mB, mC, mD), sel(sA, sB, sC, sD)
    logit = p["logit"]
    lmax = logit.max(axis=1, keepdims=True)
    el = np.exp(logit - lmax)
    softmax = el / el.sum(axis=1, keepdims=True)
    q = L + (logit - lmax) - np.log(el.sum(axis=1, keepdims=True))
    qmax = q.max(axis=1, keepdims=True)
    eq = np.exp(q - qmax)
    lse = qmax[:, 0] + np.log(eq.sum(axis=1))
    resp = eq / eq.sum(axis=1, keepdims=True)
    r = p["r"]
    nll = -lse
    hinge_on = (-r - math.log(num_classes) > 0) & bool(hinge)
    if hinge:
        nll = nll + np.maximum(0.0, -r - math.log(num_classes)).sum(axis=1)
    w = np.ones((B, Tn)) if w is None else np.asarray(w, dtype=np.float64).reshape(B, Tn)
    live = w != 0
    elem = np.where(live, w * np.where(live, nll, 0.0), 0.0)
    grad = np.zeros((B, C, T))
    wl = w[:, None, :]
    grad[:, :K, :Tn] = wl * (softmax - resp)
    grad[:, K:2 * K, :Tn] = wl * (-resp * gm)
    grad[:, 2 * K:, :Tn] = wl * (-resp * gs * (r >= log_scale_min) - hinge_on)
    grad[:, :, :Tn] = np.where(live[:, None, :], grad[:, :, :Tn], 0.0)
    return dict(elem=elem, loss=elem.sum(), grad=grad)


def offending(x, y, num_classes, log_scale_min, shift):
    """[B, K, Tn] mask of the mixture entries too close to one of the loss's switches for a float32 evaluation to
    be sure of the side: cdf_delta in (0.5e-5, 2e-5), a raw log-scale within 1e-3 of log_scale_min, a hinge argument
    within 1e-3 of 0"""
    p = branch_terms(x, y, num_classes, log_scale_min, shift)
    return (((p["delta"] > 0.5e-5) & (p["delta"] < 2e-5)) | (np.abs(p["r"] - log_scale_min) < 1e-3)
            | (np.abs(-p["r"] - math.log(num_classes)) < 1e-3))


def y_in_band(y):
    a = np.abs(np.asarray(y, dtype=np.float64))
    return (a > 0.998) & (a < 0.9999)


def inputs(B, K, T, num_classes, log_scale_min, shift, seed=0):
    """(x [B, 3K, T] float32, y [B, 1, T] float32): logits randn, means 0.6 randn, log-scales 1.5 randn - 3 (a
    tenth of them 6 lower, to reach the clamp and the hinge), targets uniform in (-1, 1).  Entries that `offending`
    or `y_in_band` name are drawn again until none is left (asserted, on the float32 values in float64); then the
    exact targets -1, 1, -0.9995, 0.9995 are placed by hand on the first frames that have a loss, so that both edge
    branches occur and |y| just inside 0.999 does too -- these four are the only targets allowed in the band."""
    rng = np.random.default_rng(1000003 * seed + 7919 * K + 31 * T + (shift or 0) + num_classes % 1000)
    s0 = shift or 0

    def draw_ms(n):
        low = rng.random(n) < 0.1
        return 0.6 * rng.standard_normal(n), 1.5 * rng.standard_normal(n) - 3.0 - 6.0 * low

    y = rng.uniform(-1.0, 1.0, size=(B, 1, T)).astype(np.float32)
    for _ in range(100):
        bad = y_in_band(y)
        if not bad.any():
            break
        y[bad] = rng.uniform(-1.0, 1.0, size=int(bad.sum())).astype(np.float32)
    assert not y_in_band(y).any()
    used = [(b, t) for t in range(s0, T) for b in range(B)]
    for (b, t), val in zip(used, HAND_Y):
        y[b, 0, t] = val
    x = np.empty((B, 3 * K, T), dtype=np.float32)
    x[:, :K] = rng.standard_normal((B, K, T))
    m, s = draw_ms(B * K * T)
    x[:, K:2 * K], x[:, 2 * K:] = m.reshape(B, K, T), s.reshape(B, K, T)
    for _ in range(100):
        bad = np.zeros((B, K, T), dtype=bool)
        bad[:, :, :T - s0] = offending(x, y, num_classes, log_scale_min, shift)
        # (the frames without a loss are held to the conditions on the log-scale too, at no cost)
        tail = x[:, 2 * K:, T - s0:].astype(np.float64)
        bad[:, :, T - s0:] = (np.abs(tail - log_scale_min) < 1e-3) | (np.abs(-tail - math.log(num_classes)) < 1e-3)
        if not bad.any():
            break
        m, s = draw_ms(int(bad.sum()))
        x[:, K:2 * K][bad], x[:, 2 * K:][bad] = m, s
    assert not offending(x, y, num_classes, log_scale_min, shift).any()
    assert np.isin(y[y_in_band(y)], np.float32(HAND_Y)).all()
    return x, y


def branch_counts(x, y, num_classes, log_scale_min, shift):
    """entries per branch (low edge, high edge, cdf_delta > 1e-5, centre of the bin)"""
    p = branch_terms(x, y, num_classes, log_scale_min, shift)
    low = np.broadcast_to(p["yy"] < -0.999, p["u"].shape)
    high = np.broadcast_to(p["yy"] > 0.999, p["u"].shape) & ~low
    wide = (p["delta"] > 1e-5) & ~low & ~high
    return int(low.sum()), int(high.sum()), int(wide.sum()), int((~low & ~high & ~wide).sum())


def torch32(torch, x, y, w, num_classes, log_scale_min, shift, hinge):
    """the reference's flow in torch float32 on the CPU (its formulas, blended conditions and two-sigmoid difference
    restated) with autograd of sum(w l): dict of elem, loss, grad -- the second half of the tolerance"""
    import torch.nn.functional as F
    leaf = torch.as_tensor(x).clone().requires_grad_(True)
    yt = torch.as_tensor(y)
    s0 = shift or 0
    T = leaf.shape[2]
    inp, tgt = leaf[..., :T - s0], yt[..., s0:]
    K = inp.shape[1] // 3
    yh = inp.transpose(1, 2)
    logit, mean = yh[..., :K], yh[..., K:2 * K]
    ls = torch.clamp(yh[..., 2 * K:], min=log_scale_min)
    yy = tgt.transpose(1, 2).expand_as(mean)
    c = yy - mean
    inv = torch.exp(-ls)
    plus_in = inv * (c + 1. / (num_classes - 1))
    min_in = inv * (c - 1. / (num_classes - 1))
    cdf_delta = torch.sigmoid(plus_in) - torch.sigmoid(min_in)
    mid_in = inv * c
    log_pdf_mid = mid_in - ls - 2. * F.softplus(mid_in)
    c3 = (cdf_delta > 1e-5).float()
    o3 = c3 * torch.log(torch.clamp(cdf_delta, min=1e-12)) + (1. - c3) * (log_pdf_mid - np.log((num_classes - 1) / 2))
    c2 = (yy > 0.999).float()
    o2 = c2 * -F.softplus(min_in) + (1. - c2) * o3
    c1 = (yy < -0.999).float()
    lp = c1 * (plus_in - F.softplus(plus_in)) + (1. - c1) * o2
    lp = lp + F.log_softmax(logit, -1)
    mx = lp.max(dim=-1, keepdim=True).values
    nll = -(mx[..., 0] + torch.log(torch.exp(lp - mx).sum(dim=-1)))
    if hinge:
        nll = nll + torch.clamp(-inp[:, 2 * K:, :] - math.log(num_classes), min=0.0).sum(dim=1)
    elem = nll * torch.as_tensor(w, dtype=torch.float32).reshape(nll.shape)
    elem.sum().backward()
    return dict(elem=elem.detach(), loss=elem.detach().sum(), grad=leaf.grad)


def errors(got, ref):
    """(relative error in the 2-norm, largest element error over max(1, max|ref|)) of a float64 pair"""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return float(np.linalg.norm(d) / (np.linalg.norm(ref) + 1e-30)), float(d.max() / max(1.0, np.abs(ref).max()))


def check(product, got, ref, t32, what=""):
    """asserts `got` against the float64 `ref`: the bound is the larger of the dense layers' (REL_BOUND, ELEM_BOUND)
    and twice the error of torch's own float32 flow `t32` on the same data.  Prints and returns the errors as
    fractions of their bound."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    t32 = np.asarray(t32, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape, (product, what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (product, what, "non-finite values")
    r32, e32 = errors(t32, ref)
    tol_rel, tol_el = max(REL_BOUND[product], 2 * r32), max(ELEM_BOUND, 2 * e32)
    rel, el = errors(got, ref)
    print("mol {} {}: rel {:.3g} ({:.2f} of bound {:.3g}; torch32 {:.3g}), elem {:.3g} ({:.2f} of bound)".format(
        what, product, rel, rel / tol_rel, tol_rel, r32, el, el / tol_el))
    assert rel < tol_rel and el < tol_el, (product, what, rel, tol_rel, el, tol_el)
    return rel / tol_rel, el / tol_el


def reduction_weight(reduction, mask, lens):
    """the row weight NamedLoss folds a [B, T'] mask and the reduction into (reference _reduce, NamedLoss.py:113-131,
    on a loss of feature width 1): float64 [B, T']"""
    mask = np.asarray(mask, dtype=np.float64)
    B = mask.shape[0]
    if reduction == "mean_per_frame":
        return mask / float(sum(int(n) for n in lens))
    if reduction == "mean_per_sample":
        return mask / (np.asarray(lens, dtype=np.float64).reshape(B, 1) * B)
    if reduction == "mean":
        return mask / float(mask.size)
    return mask
