"""A float64 restatement of the WaveNet vocoder network (idiaptts_amd.nn.WaveNet), independent of its code: the
teacher-forced forward (torch on the CPU, any dtype, differentiable), step-by-step generation with given uniforms and
per-layer ring buffers (numpy), and the two draws.

Specification (the published architecture, parameter names of the wavenet_vocoder package):
  first_conv 1x1 (out_channels, or 1 with scalar input, -> R); layer l has dilation 2 ** (l % (layers // stacks)):
  h = conv(x) causal (taps x[t - (k - 1 - j) d], zeros before the start) + conv1x1c(c), halves a | b,
  z = tanh(a) sigmoid(b), skip += conv1x1_skip(z), x = (conv1x1_out(z) + x) sqrt(1/2); head relu, 1x1, relu, 1x1.
  Weight norm: w = g v / |v|, the norm over everything but the output channel.
Draws: classes by inverse CDF -- the number of classes whose cumulative probability is <= u, at most C - 1; mixture
of logistics -- the mixture by the same rule at u0, then clamp(mean + exp(max(log_scale, log_scale_min)) (log u1 -
log(1 - u1)), -1, 1).

`generate(..., margin)` shapes its INPUT: a uniform that falls within `margin` of an edge of its own float64 CDF is
replaced by the midpoint of the interval it fell in -- or, when that interval is narrower than 2 margin, by the
midpoint of the widest interval (at least 1 / C wide, so 1 / (2 C) from its edges; C <= 256 keeps that above margin =
1e-3) -- rounded to float32.  The adjusted uniforms are returned and are what a float32 implementation is then
given: its CDF differs by ~1e-6, so its choices must equal the spec's.  The margin is no tolerance on anything."""
import collections
import math

import numpy as np

Net = collections.namedtuple("Net", "layers stacks R G S k cin C scalar log_scale_min")

SMALL = dict(layers=4, stacks=2, R=32, G=32, S=16, cin=5)


def small(k=2, mol=False):
    """the small test model: 4 layers / 2 stacks, R = G = 32, S = 16, cin 5; 16 classes or K = 2 mixtures"""
    return Net(k=k, C=6 if mol else 16, scalar=bool(mol), log_scale_min=-7.0, **SMALL)


DEFAULT = Net(layers=24, stacks=4, R=512, G=512, S=256, k=3, cin=80, C=256, scalar=False, log_scale_min=-7.0)


def dilations(net):
    return [2 ** (l % (net.layers // net.stacks)) for l in range(net.layers)]


def receptive_field(net):
    return 1 + (net.k - 1) * sum(dilations(net))


def conv_shapes(net):
    """ordered {prefix: (Cout, Cin, k, has_bias)} of every convolution, prefixes as in the state dict"""
    shapes = collections.OrderedDict()
    shapes["first_conv"] = (net.R, 1 if net.scalar else net.C, 1, True)
    for l in range(net.layers):
        p = "conv_layers.{}.".format(l)
        shapes[p + "conv"] = (net.G, net.R, net.k, True)
        if net.cin > 0:
            shapes[p + "conv1x1c"] = (net.G, net.cin, 1, False)
        shapes[p + "conv1x1_out"] = (net.R, net.G // 2, 1, True)
        shapes[p + "conv1x1_skip"] = (net.S, net.G // 2, 1, True)
    shapes["last_conv_layers.1"] = (net.S, net.S, 1, True)
    shapes["last_conv_layers.3"] = (net.C, net.S, 1, True)
    return shapes


def state_dict_shapes(net, weight_normalization=True, prefix="model."):
    """{key: shape} of the wrapper's state dict"""
    out = {}
    for name, (co, ci, k, bias) in conv_shapes(net).items():
        if bias:
            out[prefix + name + ".bias"] = (co,)
        if weight_normalization:
            out[prefix + name + ".weight_g"] = (co, 1, 1)
            out[prefix + name + ".weight_v"] = (co, ci, k)
        else:
            out[prefix + name + ".weight"] = (co, ci, k)
    return out


def random_state(net, seed=0, weight_normalization=True, scale=1.0):
    """a state dict of float32-valued float64 arrays: weights N(0, scale / sqrt(k Cin)) (so that activations stay O(1)
    through the layers), g uniform in (0.5, 1.5) times the norm of v, biases N(0, 0.1)"""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)    # noqa: E731
    sd = collections.OrderedDict()
    for name, (co, ci, k, bias) in conv_shapes(net).items():
        v = f32(rng.standard_normal((co, ci, k)) * scale / math.sqrt(k * ci))
        if bias:
            sd["model." + name + ".bias"] = f32(0.1 * rng.standard_normal(co))
        if weight_normalization:
            norm = np.sqrt((v ** 2).sum(axis=(1, 2), keepdims=True))
            sd["model." + name + ".weight_g"] = f32(norm * rng.uniform(0.5, 1.5, size=(co, 1, 1)))
            sd["model." + name + ".weight_v"] = v
        else:
            sd["model." + name + ".weight"] = v
    return sd


# ---- teacher-forced forward (torch, differentiable) --------------------------------------------------------------
def _weight(torch, sd, name):
    if name + ".weight" in sd:
        return sd[name + ".weight"]
    v, g = sd[name + ".weight_v"], sd[name + ".weight_g"]
    return g * v / torch.sqrt((v * v).sum(dim=(1, 2), keepdim=True))


def _conv(torch, sd, name, x, dilation=1):
    """causal convolution over time of x [B, T, Cin] -> [B, T, Cout]: sum_j x[t - (k - 1 - j) d] W[:, :, j]^T + b"""
    w = _weight(torch, sd, name)
    k, T = w.shape[2], x.shape[1]
    y = None
    for j in range(k):
        back = (k - 1 - j) * dilation
        if back >= T:
            continue
        xs = x if back == 0 else torch.cat([x.new_zeros(x.shape[0], back, x.shape[2]), x[:, :T - back]], dim=1)
        term = xs @ w[:, :, j].t()
        y = term if y is None else y + term
    if name + ".bias" in sd:
        y = y + sd[name + ".bias"]
    return y


def forward(torch, net, sd, x, c=None):
    """sd: {key: torch tensor} (keys with the "model." prefix), x [B, Cin0, T], c [B, cin, T] -> [B, C, T] in the
    dtype of the tensors"""
    sd = {k[len("model."):]: v for k, v in sd.items()}
    h = _conv(torch, sd, "first_conv", x.transpose(1, 2))
    ct = c.transpose(1, 2) if net.cin > 0 else None
    skips = 0
    H = net.G // 2
    for l, d in enumerate(dilations(net)):
        p = "conv_layers.{}.".format(l)
        a = _conv(torch, sd, p + "conv", h, d)
        if ct is not None:
            a = a + _conv(torch, sd, p + "conv1x1c", ct)
        z = torch.tanh(a[..., :H]) * torch.sigmoid(a[..., H:])
        skips = skips + _conv(torch, sd, p + "conv1x1_skip", z)
        h = (_conv(torch, sd, p + "conv1x1_out", z) + h) * math.sqrt(0.5)
    y = _conv(torch, sd, "last_conv_layers.1", torch.relu(skips))
    y = _conv(torch, sd, "last_conv_layers.3", torch.relu(y))
    return y.transpose(1, 2)


def teacher_input(net, out):
    """the network input that generating `out` ([B, T] classes or samples) went through: position t holds sample
    t - 1, position 0 the all-zero input; float64 [B, Cin0, T]"""
    out = np.asarray(out)
    B, T = out.shape
    if net.scalar:
        x = np.zeros((B, 1, T))
        x[:, 0, 1:] = out[:, :-1]
    else:
        x = np.zeros((B, net.C, T))
        for b in range(B):
            x[b, out[b, :-1].astype(np.int64), np.arange(1, T)] = 1.0
    return x


# ---- the draws ---------------------------------------------------------------------------------------------------
def softmax_cdf(logits):
    e = np.exp(logits - logits.max())
    return np.cumsum(e / e.sum())


def choose(cdf, u):
    """inverse CDF: the number of entries whose cumulative probability is <= u, at most len - 1"""
    return min(int((cdf <= u).sum()), len(cdf) - 1)


def adjust_uniform(cdf, u, margin):
    """u itself, or (within `margin` of an edge of cdf) the float32 midpoint of the interval it fell in / of the
    widest interval when that one is narrower than 2 margin"""
    if margin <= 0 or np.abs(cdf[:-1] - u).min(initial=np.inf) >= margin:
        return float(u)
    edges = np.concatenate([[0.0], cdf[:-1], [1.0]])
    i = choose(cdf, u)
    if edges[i + 1] - edges[i] < 2 * margin:
        i = int(np.argmax(np.diff(edges)))
    mid = float(np.float32(0.5 * (edges[i] + edges[i + 1])))
    assert min(mid - edges[i], edges[i + 1] - mid) >= 0.9 * margin, (edges[i], edges[i + 1], margin)
    return mid


def draw_class(logits, u, margin=0.0):
    """(class, the uniform used)"""
    cdf = softmax_cdf(logits)
    u = adjust_uniform(cdf, u, margin)
    return choose(cdf, u), u


def draw_mol(params, u0, u1, log_scale_min, margin=0.0):
    """(sample, mixture, the first uniform used) from params [3 K] = logits | means | log-scales"""
    K = len(params) // 3
    k, u0 = draw_class(params[:K], u0, margin)
    scale = math.exp(max(params[2 * K + k], log_scale_min))
    x = params[K + k] + scale * (math.log(u1) - math.log1p(-u1))
    return min(max(x, -1.0), 1.0), k, u0


# ---- generation (numpy, ring buffers) ----------------------------------------------------------------------------
def _np_weight(sd, name):
    if name + ".weight" in sd:
        return sd[name + ".weight"]
    v, g = sd[name + ".weight_v"], sd[name + ".weight_g"]
    return g * v / np.sqrt((v * v).sum(axis=(1, 2), keepdims=True))


def generate(net, sd, c, lengths, uniforms, margin=0.0, initial_class=None):
    """Step-by-step generation.  sd: numpy state dict; c [B, cin, T] or None; uniforms [B, T] or [B, T, 2] (float32
    values).  Returns dict(out [B, T] classes (int64) / samples, logits [B, T, C], uniforms (adjusted, float32),
    mixture [B, T] for scalar input); positions past a row's length stay zero."""
    sd = {k[len("model."):]: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    B, T = len(lengths), max(lengths)
    dil = dilations(net)
    H = net.G // 2
    # (one contiguous [Cout, Cin] matrix per tap: a strided slice would make every product a slow one)
    W = {n: [np.ascontiguousarray(w[:, :, j]) for j in range(w.shape[2])]
         for n, w in ((n, _np_weight(sd, n)) for n in conv_shapes(net))}
    uni = np.array(uniforms, dtype=np.float64)
    out = np.zeros((B, T), dtype=np.float64 if net.scalar else np.int64)
    mixture = np.zeros((B, T), dtype=np.int64)
    logits = np.zeros((B, T, net.C))
    for b in range(B):
        rings = [np.zeros(((net.k - 1) * d + 1, net.R)) for d in dil]
        prev_class, prev_x = (-1 if initial_class is None else int(initial_class)), 0.0
        for t in range(lengths[b]):
            if net.scalar:
                x = W["first_conv"][0][:, 0] * prev_x + sd["first_conv.bias"]
            else:
                x = sd["first_conv.bias"] + (W["first_conv"][0][:, prev_class] if prev_class >= 0 else 0.0)
            skips = np.zeros(net.S)
            for l, d in enumerate(dil):
                p = "conv_layers.{}.".format(l)
                depth = rings[l].shape[0]
                rings[l][t % depth] = x
                a = sd[p + "conv.bias"].copy()
                for j in range(net.k):
                    tt = t - (net.k - 1 - j) * d
                    if tt >= 0:
                        a += W[p + "conv"][j] @ rings[l][tt % depth]
                if net.cin > 0:
                    a += W[p + "conv1x1c"][0] @ c[b, :, t]
                z = np.tanh(a[:H]) / (1.0 + np.exp(-a[H:]))
                skips += W[p + "conv1x1_skip"][0] @ z + sd[p + "conv1x1_skip.bias"]
                x = (W[p + "conv1x1_out"][0] @ z + sd[p + "conv1x1_out.bias"] + x) * math.sqrt(0.5)
            y = W["last_conv_layers.1"][0] @ np.maximum(skips, 0.0) + sd["last_conv_layers.1.bias"]
            y = W["last_conv_layers.3"][0] @ np.maximum(y, 0.0) + sd["last_conv_layers.3.bias"]
            logits[b, t] = y
            if net.scalar:
                prev_x, mixture[b, t], uni[b, t, 0] = draw_mol(y, uni[b, t, 0], uni[b, t, 1], net.log_scale_min, margin)
                out[b, t] = prev_x
            else:
                prev_class, uni[b, t] = draw_class(y, uni[b, t], margin)
                out[b, t] = prev_class
    return dict(out=out, logits=logits, uniforms=uni.astype(np.float32), mixture=mixture)


def draw_uniforms(net, B, T, seed=0):
    """float32 uniforms for a batch: [B, T] in [0, 1), or [B, T, 2] in (1e-5, 1 - 1e-5) for scalar input"""
    rng = np.random.default_rng(seed)
    if net.scalar:
        return (rng.random((B, T, 2)) * (1 - 2e-5) + 1e-5).astype(np.float32)
    return rng.random((B, T)).astype(np.float32)
