"""The shared cases of the softmax cross-entropy / class-count kernels (csrc/xent.hip; tests/test_gpu_xent.py,
tests/test_xent_config.py, tests/test_xent_abi.py) and their float64 restatement: weighted row losses, the scalar
loss, the gradient, the arg-max and the confusion counts, for both layouts, with class weights, ignore_index, shift
and every reduction.  Nothing here touches a GPU."""
import numpy as np

# the dense layers' bounds (tests/lnorm_cases.py): relative error in the 2-norm per product, and the per-element bound
# as a multiple of max(1, max|ref|); the scalar loss is a sum over rows
REL_BOUND = {"elem": 2e-6, "grad": 2e-6, "loss": 3e-6}
ELEM_BOUND = 2e-5
# the ill-conditioned / degenerate cases.  Only these may use the relaxed bound.
HAZARDS = ("offset_plus_1e4", "offset_minus_1e4", "confident", "all_equal", "C1", "neg_inf_logit")

IGNORE = -100
ROWS_N = (1, 2, 7, 69)
# every width class of the class-contiguous form and both of its edges: (largest C, (lanes, steps))
PLAN_EDGES = ((4, (1, 1)), (8, (2, 1)), (16, (4, 1)), (32, (8, 1)), (64, (16, 1)), (128, (32, 1)), (256, (64, 1)),
              (512, (64, 2)), (1024, (64, 4)), (2048, (64, 8)), (4096, (64, 16)))
ROWS_C = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096)
STRIDED_B = 3
STRIDED_C = (1, 2, 5, 256, 257)      # 257: the first width whose quarter no longer stays in registers
STRIDED_T = (1, 2, 63, 64, 65, 257)
SHIFTS = (None, 1, 2)
REDUCTIONS = ("mean_per_frame", "mean_per_sample", "mean", "sum", "none")


def expected_plan(C):
    """(lanes a row, steps) written out from the design: the smallest power of two of lanes with 4 * lanes >= C up
    to the 64 of a wave, then 2, 4, 8, 16 steps of 256 columns"""
    for edge, plan in PLAN_EDGES:
        if C <= edge:
            return plan
    raise ValueError(C)


def expected_strided_plan(C):
    """(waves that share a frame, classes of each): the quarter stays in registers up to 64 classes"""
    return 4, (C + 3) // 4


def rows_inputs(torch, N, C, seed=0):
    """the well-conditioned sweep: logits randn * 3 (row losses O(1)), targets, class weights 0.5 .. 1.5, row weights
    0.5 .. 1.5 -- (x, target, cw, w)"""
    g = torch.Generator().manual_seed(100000 * seed + 17 * N + C)
    x = torch.randn(N, C, generator=g) * 3
    t = torch.randint(0, C, (N,), generator=g)
    return x, t, 0.5 + torch.rand(C, generator=g), 0.5 + torch.rand(N, generator=g)


def strided_inputs(torch, B, C, T, seed=0):
    """(x [B, C, T], one-hot target [B, C, T], class index [B, T], cw)"""
    g = torch.Generator().manual_seed(100000 * seed + 1000 * B + 31 * C + T)
    x = torch.randn(B, C, T, generator=g) * 3
    idx = torch.randint(0, C, (B, T), generator=g)
    onehot = torch.zeros(B, C, T).scatter_(1, idx[:, None, :], 1.0)
    return x, onehot, idx, 0.5 + torch.rand(C, generator=g)


def hazard_inputs(torch, name):
    """(x, target) of a HAZARDS case"""
    g = torch.Generator().manual_seed(70 + HAZARDS.index(name))
    N, C = {"offset_plus_1e4": (6, 256), "offset_minus_1e4": (6, 67), "confident": (9, 64), "all_equal": (5, 67),
            "C1": (5, 1), "neg_inf_logit": (6, 17)}[name]
    x = torch.randn(N, C, generator=g) * 3
    t = torch.randint(0, C, (N,), generator=g)
    if name == "offset_plus_1e4":
        x = x + 1e4
    elif name == "offset_minus_1e4":
        x = x - 1e4
    elif name == "confident":           # the target's logit 12 .. 20 above the rest: losses of 1e-7 .. 1e-3
        x = torch.randn(N, C, generator=g)
        x[torch.arange(N), t] = 12.0 + torch.arange(N, dtype=torch.float32)
    elif name == "all_equal":
        x = torch.full((N, C), 2.5)
    elif name == "neg_inf_logit":
        x[torch.arange(N), (t + 1) % C] = float("-inf")
    return x, t


def reference64(torch, x, target, cw=None, w=None, ignore_index=IGNORE):
    """float64 restatement on class-contiguous rows: dict of elem [N] = w[r] l_r, loss (0-d) and grad [N, C], with
    l_r = cw[t_r] (lse_r - x[r, t_r]).  Rows of weight 0 and rows whose target is ignore_index give exactly 0
    whatever they hold; a target outside [0, C) gives a NaN loss and a zero gradient row."""
    N, C = x.shape
    x = x.double()
    w = torch.ones(N, dtype=torch.float64) if w is None else w.double()
    cw = torch.ones(C, dtype=torch.float64) if cw is None else cw.double()
    elem = torch.zeros(N, dtype=torch.float64)
    grad = torch.zeros(N, C, dtype=torch.float64)
    for r in range(N):
        t = int(target[r])
        if w[r] == 0 or t == ignore_index:
            continue
        if not 0 <= t < C:
            elem[r] = float("nan")
            continue
        m = x[r].max()
        e = torch.exp(x[r] - m)
        lse = m + torch.log(e.sum())
        elem[r] = w[r] * cw[t] * (lse - x[r, t])
        p = e / e.sum()
        p[t] -= 1.0
        grad[r] = w[r] * cw[t] * p
    return dict(elem=elem, loss=elem.sum(), grad=grad)


def first_argmax(torch, x, dim):
    """the lowest index among equal maxima along dim, the first NaN if there is one (torch.argmax / torch.max),
    written out: the position of the first element that no other element beats"""
    xs = x.movedim(dim, -1).double()
    nan = torch.isnan(xs)
    filled = torch.where(nan, torch.full_like(xs, float("inf")), xs)
    filled = torch.where(nan.any(-1, keepdim=True) & ~nan, torch.full_like(xs, float("-inf")), filled)
    is_max = filled == filled.max(dim=-1, keepdim=True).values
    pos = torch.arange(xs.shape[-1]).expand_as(xs)
    return torch.where(is_max, pos, torch.full_like(pos, xs.shape[-1])).min(dim=-1).values


def reference64_strided(torch, x, onehot, cw=None, w=None, ignore_index=IGNORE, shift=None):
    """the same on [B, C, T] logits against a one-hot target (loss/OneHotCrossEntropyLoss.py): input frame t against
    target frame t + shift; elem [B, T - shift], loss, grad [B, C, T] (zeros in the last `shift` frames)"""
    B, C, T = x.shape
    s = shift or 0
    tgt = first_argmax(torch, onehot, 1)[:, s:]                              # [B, T - s]
    rows = x[:, :, :T - s].permute(0, 2, 1).reshape(-1, C)
    ref = reference64(torch, rows, tgt.reshape(-1), cw, None if w is None else w.reshape(-1), ignore_index)
    grad = torch.zeros(B, C, T, dtype=torch.float64)
    grad[:, :, :T - s] = ref["grad"].reshape(B, T - s, C).permute(0, 2, 1)
    return dict(elem=ref["elem"].reshape(B, T - s), loss=ref["loss"], grad=grad, target=tgt)


def confusion64(pred, target, C):
    """[C, C] int64 counts, rows = true class, by numpy.add.at; (matrix, number of correct rows)"""
    pred, target = np.asarray(pred, dtype=np.int64), np.asarray(target, dtype=np.int64)
    inside = (target >= 0) & (target < C)
    conf = np.zeros((C, C), dtype=np.int64)
    np.add.at(conf, (target[inside], pred[inside]), 1)
    return conf, int(np.sum(pred[inside] == target[inside]))


def reduction_weight(torch, reduction, mask, lens):
    """the row weight NamedLoss folds a [B, T'] (or [B]: T' = 1) mask and the reduction into (reference _reduce,
    NamedLoss.py:113-131, on a loss of feature width 1): float64 [B, T']"""
    mask = mask.double()
    B = mask.shape[0]
    if reduction == "mean_per_frame":
        return mask / float(sum(int(n) for n in lens))
    if reduction == "mean_per_sample":
        return mask / (torch.as_tensor(lens, dtype=torch.float64).reshape(B, *([1] * (mask.dim() - 1))) * B)
    if reduction == "mean":
        return mask / float(mask.numel())
    return mask


def errors(got, ref):
    """(relative error in the 2-norm, largest element error over max(1, max|ref|)) of a float64 pair"""
    d = (got.double() - ref).abs()
    return (d.norm().item() / (ref.norm().item() + 1e-30)), d.max().item() / max(1.0, ref.abs().max().item())


def check(product, got, ref, case=None, torch32=None):
    """asserts `got` against the float64 `ref` at the dense layers' bounds; a HAZARDS case passes `case` and torch's
    own float32 result on the same data, and the bound becomes the larger of the dense one and twice torch's error
    (the factor 2: another summation order).  Returns the errors as fractions of their tolerance."""
    tol_rel, tol_el = REL_BOUND[product], ELEM_BOUND
    if torch32 is not None:
        assert case in HAZARDS, "only the named ill-conditioned cases may use the relaxed bound"
        r32, e32 = errors(torch32, ref)
        tol_rel, tol_el = max(tol_rel, 2 * r32), max(tol_el, 2 * e32)
    got, ref = got.detach().cpu().reshape(-1), ref.reshape(-1)
    assert got.shape == ref.shape, (product, case, tuple(got.shape), tuple(ref.shape))
    assert bool(torch_isfinite(got).all()), (product, case, "non-finite values")
    rel, el = errors(got, ref)
    print("xent {} {}: rel {:.3g} ({:.2f} of tol), elem {:.3g} ({:.2f} of tol)".format(
        case or tuple(ref.shape), product, rel, rel / tol_rel, el, el / tol_el))
    assert rel < tol_rel and el < tol_el, (product, case, rel, tol_rel, el, tol_el)
    return rel / tol_rel, el / tol_el


def torch_isfinite(t):
    import torch
    return torch.isfinite(t)


def torch32(torch, x, target, cw=None):
    """torch's own float32 cross_entropy(reduction='none') and autograd of its sum on the CPU: dict of elem, loss,
    grad"""
    leaf = x.clone().requires_grad_(True)
    elem = torch.nn.functional.cross_entropy(leaf, target, weight=cw, ignore_index=IGNORE, reduction="none")
    elem.sum().backward()
    return dict(elem=elem.detach(), loss=elem.detach().sum(), grad=leaf.grad)


# ---- module-level cases (tests/golden/xent_fixture.npz; tests/golden/make_golden_xent.py, tests/test_gpu_xent_model.py) --
# name, groups (type, out_dim, nonlin, kwargs), in_dim, classes, lengths, seed
MODEL_CASES = [
    ("gru_cls", [("GRU", 8, None, {}), ("PoolLast", None, None, dict(batch_first=True)), ("Linear", 5, None, {})],
     6, 5, [11, 1, 7, 11, 5, 9], 21),
    ("conv_cls", [("Conv1d", 10, "ReLU", dict(kernel_size=3, padding=1)), ("GRU", 8, None, {}),
                  ("PoolLast", None, None, dict(batch_first=True)), ("Linear", 3, None, {})],
     7, 3, [9, 4, 12, 1, 6], 22),
]
# variant, reduction, with class weights
MODEL_VARIANTS = (("mean", "mean", False), ("sum", "sum", False), ("mean_cw", "mean", True))
ACC_NUM_PER_CLASS = [3, 0, 2, 4, 1]


def model_config(Config, case):
    """the rnn_dyn Config of a MODEL_CASES entry (the reference's package or this one: same names)"""
    _, groups, in_dim = case[:3]
    return Config(in_dim=in_dim, batch_first=True, layer_configs=[
        Config.LayerConfig(t, out_dim=d, nonlin=a, **kw) for t, d, a, kw in groups])


def model_inputs(torch, case):
    """(x [B, T, D] zero-padded, target [B, 1] int64, class weights [C]) from a generator seeded with the case's"""
    _, _, in_dim, n_cls, lens, seed = case
    g = torch.Generator().manual_seed(900 + seed)
    B, T = len(lens), max(lens)
    x = torch.randn(B, T, in_dim, generator=g)
    for b, n in enumerate(lens):
        x[b, n:] = 0
    return x, torch.randint(0, n_cls, (B, 1), generator=g), 0.5 + torch.rand(n_cls, generator=g)


def onehot_inputs(torch):
    """(logits [2, 6, 9], one-hot target [2, 6, 9], mask [2, 8, 1] of the shifted loss, its lengths)"""
    x, onehot, _, _ = strided_inputs(torch, 2, 6, 9, seed=9)
    lens = torch.tensor([8, 5], dtype=torch.int64)
    mask = (torch.arange(8)[None, :] < lens[:, None]).float().unsqueeze(-1)
    return x, onehot, mask, lens


# ---- the trainer case (reference ClassificationTrainer on the trainer fixture data: questions -> one of 3 classes) ------
TRAINER_CLASSES = 3


def trainer_table(ids):
    """the fixed table id -> class of the trainer case, by the id's position in the fixture's id list"""
    return {i: (3 * n + n // 4) % TRAINER_CLASSES for n, i in enumerate(ids)}


def trainer_hparams(hp, out_dir):
    """3 epochs, seed 1234, batch_first (the settings of the other trainer parities)"""
    hp.out_dir = out_dir
    hp.model_name = "test_classifier"
    hp.seed = 1234
    hp.epochs = 3
    hp.batch_first = True
    hp.batch_size_train = 2
    hp.batch_size_val = 50
    hp.optimiser_args["lr"] = 0.002
    hp.epochs_per_checkpoint = 1
    hp.val_set_perc = 0.3
    hp.use_best_as_final_model = False
    hp.num_classes = TRAINER_CLASSES
    hp.scheduler_type = "Plateau"
    return hp


def trainer_model_config(rnn_dyn, NamedForwardWrapper):
    LC = rnn_dyn.Config.LayerConfig
    return NamedForwardWrapper.Config(
        wrapped_model_config=rnn_dyn.Config(in_dim=409, batch_first=True, layer_configs=[
            LC("GRU", out_dim=8), LC("PoolLast", batch_first=True), LC("Linear", out_dim=TRAINER_CLASSES)]),
        input_names=["questions"], batch_first=True, name="Classifier", output_names=["class_pred"])


def trainer_loss_config(NamedLoss):
    return NamedLoss.Config(name="ce", type_="CrossEntropyLoss", seq_mask=None,
                            input_names=["class_pred", "class_true"], batch_first=True, squeeze_inputs=True)
