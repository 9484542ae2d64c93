"""loss/row_weight.py alone: the one weight per row into which the loss modules fold their sequence mask and their
reduction, against numbers written by hand (every length, count and width a power of two: each quotient is exact in
float32 and torch.equal applies), and -- through each of the three methods that call it -- against the reductions'
definitions evaluated in float64.  Nothing here needs a GPU."""
import pytest
import torch

from idiaptts_amd.src.neural_networks.pytorch.loss.NamedLoss import NamedLoss
from idiaptts_amd.src.neural_networks.pytorch.loss.VAEKLDLoss import VAEKLDLoss
from idiaptts_amd.src.neural_networks.pytorch.loss.row_weight import effective_reduction, row_weight

LENGTHS = [1, 1, 2, 4]                    # 4 utterances, 8 frames, padded to T = 4: 16 positions
MASK = torch.tensor([[1., 0, 0, 0],
                     [1., 0, 0, 0],
                     [1., 1, 0, 0],
                     [1., 1, 1, 1]])        # [B, T]
PER_SAMPLE = torch.tensor([[1 / 4], [1 / 4], [1 / 8], [1 / 16]])      # 1 / (len_b * 4 utterances)

# (reduction, width, n_pos) -> the weights [B, T], by hand
HAND = [
    ("mean_per_frame", 1, None, MASK / 8),                  # / 8 frames
    ("mean_per_frame", 4, None, MASK / 32),                 # / (8 frames * 4 features)
    ("mean_per_sample", 1, None, MASK * PER_SAMPLE),
    ("mean_per_sample", 4, None, MASK * PER_SAMPLE / 4),
    ("mean", 1, None, MASK / 16),                           # / 16 positions, padding included
    ("mean", 4, None, MASK / 64),
    ("mean", 1, 32, MASK / 32),                             # the positions given: a loss that broadcasts over more
    ("mean", 4, 32, MASK / 128),
    ("sum", 1, None, MASK),
    ("sum", 4, None, MASK),
    ("none", 1, None, MASK),
    ("none", 4, 32, MASK),
]


@pytest.mark.parametrize("lengths", [LENGTHS, torch.tensor(LENGTHS)], ids=["list", "tensor"])
@pytest.mark.parametrize("batch_dim", [0, 1])
@pytest.mark.parametrize("reduction,width,n_pos,want", HAND,
                         ids=["{}-w{}-n{}".format(r, w, n) for r, w, n, _ in HAND])
def test_row_weight_by_hand(reduction, width, n_pos, want, batch_dim, lengths):
    w = MASK if batch_dim == 0 else MASK.t()
    want = want if batch_dim == 0 else want.t()
    got = row_weight(w.clone(), reduction, lengths, batch_dim, width=width, n_pos=n_pos)
    assert got.dtype == torch.float32 and got.dim() == 1 and got.is_contiguous()
    assert torch.equal(got, want.reshape(-1))


def test_row_weight_defaults_are_width_one_and_all_positions():
    assert torch.equal(row_weight(MASK, "mean", None, 0), MASK.reshape(-1) / 16)
    assert torch.equal(row_weight(MASK, "mean_per_frame", LENGTHS, 0), MASK.reshape(-1) / 8)


@pytest.mark.parametrize("reduction,want", [("mean", 1 / 16), ("sum", 1.), ("none", 1.), ("mean_per_frame", 1 / 8)])
def test_row_weight_of_a_mask_of_ones(reduction, want):
    """no mask: the callers pass ones; the lengths are read by the per-length reductions only"""
    lengths = LENGTHS if reduction == "mean_per_frame" else None
    got = row_weight(torch.ones(4, 4), reduction, lengths, 0)
    assert torch.equal(got, torch.full((16,), want))


def test_row_weight_leaves_its_mask_alone_and_takes_one_dimension():
    mask = MASK.clone()
    row_weight(mask, "mean", None, 0)
    assert torch.equal(mask, MASK)
    # a [N] loss (utterance classification): the batch is the only extent
    got = row_weight(torch.tensor([1., 0, 1, 1]), "mean_per_sample", [1, 1, 2, 4], 0)
    assert torch.equal(got, torch.tensor([1 / 4, 0, 1 / 8, 1 / 16]))


def test_effective_reduction():
    assert effective_reduction("mean_per_frame", None) == "mean"
    assert effective_reduction("mean_per_sample", None) == "mean"
    for reduction in ("mean_per_frame", "mean_per_sample", "mean", "sum", "none"):
        assert effective_reduction(reduction, "mask") == reduction
    for reduction in ("mean", "sum", "none"):
        assert effective_reduction(reduction, None) == reduction


@pytest.mark.parametrize("reduction", ["mean_per_frame", "mean_per_sample"])
def test_the_three_fallbacks_to_mean(reduction):
    """NamedLoss.Config (classification types), NamedLoss.__init__ (a Config edited after its construction) and
    VAEKLDLoss.Config; the element-wise types keep their refusal"""
    assert NamedLoss.Config("l", "CrossEntropyLoss", ["p", "t"], reduction=reduction).reduction == "mean"
    config = NamedLoss.Config("l", "CrossEntropyLoss", ["p", "t"], seq_mask="m", reduction=reduction)
    assert config.reduction == reduction
    config.seq_mask = None
    assert NamedLoss(config).reduction == "mean"
    assert VAEKLDLoss.Config("kl", ["mu", "lv"], reduction=reduction).reduction == "mean"
    assert VAEKLDLoss.Config("kl", ["mu", "lv"], seq_mask="m", reduction=reduction).reduction == reduction
    config = NamedLoss.Config("l", "MSELoss", ["a", "b"], reduction=reduction)
    assert config.reduction == reduction
    with pytest.raises(ValueError, match="needs a seq_mask"):
        NamedLoss(config)


# ---- through the three calling methods: sum_r w[r] sum_c e[r, c] against the reduction's definition in float64 ----
# The weights are float32 quotients (relative error 2^-24 = 6e-8 each, one or two roundings), e is positive so that
# nothing cancels in either sum: the two agree to a few 1e-7 relative, and 1e-6 is asked.
B, T = 3, 5
LENS = [3, 5, 2]


def _frame_mask():
    return (torch.arange(T)[None, :] < torch.tensor(LENS)[:, None]).to(torch.float32)       # [B, T]


def _definition(reduction, e, mask):
    """e [B, T, D] float64, mask [B, T]"""
    D = e.shape[-1]
    masked = e * mask.double()[..., None]
    if reduction == "mean_per_frame":
        return masked.sum() / (sum(LENS) * D)
    if reduction == "mean_per_sample":
        per_utt = masked.sum(dim=(1, 2)) / (torch.tensor(LENS, dtype=torch.float64) * D)
        return per_utt.mean()
    return masked.sum() / (B * T * D)


def _weights(method, reduction, D, batch_first):
    mask = _frame_mask().unsqueeze(-1)                          # [B, T, 1]
    if not batch_first:
        mask = mask.transpose(0, 1).contiguous()
    lens = {"m": torch.tensor(LENS)}
    if method == "NamedLoss._row_weight":
        loss = NamedLoss.Config("l", "L1Loss", ["a", "b"], seq_mask="m", batch_first=batch_first,
                                reduction=reduction).create_loss()
        a = torch.zeros(mask.shape[:2] + (D,))
        return loss._row_weight(a, mask, lens)
    if method == "NamedLoss._class_row_weight":
        loss = NamedLoss.Config("l", "OneHotCrossEntropyLoss", ["p", "t"], seq_mask="m", batch_first=batch_first,
                                reduction=reduction).create_loss()
        return loss._class_row_weight((B, T), mask if batch_first else mask[..., 0], lens, torch.device("cpu"))
    loss = VAEKLDLoss.Config("kl", ["mu", "lv"], seq_mask="m", batch_first=batch_first,
                             reduction=reduction).create_loss()
    return loss._row_weight(torch.zeros(mask.shape[:2] + (7,)), mask, lens)


@pytest.mark.parametrize("batch_first", [True, False], ids=["batch_first", "time_major"])
@pytest.mark.parametrize("reduction", ["mean_per_frame", "mean_per_sample", "mean"])
@pytest.mark.parametrize("method,D", [("NamedLoss._row_weight", 3), ("NamedLoss._class_row_weight", 1),
                                      ("VAEKLDLoss._row_weight", 1)])
def test_calling_methods_against_the_definitions(method, D, reduction, batch_first):
    torch.manual_seed(5)
    e = torch.rand(B, T, D, dtype=torch.float64) + 0.5          # an element-wise loss, [B, T, D] whatever the layout
    w = _weights(method, reduction, D, batch_first)
    # the class losses are [B, T'] in both layouts; the others follow batch_first
    rows_batch_first = batch_first or method == "NamedLoss._class_row_weight"
    w = w.reshape(B, T) if rows_batch_first else w.reshape(T, B).t()
    got = (w.double()[..., None] * e).sum()
    want = _definition(reduction, e, _frame_mask())
    assert abs(got - want) <= 1e-6 * abs(want), (float(got), float(want))
