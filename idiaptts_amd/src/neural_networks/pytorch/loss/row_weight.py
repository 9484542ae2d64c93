"""What the loss modules share: the sequence mask and the reduction of the reference's NamedLoss._reduce
(loss/NamedLoss.py:113-131) folded into ONE float32 weight per row of the loss, and the start_step / loss_weight
tail of their forward."""
import torch


def _total(lengths):
    """float(sum(lengths)) -- on a tensor without walking it element by element through Python."""
    return float(lengths.sum()) if torch.is_tensor(lengths) else float(sum(lengths))


PER_LENGTH = ("mean_per_frame", "mean_per_sample")      # the reductions that divide by the utterances' lengths


def effective_reduction(reduction, seq_mask):
    """reference NamedLoss.Config :39-43: without a mask there are no lengths to divide by, and 'mean_per_frame' /
    'mean_per_sample' become 'mean'"""
    return "mean" if seq_mask is None and reduction in PER_LENGTH else reduction


def mask_lengths(reduction, length_dict, seq_mask):
    """the lengths row_weight divides by, looked up only where it does"""
    return length_dict[seq_mask] if reduction in PER_LENGTH else None


def row_weight(w, reduction, lengths, batch_dim, width=1, n_pos=None):
    """The float32 mask w, shaped to the loss's leading extents (ones without a mask), divided by what `reduction`
    divides by -> [w.numel()] contiguous.  `lengths`: the utterances' lengths (read by the two per-length
    reductions only), `batch_dim`: the extent of w that carries the batch, `width`: the feature extent the loss
    averages over, `n_pos`: the positions 'mean' counts (w.numel() unless the loss broadcasts over more)."""
    if reduction == "mean_per_frame":
        w = w / (_total(lengths) * width)
    elif reduction == "mean_per_sample":
        lens = torch.as_tensor(lengths, dtype=torch.float32, device=w.device)
        shape = [1] * w.dim()
        shape[batch_dim] = lens.numel()
        w = w / (lens.reshape(shape) * (lens.numel() * width))
    elif reduction == "mean":
        w = w / float((w.numel() if n_pos is None else n_pos) * width)
    return w.reshape(-1).contiguous()


def weighted_output(data, name, loss, step, start_step, loss_weight, then=None):
    """{name: loss * (0 before start_step, else loss_weight)}, passed through `then` and written into data as well.
    (x * 1.0 is x: the launch and its twin in backward are left out on the usual path)"""
    weight = 0. if step < start_step else loss_weight
    loss = loss if weight == 1.0 else loss * weight
    out = {name: loss if then is None else then(loss)}
    data.update(out)
    return out
