"""OneHotCrossEntropyLoss with the reference's interface (loss/OneHotCrossEntropyLoss.py): cross-entropy of logits
[B, C, T] against a one-hot target [B, C, T], the input's frame t scored against the target's frame t + shift
(input[..., :-shift] against target[..., shift:]), returned as [B, T - shift, 1].

On the GPU one launch of itts_softmax_xent_strided (csrc/xent.hip) takes the one-hot target's arg-max, applies the
shift by offsets and writes the loss and its gradient; CPU tensors go through torch as the reference writes it.
Only reduction 'none' keeps the reference's return shape; the other torch reductions are refused (NamedLoss, the
reference's only caller, constructs it with 'none' and reduces itself)."""
import torch

from idiaptts_amd.nn.functional import SoftmaxXentStridedFunction


class OneHotCrossEntropyLoss(torch.nn.CrossEntropyLoss):

    def __init__(self, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction='none', shift=1):
        if size_average is not None or reduce is not None:
            raise NotImplementedError("OneHotCrossEntropyLoss: the deprecated size_average / reduce arguments are not "
                                      "implemented.")
        if reduction != 'none':
            raise NotImplementedError("OneHotCrossEntropyLoss reduction {!r} is not implemented: it returns the "
                                      "per-frame losses [B, T - shift, 1] (reduction 'none').".format(reduction))
        if shift is not None and (int(shift) != shift or shift < 1):
            raise ValueError("shift = {} must be None or a positive integer.".format(shift))
        self.shift = shift
        super().__init__(weight=weight, ignore_index=ignore_index, reduction='none')

    def _check(self, input, target, need_frames=True):
        if input.dim() != 3 or target.shape != input.shape:
            raise ValueError("OneHotCrossEntropyLoss takes logits and a one-hot target of one shape [B, C, T], got {} "
                             "and {}.".format(tuple(input.shape), tuple(target.shape)))
        shift = self.shift or 0
        if need_frames and shift >= input.shape[2]:
            raise ValueError("shift = {} leaves no frame of T = {}.".format(shift, input.shape[2]))
        return shift

    def frame_losses(self, input, target, row_weight=None, elementwise=True):
        """The kernel call NamedLoss shares: per-frame values [B, T - shift] times `row_weight`, or their sum."""
        shift = self._check(input, target)
        B, _, T = input.shape
        if row_weight is None:
            row_weight = torch.ones(B * (T - shift), dtype=torch.float32, device=input.device)
        weight = self.weight.float() if self.weight is not None else None
        return SoftmaxXentStridedFunction.apply(input, target.detach().float(), row_weight, weight, self.ignore_index,
                                                shift, elementwise)

    def forward(self, input, target):
        self._check(input, target, need_frames=input.is_cuda)     # (on the CPU no frames give an empty loss, as torch)
        if not input.is_cuda:
            _, targets = target.max(dim=1)
            if self.shift is not None:
                input = input[..., :-self.shift]
                targets = targets[..., self.shift:]
            return super().forward(input, targets).unsqueeze(-1)
        return self.frame_losses(input, target).unsqueeze(-1)
