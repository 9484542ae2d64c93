"""NamedLoss with the reference's interface (loss/NamedLoss.py:16-131).  The loss on the hot path --
MSELoss(reduction='none') * seq_mask, reduced 'mean_per_frame' (sum over batch and time / total
frames, mean over features) -- is one fused HIP kernel producing the loss and its gradient.  The
other element-wise types (MSELoss, L1Loss) and reductions ('mean_per_sample', 'mean', 'sum',
'none', with or without a sequence mask; reference :113-131) run a second kernel in which the mask
and the reduction are folded into one weight per frame.

The classification types -- "CrossEntropyLoss" (torch's, on [N, C] logits and int64 targets, usually behind
squeeze_inputs), "OneHotCrossEntropyLoss" ([B, C, T] logits against a one-hot target) and "UnWeightedAccuracy" (a
score without gradient) -- run on csrc/xent.hip: softmax, loss and gradient from one launch, the mask and the
reduction again one weight per row.  Their keyword arguments are torch's `weight` and `ignore_index` (plus `shift` /
`num_per_class` of the reference's two classes); a non-zero `label_smoothing` and anything else is refused by name.
"DiscretizedMixturelogisticLoss" ([B, 3K, T] mixture parameters against samples [B, 1, T]; keywords `num_classes`,
`log_scale_min`, `shift`, `hinge_loss`) runs on csrc/mol.hip in the same way.
CPU tensors of these types go through torch."""
import torch
from torch import nn

from idiaptts_amd.nn.functional import MaskedMSEFunction, SoftmaxXentFunction, WeightedLossFunction

from .DiscretizedMixturelogisticLoss import DiscretizedMixturelogisticLoss
from .OneHotCrossEntropyLoss import OneHotCrossEntropyLoss
from .row_weight import _total, effective_reduction, mask_lengths, row_weight, weighted_output
from .UnWeightedAccuracy import UnWeightedAccuracy


class NamedLoss(nn.Module):

    class Config:
        def __init__(self, name, type_, input_names, seq_mask=None, batch_first=False,
                     reduction='mean_per_frame', loss_weight=1.0, start_step=0, squeeze_inputs=False, **kwargs):
            self.name = name
            self.type = type_
            self.input_names = input_names
            self.seq_mask = seq_mask
            self.batch_first = batch_first
            self.squeeze_inputs = squeeze_inputs         # used for classification (reference NamedLoss.py:26)
            # reference NamedLoss.Config :39-43, for the classification types: nothing to divide by without a mask
            self.reduction = effective_reduction(reduction, seq_mask) if type_ in NamedLoss.CLASS_TYPES else reduction
            self.loss_weight = loss_weight
            self.start_step = start_step
            self.kwargs = kwargs

        def create_loss(self):
            return NamedLoss(self)

    KINDS = {"MSELoss": 0, "L1Loss": 1}
    CLASS_TYPES = ("CrossEntropyLoss", "OneHotCrossEntropyLoss", "UnWeightedAccuracy",
                   "DiscretizedMixturelogisticLoss")
    CLASS_KWARGS = {"CrossEntropyLoss": ("weight", "ignore_index", "label_smoothing"),
                    "OneHotCrossEntropyLoss": ("weight", "ignore_index", "label_smoothing", "shift"),
                    "UnWeightedAccuracy": ("num_per_class",),
                    "DiscretizedMixturelogisticLoss": ("num_classes", "log_scale_min", "shift", "hinge_loss")}
    REDUCTIONS = ("mean_per_frame", "mean_per_sample", "mean", "sum", "none")

    def __init__(self, config):
        super().__init__()
        if config.type not in self.KINDS and config.type not in self.CLASS_TYPES:
            raise NotImplementedError("Loss type {} has no kernel here (element-wise MSELoss and L1Loss, "
                                      "CrossEntropyLoss, OneHotCrossEntropyLoss, UnWeightedAccuracy and "
                                      "DiscretizedMixturelogisticLoss do)."
                                      .format(config.type))
        if config.reduction not in self.REDUCTIONS:
            raise NotImplementedError("Unknown reduction type {}.".format(config.reduction))
        reduction = effective_reduction(config.reduction, config.seq_mask)  # (a Config edited after its construction)
        if reduction != config.reduction and config.type not in self.CLASS_TYPES:
            raise ValueError("Reduction '{}' divides by the sequence lengths: it needs a seq_mask "
                             "(reference NamedLoss.py:114-121).".format(config.reduction))
        self.kind = self.KINDS.get(config.type)
        self.type = config.type
        self.squeeze_inputs = getattr(config, "squeeze_inputs", False)
        if config.type in self.CLASS_TYPES:
            self._init_classification(config)
        self.reduction = reduction
        self.name = config.name
        self.input_names = config.input_names
        self.seq_mask = config.seq_mask
        self.batch_first = config.batch_first
        self.loss_weight = config.loss_weight
        self.start_step = config.start_step

    def _row_weight(self, a, mask, length_dict):
        """One weight per (time, batch) position: sequence mask x what the reduction divides by."""
        lead = tuple(a.shape[:-1])                            # [T, B] or [B, T]
        if mask is not None:
            w = mask.reshape(lead).to(torch.float32)
        else:
            w = torch.ones(lead, dtype=torch.float32, device=a.device)
        return row_weight(w, self.reduction, mask_lengths(self.reduction, length_dict, self.seq_mask),
                          0 if self.batch_first else 1, width=a.shape[-1])

    def _init_classification(self, config):
        kwargs = dict(getattr(config, "kwargs", None) or {})
        for key in kwargs:
            if key not in self.CLASS_KWARGS[config.type]:
                raise NotImplementedError("{} keyword {!r} is not implemented (it takes {})."
                                          .format(config.type, key, ", ".join(self.CLASS_KWARGS[config.type])))
        if kwargs.get("label_smoothing", 0.0) != 0.0:
            raise NotImplementedError("{} keyword label_smoothing = {} is not implemented."
                                      .format(config.type, kwargs["label_smoothing"]))
        if len(config.input_names) != 2:
            raise ValueError("{} takes input_names = [prediction, target], got {}."
                             .format(config.type, config.input_names))
        if config.type == "DiscretizedMixturelogisticLoss":
            for key in ("num_classes", "log_scale_min"):
                if key not in kwargs:
                    raise ValueError("DiscretizedMixturelogisticLoss needs {}.".format(key))
            self.loss_fn = DiscretizedMixturelogisticLoss(kwargs["num_classes"], kwargs["log_scale_min"],
                                                          shift=kwargs.get("shift", 1),
                                                          hinge_loss=kwargs.get("hinge_loss", True))
            return
        if config.type == "UnWeightedAccuracy":
            if "num_per_class" not in kwargs:
                raise ValueError("UnWeightedAccuracy needs num_per_class.")
            if config.seq_mask is not None:
                raise ValueError("UnWeightedAccuracy is one score per batch: it takes no seq_mask ({})."
                                 .format(config.seq_mask))
            self.loss_fn = UnWeightedAccuracy(kwargs["num_per_class"])
            return
        weight = kwargs.get("weight")
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32)
        self.ignore_index = int(kwargs.get("ignore_index", -100))
        if config.type == "OneHotCrossEntropyLoss":
            self.loss_fn = OneHotCrossEntropyLoss(weight=weight, ignore_index=self.ignore_index,
                                                  shift=kwargs.get("shift", 1))
        else:
            self.register_buffer("class_weight", weight)

    def _squeeze(self, inputs):
        """reference NamedLoss.py:77-86: squeeze every input, put the batch extent back when it was 1"""
        batch_dim = 0 if self.batch_first else 1
        batch_size = inputs[0].shape[batch_dim]
        inputs = [input_.squeeze() for input_ in inputs]
        if batch_size == 1:
            # (the squeezed [C] / [] have lost time and batch alike: the batch extent of [B, C] / [B] leads.  The
            # reference unsqueezes at batch_dim, which is the same for batch_first and fails time-major)
            inputs = [input_.unsqueeze(0) for input_ in inputs]
        return inputs

    def _class_row_weight(self, lead, mask, length_dict, device):
        """One weight per position of a [B] or [B, T'] loss: the mask times what the reduction divides by
        (reference _reduce, :113-131, on a loss whose feature extent is 1)."""
        n_pos = 1
        for n in lead:
            n_pos *= int(n)
        if mask is None:
            w = torch.ones(lead, dtype=torch.float32, device=device)
        else:
            mask = mask.to(torch.float32)
            if len(lead) == 2:
                if mask.dim() == 3:
                    mask = mask[..., 0]
                if mask.dim() != 2:
                    raise ValueError("Sequence mask {} {} is no [batch, time(, 1)] mask."
                                     .format(self.seq_mask, tuple(mask.shape)))
                if not self.batch_first:
                    mask = mask.t()
                if mask.shape[1] != lead[1] or mask.shape[0] != lead[0]:
                    raise ValueError("Sequence mask {} of {} x {} frames cannot be applied to the loss {} of {} x {} "
                                     "frames.".format(self.seq_mask, mask.shape[0], mask.shape[1], self.name,
                                                      lead[0], lead[1]))
                w = mask
            else:
                if mask.numel() != n_pos:
                    raise ValueError("Sequence mask {} of {} frames cannot be applied to the loss {} of {} x 1 frames."
                                     .format(self.seq_mask, "x".join(str(n) for n in mask.shape), self.name, lead[0]))
                w = mask.reshape(lead)
        return row_weight(w, self.reduction, mask_lengths(self.reduction, length_dict, self.seq_mask), 0)

    def _forward_classification(self, data, length_dict, step):
        inputs = [data[n] for n in self.input_names]     # (prediction, target), as torch's losses take them
        if self.squeeze_inputs:
            inputs = self._squeeze(inputs)
        pred, target = inputs
        elementwise = self.reduction == "none"
        mask = data[self.seq_mask] if self.seq_mask is not None else None
        if self.type == "UnWeightedAccuracy":
            loss = self.loss_fn(pred, target)
            if not elementwise:
                loss = loss.reshape(())                  # mean / sum of the one element
        elif self.type in ("OneHotCrossEntropyLoss", "DiscretizedMixturelogisticLoss"):
            shift = self.loss_fn._check(pred, target)    # input frame t is scored against target frame t + shift
            B, _, T = pred.shape
            w = self._class_row_weight((B, T - shift), mask, length_dict, pred.device)
            if pred.is_cuda:
                loss = self.loss_fn.frame_losses(pred, target, w, elementwise)
            else:
                loss = self.loss_fn(pred, target)[..., 0] * w.reshape(B, T - shift)
                loss = loss if elementwise else loss.sum()
            if elementwise:
                loss = loss.unsqueeze(-1)
        else:
            if pred.dim() != 2 or target.dim() != 1 or target.shape[0] != pred.shape[0]:
                raise NotImplementedError("CrossEntropyLoss takes logits [N, C] and class indices [N] (use "
                                          "squeeze_inputs for [B, 1, C] / [B, 1]), got {} and {}; frame-level "
                                          "logits [B, C, T] go through OneHotCrossEntropyLoss."
                                          .format(tuple(pred.shape), tuple(target.shape)))
            if target.dtype != torch.int64:
                if target.is_floating_point():
                    raise NotImplementedError("CrossEntropyLoss with probability (floating point) targets is not "
                                              "implemented: the target {} must hold int64 class indices."
                                              .format(self.input_names[1]))
                target = target.to(torch.int64)
            w = self._class_row_weight((pred.shape[0],), mask, length_dict, pred.device)
            if pred.is_cuda:
                loss = SoftmaxXentFunction.apply(pred, target, w, self.class_weight, self.ignore_index, elementwise)
            else:
                loss = torch.nn.functional.cross_entropy(pred, target, weight=self.class_weight,
                                                         ignore_index=self.ignore_index, reduction="none") * w
                loss = loss if elementwise else loss.sum()
        return weighted_output(data, self.name, loss, step, self.start_step, self.loss_weight)

    def forward(self, data, length_dict, step):
        if self.kind is None:
            return self._forward_classification(data, length_dict, step)
        a, b = (data[n] for n in self.input_names)       # (target, prediction)
        if self.squeeze_inputs:
            a, b = self._squeeze([a, b])
        if self.kind == 0 and self.reduction == "mean_per_frame":
            mask = data[self.seq_mask]                   # [.., .., 1] float, 1 inside the sequence
            row_valid = (mask.reshape(-1) > 0).view(torch.uint8)      # (bool and uint8 are both one byte of 0 / 1)
            total_num_frames = _total(length_dict[self.seq_mask])
            # MSE is symmetric: differentiate through whichever input needs it
            if b.requires_grad or not a.requires_grad:
                loss = MaskedMSEFunction.apply(b, a.detach(), row_valid, total_num_frames)
            else:
                loss = MaskedMSEFunction.apply(a, b.detach(), row_valid, total_num_frames)
        else:
            w = self._row_weight(a, data[self.seq_mask] if self.seq_mask is not None else None,
                                 length_dict)
            # both element-wise losses are symmetric in their arguments
            if b.requires_grad or not a.requires_grad:
                loss = WeightedLossFunction.apply(b, a.detach(), w, self.kind,
                                                  self.reduction == "none")
            else:
                loss = WeightedLossFunction.apply(a, b.detach(), w, self.kind,
                                                  self.reduction == "none")
        return weighted_output(data, self.name, loss, step, self.start_step, self.loss_weight)
