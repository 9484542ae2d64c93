"""VAEKLDLoss with the reference's interface (loss/VAEKLDLoss.py): the KL divergence of N(mu, exp(log_var)) to
the standard normal, summed over the latent axis with keepdim (loss_fn, :56-58), masked and reduced as
NamedLoss does (loss/NamedLoss.py:93-131), weighted by start_step / loss_weight and annealed (_anneal, :60-68).

Loss and both gradients come from one launch of itts_vae_kld (csrc/latent.hip).  As for the other element-wise
losses the sequence mask and the reduction are folded into one weight per (batch, time) position; the "feature"
width after loss_fn is 1, so 'mean_per_frame' is sum / frames.  When the mask has a time extent and the inputs have
one frame per utterance (a pooled embedding with a frame-level mask) the reference's `seq_mask * v` broadcasts the
utterance's KL over the mask's frames: the utterance's weight is the sum of its mask over time.
Data-parallel rescaling of `annealing_points` is not done (a TODO in the reference as well)."""
import torch
from torch import nn

from idiaptts_amd.nn.functional import VAEKLDFunction

from .row_weight import effective_reduction, mask_lengths, row_weight, weighted_output


class VAEKLDLoss(nn.Module):

    class Config:
        def __init__(self, name, input_names, annealing_steps=200, annealing_points=(25000, 150000),
                     batch_first=True, input_merge_type="list", seq_mask=None, start_step=0,
                     reduction='mean_per_frame', loss_weight=1.0, **kwargs):
            kwargs.pop("type_", None)
            self.name = name
            self.type = "VAEKLDLoss"
            self.input_names = input_names
            self.seq_mask = seq_mask
            self.batch_first = batch_first
            self.input_merge_type = input_merge_type
            self.reduction = effective_reduction(reduction, seq_mask)
            self.loss_weight = loss_weight
            self.start_step = start_step
            self.kwargs = kwargs
            if annealing_steps < 0:
                raise ValueError("annealing_steps = {} is negative.".format(annealing_steps))
            if annealing_points[0] > annealing_points[1]:
                raise ValueError("annealing_points = {} do not ascend.".format(tuple(annealing_points)))
            self.annealing_steps = annealing_steps
            self.annealing_points = annealing_points

        def create_loss(self):
            return VAEKLDLoss(self)

    REDUCTIONS = ("mean_per_frame", "mean_per_sample", "mean", "sum", "none")

    def __init__(self, config):
        super().__init__()
        if config.reduction not in self.REDUCTIONS:
            raise NotImplementedError("Unknown reduction type {}.".format(config.reduction))
        if len(config.input_names) != 2:
            raise ValueError("VAEKLDLoss takes input_names = [mu, log_var], got {}.".format(config.input_names))
        self.name = config.name
        self.input_names = config.input_names
        self.seq_mask = config.seq_mask
        self.batch_first = config.batch_first
        self.reduction = config.reduction
        self.loss_weight = config.loss_weight
        self.start_step = config.start_step
        self._annealing_steps = config.annealing_steps
        self._annealing_points = config.annealing_points

    def _row_weight(self, mu, mask, length_dict):
        """(one weight per position of mu, number of positions the reference's masked tensor has)"""
        time_dim = 1 if self.batch_first else 0
        lead = tuple(mu.shape[:-1])
        T = lead[time_dim]
        n_pos = lead[0] * lead[1]
        if mask is None:
            w = torch.ones(lead, dtype=torch.float32, device=mu.device)
        else:
            mask = mask.to(torch.float32)
            if mask.dim() < 3:
                mask = mask.unsqueeze(time_dim)
            Tm = mask.shape[time_dim]
            if Tm == T:
                w = mask.reshape(lead)
            elif T == 1:                    # one KL per utterance under a frame mask: broadcast over its frames
                w = mask.sum(dim=time_dim, keepdim=True).reshape(lead)
                n_pos = lead[1 - time_dim] * Tm
            elif Tm == 1:
                w = mask.expand(*lead, 1).reshape(lead)
            else:
                raise ValueError("Sequence mask {} of {} frames cannot be applied to {} of {} frames."
                                 .format(self.seq_mask, Tm, self.input_names, T))
        return row_weight(w, self.reduction, mask_lengths(self.reduction, length_dict, self.seq_mask), 1 - time_dim,
                          n_pos=n_pos)

    def forward(self, data, length_dict, step):
        mu, log_var = (data[n] for n in self.input_names)
        time_dim = 1 if self.batch_first else 0
        if mu.dim() < 3:
            mu, log_var = mu.unsqueeze(time_dim), log_var.unsqueeze(time_dim)
        if mu.shape != log_var.shape:
            raise ValueError("{} {} and {} {} differ in shape.".format(self.input_names[0], tuple(mu.shape),
                                                                      self.input_names[1], tuple(log_var.shape)))
        mask = data[self.seq_mask] if self.seq_mask is not None else None
        if self.reduction == "none" and mask is not None and mask.dim() == 3 \
                and mask.shape[time_dim] != mu.shape[time_dim]:
            ones = torch.ones(mu.shape[:-1].numel(), dtype=torch.float32, device=mu.device)
            loss = VAEKLDFunction.apply(mu, log_var, ones, True) * mask       # the reference's broadcast, as it is
        else:
            w = self._row_weight(mu, mask, length_dict)
            loss = VAEKLDFunction.apply(mu, log_var, w, self.reduction == "none")
        return weighted_output(data, self.name, loss, step, self.start_step, self.loss_weight,
                               then=lambda weighted: self._anneal(weighted, step))

    def annealing_factor(self, step):
        """reference _anneal (:60-67), literally: non-zero only on a multiple of annealing_steps past the first
        point, linear between the points, 1 beyond the second"""
        if step % self._annealing_steps == 0 and step > self._annealing_points[0]:
            if step > self._annealing_points[1]:
                return 1.0
            return (step - self._annealing_points[0]) / (self._annealing_points[1] - self._annealing_points[0])
        return 0.0

    def _anneal(self, loss, step):
        return loss * self.annealing_factor(step)
