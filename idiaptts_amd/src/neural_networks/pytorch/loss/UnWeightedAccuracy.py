"""UnWeightedAccuracy with the reference's interface (loss/UnWeightedAccuracy.py): minus (weighted accuracy +
unweighted accuracy) of a batch as a one-element tensor, for use as a validation "loss".  The divisors are those
given at construction -- `num_total = num_per_class.sum()` and `num_per_class` with zeros replaced by 1 -- not the
batch's (reference :13-17, :25-28), reproduced literally.  It carries no gradient.

On the GPU the arg-max, the number of correct rows and the confusion matrix come from one launch of
itts_class_counts (csrc/xent.hip); CPU tensors go through torch.  The reference's scikit-learn confusion_matrix is
restated: entry [i, j] counts the rows of true class i predicted as j, labels 0 .. num_classes - 1."""
import torch

from idiaptts_amd import ops


class UnWeightedAccuracy(torch.nn.modules.loss._Loss):

    def __init__(self, num_per_class, reduction='none'):
        super().__init__()
        num_per_class = torch.as_tensor(num_per_class).clone()
        self._num_classes = len(num_per_class)
        self._num_total = num_per_class.sum().float()
        num_per_class[num_per_class == 0] = 1.0  # Prevent NaNs.
        self._num_per_class = num_per_class

    def counts(self, input_, target):
        """(correct [1] int64, diagonal of the confusion matrix [num_classes] int64) of a batch"""
        C = self._num_classes
        x = input_.detach().reshape(-1, input_.shape[-1])
        t = target.detach().reshape(-1).to(torch.int64)
        if x.shape[-1] != C:
            raise ValueError("UnWeightedAccuracy for {} classes got predictions of width {}.".format(C, x.shape[-1]))
        if x.is_cuda:
            x = x.float()
            if x.stride(-1) != 1:
                x = x.contiguous()
            _, correct, conf = ops.class_counts(x, t, want_pred=False)
            return correct, conf.diagonal()
        pred = x.argmax(dim=-1)
        hit = pred == t
        inside = (t >= 0) & (t < C)
        return hit.sum().reshape(1), torch.bincount(t[hit & inside], minlength=C)

    def forward(self, input_, target):
        correct, diag = self.counts(input_, target)
        dev = input_.device
        weighted_acc = correct.reshape(()) / self._num_total.to(dev)
        # (numpy's float64 sum over the normalised diagonal, then float32: reference :28-29)
        unweighted_acc = (diag.double() / self._num_per_class.to(dev).double()).sum() / self._num_classes
        return -(weighted_acc + unweighted_acc.float().reshape(1))
