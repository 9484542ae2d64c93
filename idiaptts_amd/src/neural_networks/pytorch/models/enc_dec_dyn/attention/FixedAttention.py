"""Attention taken from the ground-truth durations (the reference's enc_dec_dyn/attention/FixedAttention.py): the
attention matrix [B, T, P] of a batch -- PhonemeDurationLabelGen(load_as_matrix=True), one 1 per frame -- is averaged
over chunks of n_frames_per_step frames and multiplied with the encoder output [B, P, C].  Both run in one launch of
csrc/fixed_attention.hip, which walks each row's non-zeros; the gradient flows into the encoder output only.

Deviations from the reference, all at its edges:
  * `forward_incremental` on a slice that reaches past the last frame takes the mean over the frames it has (as the
    reference's slice does); on an EMPTY slice (idx >= T) the reference returns NaN weights and context -- here that
    is an IndexError.
  * a weight of exactly zero skips its encoder row, so Inf / NaN in an encoder row nobody attends to does not reach
    the context (a dense bmm gives NaN there).
  * `forward_batched` with T not a multiple of n_frames_per_step raises a ValueError naming both (the reference's
    `view` raises a RuntimeError about shapes)."""
from idiaptts_amd.nn.functional import fixed_attention

from .Attention import Attention


class FixedAttention(Attention):

    class Config:
        def __init__(self, ground_truth_feature_name, n_frames_per_step):
            self.ground_truth_feature_name = ground_truth_feature_name
            self.n_frames_per_step = n_frames_per_step

        def create_model(self):
            return FixedAttention(self)

    def __init__(self, config):
        super().__init__()
        self.attention_ground_truth = config.ground_truth_feature_name
        self.n_frames_per_step = config.n_frames_per_step

    def allows_batched_forward(self):
        return True

    def forward_batched(self, encoder_input, attention_matrix):
        return fixed_attention(attention_matrix, encoder_input, self.n_frames_per_step, partial_last=False)

    def forward_all_steps(self, encoder_input, attention_matrix):
        """(contexts [B, ceil(T / n), C], weights [B, ceil(T / n), P]) of every step of the iterative pass in one
        launch: the fixed context does not depend on the decoder's state."""
        return fixed_attention(attention_matrix, encoder_input, self.n_frames_per_step, partial_last=True)

    def forward_incremental(self, idx, encoder_input, decoder_input, attention_matrix):
        if not 0 <= idx < attention_matrix.shape[1]:
            raise IndexError("FixedAttention.forward_incremental: frame {} lies outside the {} frames of the attention "
                             "matrix".format(idx, attention_matrix.shape[1]))
        context, weights = fixed_attention(attention_matrix[:, idx:idx + self.n_frames_per_step], encoder_input,
                                           self.n_frames_per_step, partial_last=True)
        return context, weights, attention_matrix

    def extra_repr(self):
        return "ground_truth={}, n_frames_per_step={}".format(self.attention_ground_truth, self.n_frames_per_step)
