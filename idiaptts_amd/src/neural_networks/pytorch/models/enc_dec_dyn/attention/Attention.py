"""Base class of the attention mechanisms of a DecoderModule (the reference's enc_dec_dyn/attention/Attention.py)."""
from torch import nn


class Attention(nn.Module):

    def allows_batched_forward(self):
        """whether the attention of a whole sequence can be computed at once, not frame by frame"""
        raise NotImplementedError()

    def get_go_frame(self):
        """the attention state in front of the first frame (anything; handed through the forward calls)"""
        raise NotImplementedError()

    def forward_batched(self, encoder_input, attention_state):
        """-> (attention_context, attention_matrix) of the whole sequence"""
        raise NotImplementedError()

    def forward_incremental(self, current_frame_idx, encoder_input, decoder_input, attention_state):
        """-> (attention_context, attention_weights, attention_state) of the step that starts at current_frame_idx"""
        raise NotImplementedError()
