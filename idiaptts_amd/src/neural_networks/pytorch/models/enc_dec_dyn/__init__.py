# (the constants stand in front of the imports that read them, as in the reference)
FIXED_ATTENTION = "FixedAttention"
ATTENTION_GROUND_TRUTH = "ground_truth_durations"

from .Config import Config  # noqa: E402,F401
from .EncDecDyn import EncDecDyn, SubModule  # noqa: E402,F401
from .DecoderModule import DecoderModule  # noqa: E402,F401
from .attention.FixedAttention import FixedAttention  # noqa: E402,F401
