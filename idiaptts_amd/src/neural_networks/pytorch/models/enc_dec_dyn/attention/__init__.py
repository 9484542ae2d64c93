from .Attention import Attention  # noqa: F401
from .FixedAttention import FixedAttention  # noqa: F401
