from .Config import Config  # noqa: F401
from .EncDecDyn import EncDecDyn, SubModule  # noqa: F401
