"""Reference module path of the all-pass warping module (layers/AllPassWarp.py); see idiaptts_amd.nn.AllPassWarp."""
from idiaptts_amd.nn.modules import AllPassWarp  # noqa: F401
