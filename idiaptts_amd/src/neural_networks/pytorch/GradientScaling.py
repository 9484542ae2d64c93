"""Reference module path of the gradient-scaling layer (GradientScaling.py): identity forward, gradient times a
constant.  The implementation lives with the other autograd functions and modules in idiaptts_amd.nn."""
from idiaptts_amd.nn.functional import grad_scaling  # noqa: F401
from idiaptts_amd.nn.modules import GradientScaling  # noqa: F401
