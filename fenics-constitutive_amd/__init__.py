"""MI355X-native quadrature-point constitutive-update engine (see ``_api.py``); import as ``fenics_constitutive_amd``."""

from ._api import *  # noqa: F401,F403
from ._api import __all__ as _api_all
from ._api import __version__  # noqa: F401
from .bicgstab import BiCGStab  # noqa: F401
from .multilevel import MultilevelPreconditioner  # noqa: F401
from .solver import ConjugateGradient  # noqa: F401
from .tangent_operator import TangentOperator  # noqa: F401

__all__ = [*_api_all, "BiCGStab", "ConjugateGradient", "MultilevelPreconditioner", "TangentOperator"]
