"""Importable name of the package directory ``fenics-constitutive_amd/``.

The product lives in ``fenics-constitutive_amd/`` (the name the build contract asks for); a hyphen cannot appear in a
Python import, so this package has no modules of its own: its ``__path__`` is that directory, and every submodule
(``fenics_constitutive_amd.models``, ``._capi``, ...) is the file there -- an ordinary import, visible to coverage, type
checkers and ``importlib.reload``.
"""

import os as _os

__path__ = [_os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "fenics-constitutive_amd")]

from ._api import *  # noqa: E402,F401,F403
from ._api import __all__ as _api_all  # noqa: E402
from ._api import __version__  # noqa: E402,F401
from .bicgstab import BiCGStab  # noqa: E402,F401
from .bicgstab_free import MatrixFreeBiCGStab  # noqa: E402,F401
from .multilevel import MultilevelPreconditioner  # noqa: E402,F401
from .solver import ConjugateGradient  # noqa: E402,F401
from .tangent_operator import TangentOperator  # noqa: E402,F401

__all__ = [*_api_all, "BiCGStab", "ConjugateGradient", "MatrixFreeBiCGStab", "MultilevelPreconditioner", "TangentOperator"]
