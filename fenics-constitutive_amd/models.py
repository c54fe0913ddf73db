"""GPU-backed constitutive laws with the reference's class names, constructor arguments,
``evaluate`` signature, ``history_dim`` and error behaviour.

Each class is a thin host-side mirror: it keeps the material parameters, and ``evaluate``
goes through the C ABI (``include/fcamd.h``) into the HIP kernels -- NumPy arrays via the
staged host path, torch ROCm tensors zero-copy (see ``device.py``).

Reference classes mirrored:
  LinearElasticityModel              models/linear_elasticity_model.py:9-56
  VonMises3D                         models/mises_plasticity_isotropic_hardening.py:9-186
  SpringMaxwellModel                 models/spring_maxwell_model.py:8-102
  SpringKelvinModel                  models/spring_kelvin_model.py:9-102
  LinearElasticity3D                 models/rust_models.py:84-94  (comfe-rs linear_elasticity.rs)
  MisesPlasticityLinearHardening3D   models/rust_models.py:145-161 (comfe-rs mises_plasticity.rs)

Per-point parameters (LinearElasticityModel under FULL, LinearElasticity3D, VonMises3D, MisesPlasticityLinearHardening3D):
any parameter may be a 1-D float64 array (or ROCm tensor) with more than one element -- a field over that many quadrature
points (``field_points``); the other parameters keep their scalar meaning.  See ``device.parameter_field``.
"""

from __future__ import annotations

import numpy as np

from . import _capi
from .device import DeviceLaw, parameter_field
from .interfaces import StressStrainConstraint
from .utils import get_elastic_tangent, get_identity, lame_parameters

__all__ = [
    "DruckerPrager3D",
    "DruckerPragerHyperbolic3D",
    "LinearElasticityModel",
    "VonMises3D",
    "SpringMaxwellModel",
    "SpringKelvinModel",
    "LinearElasticity3D",
    "MisesPlasticityLinearHardening3D",
]


class LinearElasticityModel(DeviceLaw):
    """Linear elasticity: ``sigma += d_eps . D``, ``tangent = D`` at every point.

    Args:
        parameters: ``{"E": Young's modulus, "nu": Poisson ratio}``.
        constraint: stress/strain constraint (device kernels: FULL).
    """

    _model_id = _capi.LINEAR_ELASTICITY
    _supports_fields = True
    _parameter_names = ("E", "nu")

    def __init__(self, parameters: dict[str, float], constraint: StressStrainConstraint):
        E, nu = parameters["E"], parameters["nu"]
        super().__init__([E, nu], constraint)
        if self.field_points is None:
            self.D = get_elastic_tangent(E, nu, constraint)
        else:  # one D per point, built by the kernels; refused where the scalar law refuses (lame_parameters' divisions)
            nu_f = np.asarray(self._fields.get(1, self._parameter_vector[1]), dtype=np.float64)
            if np.any(2.0 * (1.0 + nu_f) == 0.0) or np.any((1.0 + nu_f) * (1.0 - 2.0 * nu_f) == 0.0):
                raise ZeroDivisionError("float division by zero")
            self.D = None

    @property
    def history_dim(self) -> None:
        return None


class VonMises3D(DeviceLaw):
    r"""Von Mises plasticity with nonlinear (saturation) isotropic hardening; per-point scalar
    Newton iteration on the plastic multiplier, algorithmically consistent tangent.

    Args:
        param: ``p_ka`` bulk modulus, ``p_mu`` shear modulus, ``p_y0`` initial yield stress,
            ``p_y00`` saturated yield stress, ``p_w`` saturation parameter.
    """

    _model_id = _capi.VON_MISES_3D
    _supports_fields = True
    _parameter_names = ("p_ka", "p_mu", "p_y0", "p_y00", "p_w")

    def __init__(self, param: dict[str, float]):
        self.p_ka = param["p_ka"]
        self.p_mu = param["p_mu"]
        self.p_y0 = param["p_y0"]
        self.p_y00 = param["p_y00"]
        self.p_w = param["p_w"]
        super().__init__([self.p_ka, self.p_mu, self.p_y0, self.p_y00, self.p_w], StressStrainConstraint.FULL)
        # host mirrors of the reference's public attributes (:33-49)
        self.xioi = np.zeros((6, 6), dtype=np.int64)
        self.xioi[:3, :3] = 1
        self.I2 = get_identity(6, StressStrainConstraint.FULL)
        self.I4 = np.eye(6, dtype=np.float64)
        self.xpp = self.I4 - (1 / 3) * self.xioi

    @property
    def history_dim(self) -> dict[str, int]:
        return {"eps_n": 6, "alpha": 1}


class _SpringBase(DeviceLaw):
    def __init__(self, parameters: dict[str, float], constraint: StressStrainConstraint):
        self.E0 = parameters["E0"]
        self.E1 = parameters["E1"]
        self.tau = parameters["tau"]
        self.nu = 0.0 if constraint.name == "UNIAXIAL_STRESS" else parameters["nu"]
        super().__init__([self.E0, self.E1, self.tau, self.nu], constraint)

    @property
    def history_dim(self) -> dict[str, int]:
        return {"strain_visco": self.stress_strain_dim, "strain": self.stress_strain_dim}

    def evaluate(self, t, del_t, grad_del_u, stress, tangent, history, check: bool = False) -> None:
        if history is None:
            raise ValueError("history must not be None")
        assert del_t > 0, "Time step must be defined and positive."
        super().evaluate(t, del_t, grad_del_u, stress, tangent, history, check=check)


class SpringMaxwellModel(_SpringBase):
    """Standard linear solid, spring parallel to a Maxwell arm, backward Euler.

    Args:
        parameters: ``E0`` elastic modulus, ``E1`` viscous-arm modulus, ``tau`` relaxation
            time, ``nu`` Poisson ratio.
        constraint: stress/strain constraint (device kernels: FULL).
    """

    _model_id = _capi.SPRING_MAXWELL

    def __init__(self, parameters, constraint):
        super().__init__(parameters, constraint)
        self.D_0 = get_elastic_tangent(self.E0, self.nu, constraint)
        self.D_1 = get_elastic_tangent(self.E1, self.nu, constraint)
        self.mu1, _ = lame_parameters(self.E1, self.nu)


class SpringKelvinModel(_SpringBase):
    """Standard linear solid, spring in series with a Kelvin body, backward Euler.

    Args: as :class:`SpringMaxwellModel`.
    """

    _model_id = _capi.SPRING_KELVIN

    def __init__(self, parameters, constraint):
        super().__init__(parameters, constraint)
        self.D_0 = get_elastic_tangent(self.E0, self.nu, constraint)
        self.I2 = get_identity(self.stress_strain_dim, constraint)
        self.mu0, self.lam0 = lame_parameters(self.E0, self.nu)
        self.mu1, _ = lame_parameters(self.E1, self.nu)


def _scalar(parameters: dict, key: str) -> float:
    """Rust-style parameter dicts carry one-element arrays (tests/models/test_plasticity.py:26-31)."""
    try:
        field = parameter_field(key, parameters[key]) is not None
    except (TypeError, ValueError):
        field = False  # not a well-formed field: refused below as before
    if field:
        raise NotImplementedError(f"parameter '{key}': this law takes no per-point parameter fields")
    v = np.asarray(parameters[key], dtype=np.float64).reshape(-1)
    if v.size != 1:
        raise ValueError(f"parameter '{key}' must have exactly one entry")
    return float(v[0])


def _scalar_or_field(parameters: dict, key: str):
    """``_scalar``, or the value itself when it is a per-point field (``device.parameter_field``; the laws with field kernels)"""
    v = parameters[key]
    return v if parameter_field(key, v) is not None else _scalar(parameters, key)


class LinearElasticity3D(DeviceLaw):
    """comfe-rs ``LinearElasticity3D``: ``sigma += C . d_eps`` with ``C = 2 mu P_dev + 3 kappa P_vol``.

    Args:
        parameters: ``{"mu": array([..]), "kappa": array([..])}``.
    """

    _model_id = _capi.COMFE_LINEAR_ELASTICITY
    _supports_fields = True
    _parameter_names = ("mu", "kappa")

    def __init__(self, parameters: dict[str, np.ndarray]):
        super().__init__([_scalar_or_field(parameters, "mu"), _scalar_or_field(parameters, "kappa")], StressStrainConstraint.FULL)

    @property
    def history_dim(self) -> None:
        return None


class MisesPlasticityLinearHardening3D(DeviceLaw):
    """comfe-rs ``MisesPlasticity3D``: von Mises yield function, linear isotropic hardening,
    closed-form radial return.  History ``{"history": 7}`` = ``[alpha, plastic_strain(6)]``.

    Args:
        parameters: ``{"mu", "kappa", "y_0", "h"}`` as one-element arrays.
    """

    _model_id = _capi.COMFE_MISES_PLASTICITY
    _supports_fields = True
    _parameter_names = ("mu", "kappa", "y_0", "h")

    def __init__(self, parameters: dict[str, np.ndarray]):
        super().__init__(
            [_scalar_or_field(parameters, k) for k in self._parameter_names], StressStrainConstraint.FULL
        )

    @property
    def history_dim(self) -> dict[str, int]:
        return {"history": 7}


class DruckerPrager3D(DeviceLaw):
    """comfe-rs classic Drucker-Prager plasticity (``f = sqrt(J2) + b I1 - a``) solved by the general
    return mapping (reference: models/rust_models.py:97-118, comfe-rs/src/plasticity/general.rs,
    drucker_prager_classic.rs).  History ``{"history": 7}`` = ``[alpha, plastic_strain(6)]``.

    Args:
        parameters: ``{"mu", "kappa", "a", "b", "b_flow"}`` as one-element arrays.
    """

    _model_id = _capi.COMFE_DRUCKER_PRAGER

    def __init__(self, parameters: dict[str, np.ndarray]):
        super().__init__([_scalar(parameters, k) for k in ("mu", "kappa", "a", "b", "b_flow")], StressStrainConstraint.FULL)

    @property
    def history_dim(self) -> dict[str, int]:
        return {"history": 7}


class DruckerPragerHyperbolic3D(DeviceLaw):
    """comfe-rs hyperbolically smoothed Drucker-Prager plasticity (``f = sqrt(J2 + d^2) + b I1 - a``),
    reference: models/rust_models.py:121-142, drucker_prager_hyperbolic.rs.

    Args:
        parameters: ``{"mu", "kappa", "a", "b", "d", "b_flow"}`` as one-element arrays.
    """

    _model_id = _capi.COMFE_DRUCKER_PRAGER_HYPERBOLIC

    def __init__(self, parameters: dict[str, np.ndarray]):
        super().__init__([_scalar(parameters, k) for k in ("mu", "kappa", "a", "b", "d", "b_flow")], StressStrainConstraint.FULL)

    @property
    def history_dim(self) -> dict[str, int]:
        return {"history": 7}
