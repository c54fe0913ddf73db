"""Objective stress rates: ``JaumannRate`` wraps a FULL small-strain law so that its committed stress and tensor-valued history
turn with the material between increments (the Jaumann rate, integrated with the Hughes-Winget rotation).

Every call takes the incremental spin ``W = (G - G^T) / 2`` of ``G = grad_del_u``, forms ``R = (I - W / 2)^-1 (I + W / 2)``,
rotates the committed stress and every rotatable history block to ``R S R^T`` and evaluates the law on the rotated state with
the unchanged strain increment -- what an Abaqus host does to STRESS and the tensor state variables before it calls a UMAT.
The math and its device code: ``csrc/jit/rotation.h``.

Two paths:

* fused: the rotation runs in registers inside the law's own kernel, between the transposition of the state and the point
  function (no extra bytes per point).  For ``UserLaw`` (every tangent mode) and, through their ``userlaw_sources``
  transcriptions, ``LinearElasticityModel`` (FULL), ``SpringMaxwellModel`` (FULL) and ``VonMises3D`` with scalar parameters.
* array-level: every other FULL law of the package (``SpringKelvinModel``, the comfe-rs laws, laws with parameter fields).
  A standalone kernel (``csrc/jit/rotate_state.hip``) writes the rotated committed state into the arrays the law then
  evaluates in place.
"""

from __future__ import annotations

import ctypes as C

from . import jit
from .device import _check_torch, _is_torch
from .interfaces import StressStrainConstraint
from .userlaw import UserLaw

__all__ = ["JaumannRate", "default_rotatable"]

ROTATE_KERNEL = "fcamd_rotate_state_kernel"


def default_rotatable(model) -> dict:
    """history name -> offsets of the Mandel 6-vectors that rotate, for the laws the package ships (``{}`` for a UserLaw)"""
    from . import models as M

    if isinstance(model, M.VonMises3D):
        return {"eps_n": [0]}  # alpha is a scalar
    if isinstance(model, (M.SpringMaxwellModel, M.SpringKelvinModel)):
        return {"strain_visco": [0], "strain": [0]}
    if isinstance(model, (M.MisesPlasticityLinearHardening3D, M.DruckerPrager3D, M.DruckerPragerHyperbolic3D)):
        return {"history": [1]}  # [alpha, eps_p(6)]
    return {}


def _history_dims(model) -> list:
    """[(name, doubles per point)] of the law's history, in its order"""
    if isinstance(model, UserLaw):
        return list(model._hist)
    hd = model.history_dim
    return [] if hd is None else [(k, int(v)) for k, v in hd.items()]


def _blocks(model, rotatable) -> tuple:
    """((history name, offset), ...) of ``rotatable``, checked against the law's history"""
    dims = dict(_history_dims(model))
    out = []
    for name, offsets in rotatable.items():
        if name not in dims:
            raise ValueError(f"JaumannRate: rotatable names history '{name}', which {type(model).__name__} does not have "
                             f"(history: {sorted(dims)})")
        if isinstance(offsets, (int, float, str)):
            raise ValueError(f"JaumannRate: rotatable['{name}'] must be a list of offsets, not {offsets!r}")
        taken = set()
        for off in offsets:
            if isinstance(off, bool) or not hasattr(off, "__index__"):
                raise ValueError(f"JaumannRate: rotatable['{name}'] offset {off!r} is not an integer")
            off = off.__index__()
            if off < 0 or off + 6 > dims[name]:
                raise ValueError(f"JaumannRate: the Mandel block at offset {off} of history '{name}' runs past the end of its "
                                 f"{dims[name]} doubles per point")
            if taken & set(range(off, off + 6)):
                raise ValueError(f"JaumannRate: the blocks of history '{name}' overlap at offset {off}")
            taken |= set(range(off, off + 6))
            out.append((name, off))
    return tuple(out)


def _fused_law(model, blocks):
    """the law with the rotation compiled into its kernel, or None where only the array-level path exists"""
    from . import models as M
    from . import userlaw_sources as S

    if isinstance(model, UserLaw):
        return UserLaw(model.source, model.parameters, model.history_dim, model.constraint, name=model.name,
                       tangent=model.tangent_mode, unknowns=model.unknowns, newton=model.newton, fields=model.fields or None,
                       _rotate=blocks)
    if getattr(model, "field_points", None) is not None:
        return None
    if type(model) is M.LinearElasticityModel:
        src, p, hist = S.LINEAR_ELASTICITY, dict(zip(("E", "nu"), model._parameter_vector)), None
    elif type(model) is M.SpringMaxwellModel:
        src, p = S.SPRING_MAXWELL, {"E0": model.E0, "E1": model.E1, "tau": model.tau, "nu": model.nu}
        hist = {"strain_visco": 6, "strain": 6}
    elif type(model) is M.VonMises3D:
        src = S.VON_MISES_3D
        p = {k: getattr(model, k) for k in ("p_ka", "p_mu", "p_y0", "p_y00", "p_w")}
        hist = {"eps_n": 6, "alpha": 1}
    else:
        return None
    name = {S.LINEAR_ELASTICITY: "linear_elasticity", S.SPRING_MAXWELL: "spring_maxwell", S.VON_MISES_3D: "von_mises_3d"}[src]
    return UserLaw(src, p, hist, StressStrainConstraint.FULL, name=name, _rotate=blocks)


class JaumannRate(jit.JitLaw):
    """A FULL ``IncrSmallStrainModel`` of this package whose committed state is rotated with the material before every
    evaluation (Jaumann rate, Hughes-Winget rotation; module docstring).

    ``rotatable``: history name -> list of offsets, each the start of a Mandel 6-vector ``[xx, yy, zz, r xy, r xz, r yz]``
    (r = sqrt(2)) inside that field's per-point row; None takes ``default_rotatable(model)``.  The stress always rotates.

    ``G = grad_del_u`` means what the caller means by it: in an updated-Lagrangian loop, the gradient of the displacement
    increment on the current configuration.  The tangent is the law's ``d sigma / d delta eps`` at the rotated state (the UMAT
    convention): it has no geometric or spin term.

    ``evaluate`` (NumPy arrays or device tensors, in place) and ``evaluate_from`` (device tensors, out of place: the committed
    arrays are left untouched) as the wrapped law.  Refused with ``NotImplementedError``: ``ResidentState``,
    ``ResidentProblemState``, ``MultiDeviceResidentState``, ``batched_launches``, ``evaluate_indexed`` and the ``*From3D``
    wrappers.  ``fused = False`` (on the instance) forces the array-level path."""

    #: use the kernel with the rotation compiled in where one exists; False: the standalone rotation kernel, then the law
    fused = True

    def __init__(self, model, rotatable=None):
        from .device import DeviceLaw

        if isinstance(model, JaumannRate):
            raise ValueError("JaumannRate: the model is a JaumannRate already")
        if not isinstance(model, (DeviceLaw, UserLaw)):
            raise NotImplementedError(f"JaumannRate: {type(model).__name__} is not a law of this package (a DeviceLaw or a UserLaw)")
        if model.constraint != StressStrainConstraint.FULL:
            raise NotImplementedError(f"JaumannRate: constraint {model.constraint.name}: objective rates need the FULL (3-D) law")
        if getattr(model, "_devices", None) is not None:
            self._refuse("a law on several GPUs (use_devices)")
        self.model = model
        if rotatable is None:
            rotatable = default_rotatable(model)
        if not hasattr(rotatable, "items"):
            raise ValueError(f"JaumannRate: rotatable must map history names to lists of offsets, not {rotatable!r}")
        self._blocks = _blocks(model, rotatable)
        self.rotatable = {}
        for name, off in self._blocks:
            self.rotatable.setdefault(name, []).append(off)
        self._fused = _fused_law(model, self._blocks)
        self._hist = _history_dims(model)
        self._rot_fields = [(name, dim) for name, dim in self._hist if any(b[0] == name for b in self._blocks)]
        self._rot = None  # the standalone rotation kernel, compiled on first use
        self._last = model  # the law that ran last (device_stats)

    @staticmethod
    def _refuse(what: str):
        raise NotImplementedError(f"JaumannRate: {what} is not supported for objective-rate wrappers")

    def evaluate_path(self, *args, **kwargs):
        self._refuse("evaluate_path (a Mandel load path has no spin)")

    # -- interface ------------------------------------------------------------------------------------------------------
    @property
    def constraint(self) -> StressStrainConstraint:
        return StressStrainConstraint.FULL

    @property
    def history_dim(self):
        return self.model.history_dim

    @property
    def field_points(self):
        return getattr(self.model, "field_points", None)

    @property
    def path(self) -> str:
        """``"fused"`` or ``"array"``: the path the next call takes"""
        return "fused" if self.fused and self._fused is not None else "array"

    @property
    def resources(self) -> dict:
        """the compiler's resource report of the fused kernel (``UserLaw.resources``), else of the rotation kernel"""
        if self.path == "fused":
            return self._fused.resources
        return dict(self._rotate_kernel().resources)

    def update(self) -> None:
        self.model.update()

    def device_stats(self, device: int = 0):
        """``device_stats`` of the law that ran last on the call's behalf (the fused UserLaw returns its count, a built-in law
        raises on non-convergence)"""
        return self._last.device_stats(device)

    # -- evaluate ---------------------------------------------------------------------------------------------------------
    def _spring_checks(self, del_t) -> None:
        from .models import _SpringBase

        if isinstance(self.model, _SpringBase):
            assert del_t > 0, "Time step must be defined and positive."

    def evaluate(self, t, del_t, grad_del_u, stress, tangent, history, check: bool = False) -> None:
        """``IncrSmallStrainModel.evaluate`` with the committed ``stress`` and history rotated first; all in place."""
        self._refuse_batched()
        self._spring_checks(del_t)
        if self.path == "fused":
            self._last = self._fused
            self._fused.evaluate(t, del_t, grad_del_u, stress, tangent, history, check=check)
            return
        self._last = self.model
        hist = self._history_arrays(history)
        n = self._sizes(grad_del_u, stress, tangent, hist)
        self._check_fields(n)
        if _is_torch(grad_del_u):
            self._check_call(grad_del_u, stress, stress, tangent, hist, hist)
            self._rotate(n, grad_del_u, stress, stress, hist, hist)
            self.model.evaluate(t, del_t, grad_del_u, stress, tangent, history, check=check)
            return
        self._evaluate_host(t, del_t, n, grad_del_u, stress, tangent, hist)

    def evaluate_from(self, t, del_t, grad_del_u, stress_prev, stress, tangent, history_prev, history) -> None:
        """Out-of-place device evaluate: reads the committed state (``stress_prev``, ``history_prev``, never written), rotates
        it into ``stress`` / ``history`` and evaluates there.  Device tensors only."""
        self._refuse_batched()
        self._spring_checks(del_t)
        if not _is_torch(grad_del_u):
            raise TypeError("JaumannRate.evaluate_from takes device tensors (use evaluate for NumPy arrays)")
        if self.path == "fused":
            self._last = self._fused
            self._fused.evaluate_from(t, del_t, grad_del_u, stress_prev, stress, tangent, history_prev, history)
            return
        self._last = self.model
        hist, hprev = self._history_arrays(history), self._history_arrays(history_prev)
        n = self._sizes(grad_del_u, stress, tangent, hist, stress_prev, hprev)
        self._check_fields(n)
        self._check_call(grad_del_u, stress_prev, stress, tangent, hprev, hist)
        rotated = {name for name, _ in self._rot_fields}
        for (name, _), hp, h in zip(self._hist, hprev, hist):
            if name not in rotated:  # the rotation kernel writes the rotated fields; the rest is the committed state as it is
                _check_torch(f"history['{name}']", h).copy_(_check_torch(f"history_prev['{name}']", hp))
        self._evaluate_device(t, del_t, n, grad_del_u, stress_prev, stress, tangent, hprev, hist)

    def _check_fields(self, n: int) -> None:
        """the array-level path: a user law's size check of its parameter fields, before the rotation kernel writes"""
        if isinstance(self.model, UserLaw):
            self.model._check_field_points(n)

    def _check_call(self, grad, stress_prev, stress, tangent, hist_prev, hist) -> None:
        """the array-level path on device tensors: what the wrapped law will refuse (``UserLaw._check_device_arrays``;
        ``DeviceLaw._evaluate_device`` and ``check_device_ex`` of fcamd_capi.cpp), with its error, before the rotation kernel
        writes the rotated state over the committed one (in place) or into the trial arrays.  The rotation kernel itself moves
        8-byte words and needs no alignment; the laws' kernels move 16-byte chunks."""
        if isinstance(self.model, UserLaw):
            self.model._check_device_arrays(grad, stress_prev, stress, tangent, hist_prev, hist)
            return
        from . import _capi

        arrays = [("grad_del_u", grad), ("stress", stress)] + ([] if tangent is None else [("tangent", tangent)])
        arrays += [(f"history['{name}']", h) for (name, _), h in zip(self._hist, hist)]
        if stress_prev is not stress:
            arrays += [("stress_prev", stress_prev)] + [("history_prev", h) for h in hist_prev]
        for label, a in arrays:
            _check_torch(label, a)
        if any(a.data_ptr() % 16 for label, a in arrays if not label.startswith("history")):
            raise ValueError(_capi.status_string(_capi.ERR_ALIGN))
        if any(a.data_ptr() % 16 for label, a in arrays if label.startswith("history")):
            raise ValueError("device history arrays must be 16-byte aligned")

    def _evaluate_device(self, t, del_t, n, grad, stress_prev, stress, tangent, hist_prev, hist) -> None:
        """the array-level path on device tensors: the rotated committed state into ``stress`` and the rotated fields of
        ``hist`` (the others hold the committed state already), then the law evaluates there in place"""
        self._rotate(n, grad, stress_prev, stress, hist_prev, hist)
        self.model.evaluate(t, del_t, grad, stress, tangent, {name: h for (name, _), h in zip(self._hist, hist)})

    def _nonconverged(self, device: int) -> int:
        count = self.model.device_stats(device)  # a built-in law raises here
        return count if isinstance(self.model, UserLaw) else 0

    # -- the standalone rotation kernel ---------------------------------------------------------------------------------
    def _rotate_kernel(self):
        if self._rot is None:
            names = {name: f"f{k}" for k, (name, _) in enumerate(self._rot_fields)}
            lines = [f"#define FCAMD_ROT_NFIELDS {len(self._rot_fields)}",
                     "#define FCAMD_ROT_FIELDS(X) " + " ".join(f"X({k}, {names[n]}, {d})" for k, (n, d) in enumerate(self._rot_fields)),
                     "#define FCAMD_USER_ROTATE(X) " + " ".join(f"X({names[n]}, {o})" for n, o in self._blocks),
                     "struct RotHistory {" + "".join(f" double {names[n]}[{d}];" for n, d in self._rot_fields) + " };",
                     '#include "rotate_state.hip"']
            self._rot = jit.compile_program("\n".join(lines) + "\n", "jaumann_rotate_state", ROTATE_KERNEL)
            if self._rot.resources.get("scratch_bytes"):
                raise RuntimeError(f"JaumannRate: the rotation kernel uses {self._rot.resources['scratch_bytes']} bytes of scratch")
        return self._rot

    def _rotate(self, n, grad, stress_in, stress_out, hist_in, hist_out) -> None:
        """the rotated committed state -> ``stress_out`` and the rotated history fields of ``hist_out`` (asynchronous, on torch's
        current stream)"""
        rotated = {name for name, _ in self._rot_fields}
        pairs = [(hi, ho) for (name, _), hi, ho in zip(self._hist, hist_in, hist_out) if name in rotated]
        dev = grad.device.index or 0
        for label, a in [("grad_del_u", grad), ("stress_prev", stress_in), ("stress", stress_out)] + \
                [("history", x) for p in pairs for x in p]:
            _check_torch(label, a)
            if (a.device.index or 0) != dev:
                raise ValueError(f"{label} is on {a.device}, grad_del_u on cuda:{dev}")
        if n == 0:
            return
        a = _rotate_args_type(max(1, len(pairs)))()
        a.grad, a.s_in, a.s_out = grad.data_ptr(), stress_in.data_ptr(), stress_out.data_ptr()
        for k, (hi, ho) in enumerate(pairs):
            a.h_in[k], a.h_out[k] = hi.data_ptr(), ho.data_ptr()
        a.n = n
        jit.launch(self._rotate_kernel(), dev, min((n + 255) // 256, 64 * jit.num_cu(dev)), a, "JaumannRate rotation launch")


def _rotate_args_type(nf: int):
    """ctypes mirror of RotateArgs (rotate_state.hip) for ``nf`` history slots"""
    vp = C.c_void_p

    class RotateArgs(C.Structure):
        _fields_ = [("grad", vp), ("s_in", vp), ("s_out", vp), ("h_in", vp * nf), ("h_out", vp * nf), ("n", C.c_int64)]

    return RotateArgs
