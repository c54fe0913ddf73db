"""User-defined constitutive laws compiled at run time to HIP kernels for gfx950.

A ``UserLaw`` is one ``__device__`` point function in HIP C++, given as a Python string (the contract: ``csrc/jit/user_law_api.h``,
INTEGRATION.md "Custom laws").  The constructor generates the parameter and history structs from the law's dicts and compiles
them, with the user's source and the kernel template ``csrc/jit/user_law.hip``, through ``jit`` (hiprtc, cached); the template's
tile code (``csrc/jit/user_law_tile.h``) does all the memory work with the built-in kernels' own (``csrc/kernels/tile_io.h``).
The first call on a device loads the code object there and every call launches it on torch's current stream.  Compiling needs
no GPU: the arch is fixed.

With ``tangent="autodiff"`` the source defines a stress and history update templated on the scalar type, compiled inside
``csrc/jit/user_law_ad.hip``; the tangent comes from forward-mode automatic differentiation (``csrc/jit/user_law_ad.h``).

With ``tangent="implicit"`` the source states the law as a residual in ``unknowns`` local unknowns and the state update from
their solution (``csrc/jit/user_law_implicit.h``); the kernel template ``csrc/jit/user_law_implicit.hip`` brings the Jacobian (dual
numbers), the per-point Newton loop, the dense solve and the consistent tangent by the implicit-function theorem.

A parameter given in ``fields`` instead of ``parameters`` is a per-point field: one value per quadrature point, loaded by the
point's lane (``csrc/jit/user_law_fields.h``).  The source does not change: a field is a ``double`` member of ``UserParams`` like a
scalar.

``evaluate_path`` drives every point through a whole load path of S increments in one launch, with the state in registers
across the steps and any set of Mandel components stress-controlled (a Newton loop per point on the law's own tangent entries,
or on ``Dual`` partials seeded on the controlled components only): the kernel template ``csrc/jit/user_law_path.hip``, compiled
on first use per control set behind the same generated definitions.  Implicit laws: strain control only.

The 1-D / 2-D wrappers (``wrappers.py``: uniaxial strain, plane strain, plane stress, uniaxial stress) run a law with an explicit
or autodiff tangent as one launch of the kernel template ``csrc/jit/user_law_wrapped.hip``, compiled on first use per wrapper
(``_wrapped_kernel``, ``wrapped_resources``; the launch: ``_evaluate_wrapped``): map, evaluate -- under the stress wrappers inside a
Newton loop per point in registers -- and map back, with only the wrapper's cached 3-D stress next to the low-dimensional arrays
(DESIGN.md §18).  Implicit laws go through the wrappers' generic path.

FULL constraint, ``evaluate`` / ``evaluate_from`` / ``evaluate_path``: the resident, batched, indexed and multi-GPU forms of the built-in laws are
refused with ``NotImplementedError``.
"""

from __future__ import annotations

import ctypes as C
import re
import warnings

import numpy as np

from . import _capi, jit
from .device import _check_numpy, _check_torch, _is_torch, _size
from .interfaces import StressStrainConstraint
from .jit import UserLawCompileError, _cache, compile_count  # noqa: F401 (importable from here, as before jit.py)

__all__ = ["UserLaw", "UserLawCompileError", "compile_count"]

KERNEL = "fcamd_user_law_kernel"
MAX_PARAMS = 32  # UserArgs.params (user_law_tile.h: kMaxParams)
#: register budgets tried in turn (waves per SIMD: 128 / 168 / 256 VGPRs): the first without scratch is kept
WAVES_PER_SIMD = (4, 3, 2)
#: tangent kernels of autodiff laws: (waves per SIMD, directions per pass) tried in turn, the first without scratch is kept.  One
#: pass (K = 6) at any budget first: it writes the tangent as coalesced 16-byte chunks, while K < 6 writes every pass's columns
#: as 8-byte entries (SpringMaxwellModel: 2.09x the time of K = 6 at 3 instead of 2 waves); then the most waves
#: with the fewest passes
AD_LADDER = tuple((w, 6) for w in WAVES_PER_SIMD) + tuple((w, k) for w in WAVES_PER_SIMD for k in (3, 2, 1))
#: the path kernel (evaluate_path) holds the committed and the trial state, the load row and the control system next to the
#: law's temporaries: its ladder goes down to a lone wave per SIMD (512 registers), as IMPLICIT_BUDGETS does
PATH_WAVES_PER_SIMD = (4, 3, 2, 1)
PATH_KERNEL = "fcamd_user_law_path_kernel"
#: evaluate_path: max_iter and tol of the stress-control Newton loop
PATH_NEWTON_DEFAULTS = {"max_iter": 25, "tol": 1e-10}
#: the 1-D / 2-D wrappers (wrappers.py) around an explicit or autodiff law: one kernel per wrap mode (csrc/jit/user_law_wrapped.hip),
#: the stress wrappers with the committed and the trial state and the local Newton iteration in registers -- the path kernel's ladder
WRAPPED_WAVES_PER_SIMD = (4, 3, 2, 1)
WRAPPED_KERNEL = "fcamd_user_law_wrapped_kernel"
#: FCAMD_USER_WRAP, the built-in kernels' numbering (kernels/wrapped_io.h, stress_wrapped.h)
WRAP_MODES = {StressStrainConstraint.UNIAXIAL_STRAIN: 1, StressStrainConstraint.PLANE_STRAIN: 2,
              StressStrainConstraint.PLANE_STRESS: 3, StressStrainConstraint.UNIAXIAL_STRESS: 4}
TANGENT_MODES = ("explicit", "autodiff", "implicit")
#: implicit laws: the most local unknowns (an 8 x 8 Jacobian and its right-hand sides stay in registers)
MAX_UNKNOWNS = 8
#: implicit laws: max_iter and tol travel in two slots of UserArgs.params behind the law's own parameters
MAX_IMPLICIT_PARAMS = MAX_PARAMS - 2
NEWTON_DEFAULTS = {"max_iter": 50, "tol": 1e-10}
MAX_HISTORY_DIM = 36  # doubles per point of one history field (user_law_tile.h: kUserMaxDim)
FACTOR_PY = float.fromhex("0x1.6a09e667f3bccp-1")  # the off-diagonal Mandel factor of the Python laws (fcamd_capi.cpp: kFactorPy)

_CXX_KEYWORDS = frozenset("""
alignas alignof and and_eq asm auto bitand bitor bool break case catch char char8_t char16_t char32_t class compl concept const
consteval constexpr constinit const_cast continue co_await co_return co_yield decltype default delete do double dynamic_cast else
enum explicit export extern false float for friend goto if inline int long mutable namespace new noexcept not not_eq nullptr
operator or or_eq private protected public register reinterpret_cast requires return short signed sizeof static static_assert
static_cast struct switch template this thread_local throw true try typedef typeid typename union unsigned using virtual void
volatile wchar_t while xor xor_eq restrict
""".split())
_IDENT = re.compile(r"[A-Za-z_][A-Za-z0-9_]*\Z")


def _check_name(name, what: str) -> str:
    if not isinstance(name, str) or not _IDENT.match(name):
        raise ValueError(f"UserLaw: {what} name {name!r} is not a C identifier")
    if name in _CXX_KEYWORDS:
        raise ValueError(f"UserLaw: {what} name {name!r} is a C++ keyword")
    return name


def _items(d):
    """(name, value) pairs of a mapping or of a sequence of pairs (where repeats can be written)"""
    if d is None:
        return []
    return list(d.items()) if hasattr(d, "items") else [tuple(x) for x in d]


def _param_value(name, value) -> float:
    if isinstance(value, np.ndarray) or _is_torch(value) or isinstance(value, (list, tuple)):
        raise NotImplementedError(f"UserLaw: parameter '{name}' is an array; user laws take scalar parameters only "
                                  "(per-point parameter fields are not supported)")
    return float(value)


def _field_value(name, value) -> np.ndarray:
    """a host copy of the per-point field ``value``: a 1-D float64 NumPy array or ROCm tensor over ``len(value)`` >= 1 points
    (one element: a field over one point).  The messages of ``device.parameter_field``."""
    if _is_torch(value):
        import torch

        shape, is_f64 = tuple(value.shape), value.dtype == torch.float64
    elif isinstance(value, np.ndarray):
        shape, is_f64 = value.shape, value.dtype == np.float64
    else:
        raise TypeError(f"UserLaw: field '{name}' must be a 1-D float64 NumPy array or ROCm tensor, got {type(value).__name__}")
    if len(shape) != 1:
        raise ValueError(f"parameter field '{name}' must be 1-D, got shape {shape}")
    if not is_f64:
        raise TypeError(f"parameter field '{name}' must be float64, got {value.dtype}")
    if shape[0] < 1:
        raise ValueError(f"parameter field '{name}' is empty; a field has one value per point")
    if _is_torch(value):
        return value.detach().cpu().numpy().copy()
    return np.array(value, dtype=np.float64, copy=True)


def _dim_value(name, dim) -> int:
    if isinstance(dim, tuple):
        d = int(np.prod([int(x) for x in dim])) if dim else 0
    else:
        d = int(dim)
    if d < 1 or d > MAX_HISTORY_DIM:
        raise ValueError(f"UserLaw: history field '{name}' has {d} doubles per point; 1 to {MAX_HISTORY_DIM} are supported")
    return d


def jacobian_directions(unknowns: int) -> tuple:
    """directions per Jacobian pass tried for ``unknowns`` local unknowns: one pass, two passes, one unknown per pass"""
    return tuple(sorted({unknowns, (unknowns + 1) // 2, 1}, reverse=True))


#: implicit laws: registers per lane at each number of waves per SIMD (1: the 256 accumulation registers of a lone wave too)
IMPLICIT_BUDGETS = {4: 128, 3: 168, 2: 256, 1: 512}


def implicit_register_floor(unknowns: int, tangent_directions: int, state_doubles: int) -> int:
    """registers an implicit kernel whose Jacobian is dense and varies holds at once (two per double): the Jacobian, the
    right-hand sides of the solve (the residual, or ``tangent_directions`` columns of dr / deps), x, the strain increment and the
    committed state.  Rungs below it are not tried: for such a law each would cost a compilation that ends in scratch (the eight
    unknowns of VON_MISES_SWIFT_GENERAL: 27 compilations, 80 s).  A law whose Jacobian folds to constants needs less; the compiler
    then takes less than the rung allows and ``resources["waves_per_simd"]`` shows the occupancy it reached."""
    return 2 * (unknowns * unknowns + unknowns * max(tangent_directions, 1) + unknowns + 6 + state_doubles)


def implicit_ladder(unknowns: int, tangent: bool, state_doubles: int = 6) -> tuple:
    """implicit laws: the rungs tried in turn, the first without scratch is kept.  Stress-only kernel: (waves per SIMD,
    directions per Jacobian pass), the most waves first and at each the fewest passes.  Tangent kernel: (waves, directions per
    Jacobian pass, directions per tangent pass), the single tangent pass at any budget first as in ``AD_LADDER``; the several-pass
    rungs evaluate the Jacobian again in every pass and take it one unknown at a time.  ``state_doubles``: committed stress and
    history per point.  A rung whose budget is below ``implicit_register_floor`` is left out; the last rung always stays."""
    kj = jacobian_directions(unknowns)
    if not tangent:
        rungs = tuple((w, k) for w in IMPLICIT_BUDGETS for k in kj)
    else:
        rungs = tuple((w, k, 6) for w in IMPLICIT_BUDGETS for k in kj) + tuple((w, 1, kt) for w in IMPLICIT_BUDGETS for kt in (3, 2, 1))
    fit = tuple(r for r in rungs if IMPLICIT_BUDGETS[r[0]] >= implicit_register_floor(unknowns, r[2] if tangent else 0, state_doubles))
    return fit or rungs[-1:]


def _control_set(stress_controlled) -> tuple:
    """evaluate_path's ``stress_controlled`` as a tuple of distinct Mandel component indices 0-5"""
    if isinstance(stress_controlled, (str, bytes)) or not hasattr(stress_controlled, "__iter__"):
        raise ValueError(f"UserLaw: stress_controlled={stress_controlled!r}; expected a tuple of component indices 0-5")
    out = []
    for c in stress_controlled:
        if isinstance(c, bool) or not hasattr(c, "__index__"):
            raise ValueError(f"UserLaw: stress_controlled holds {c!r}; expected ints (Mandel component indices 0-5)")
        c = c.__index__()
        if not 0 <= c <= 5:
            raise ValueError(f"UserLaw: stress_controlled holds {c}; Mandel component indices are 0-5")
        if c in out:
            raise ValueError(f"UserLaw: stress_controlled holds {c} more than once")
        out.append(c)
    return tuple(out)


def _path_del_t(del_t):
    """evaluate_path's time increments, float64 [S]: (S, the contiguous ROCm tensor that holds them or None, the host array or None)"""
    if _is_torch(del_t):
        import torch

        if del_t.dtype != torch.float64:
            raise TypeError(f"del_t must be float64, got {del_t.dtype}")
        if del_t.dim() != 1:
            raise ValueError(f"del_t must be 1-D (one increment per step), got shape {tuple(del_t.shape)}")
        if del_t.is_cuda and del_t.is_contiguous():
            return int(del_t.shape[0]), del_t, None
        del_t = del_t.detach().cpu().contiguous().numpy()
    if not isinstance(del_t, np.ndarray):
        raise TypeError(f"del_t must be a 1-D float64 array of time increments, got {type(del_t).__name__}")
    if del_t.dtype != np.float64:
        raise TypeError(f"del_t must be float64, got {del_t.dtype}")
    if del_t.ndim != 1:
        raise ValueError(f"del_t must be 1-D (one increment per step), got shape {del_t.shape}")
    return len(del_t), None, np.ascontiguousarray(del_t)


def _newton_options(newton, defaults=None) -> dict:
    defaults = NEWTON_DEFAULTS if defaults is None else defaults
    if newton is None:
        return dict(defaults)
    if not hasattr(newton, "items"):
        raise ValueError(f"UserLaw: newton must be a dict with the keys {sorted(defaults)}, not {newton!r}")
    if set(newton) != set(defaults):
        raise ValueError(f"UserLaw: newton has the keys {sorted(map(str, newton))}; expected exactly {sorted(defaults)}")
    max_iter, tol = newton["max_iter"], newton["tol"]
    if isinstance(max_iter, bool) or not hasattr(max_iter, "__index__") or not 0 <= max_iter.__index__() < 2 ** 31:
        raise ValueError(f"UserLaw: newton['max_iter'] = {max_iter!r}; expected an int >= 0")
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.floating, np.integer)) or not 0.0 < float(tol) < float("inf"):
        raise ValueError(f"UserLaw: newton['tol'] = {tol!r}; expected a float > 0")
    return {"max_iter": max_iter.__index__(), "tol": float(tol)}


def refuse_user_law(law, what: str) -> None:
    """the forms of the built-in laws that user laws and objective-rate wrappers do not have (resident and multi-GPU states)"""
    if isinstance(law, jit.JitLaw):
        law._refuse(what)


class UserLaw(jit.JitLaw):
    """A constitutive law written by the user as one HIP C++ point function (``source``; contract in
    ``csrc/jit/user_law_api.h``), compiled at construction for gfx950.

    ``parameters``: name -> scalar float, at most 32; the values are kernel arguments, so laws that differ only in them share
    one code object.  ``history_dim``: name -> doubles per point (an int or a tuple, whose product counts), or None.  The
    names are C identifiers, not C++ keywords, and do not repeat.  FULL constraint only.

    ``fields``: name -> 1-D float64 NumPy array or ROCm tensor, a parameter with one value per point (a dict or a list of pairs;
    an array in ``parameters`` stays refused).  All fields have the same length, ``field_points``, and every call must have that
    many points.  The values are copied here and uploaded once per device on first use.  A field is a ``double`` member of
    ``UserParams`` behind the scalars, so a source reads ``p.K`` whether ``K`` is a scalar or a field; parameters and fields
    together count against the 32.  Laws that differ only in field values or lengths share one code object.

    ``tangent``: ``"explicit"`` (the source defines ``fcamd_user_point``, which writes the tangent itself) or ``"autodiff"`` (the
    source defines the function template ``fcamd_user_stress<T>``, stress and history only; the tangent comes from forward-mode
    automatic differentiation, contract in ``csrc/jit/user_law_ad.h``) or ``"implicit"`` (the source defines the templates
    ``fcamd_user_start<T>``, ``fcamd_user_residual<T>`` and ``fcamd_user_update<T>`` over ``unknowns`` local unknowns; the kernel
    solves the residual per point by Newton's method and forms the consistent tangent, contract in
    ``csrc/jit/user_law_implicit.h``).

    Implicit mode only: ``unknowns`` (1 to ``MAX_UNKNOWNS``, required) and ``newton`` (``{"max_iter": int >= 0, "tol": float > 0}``,
    default 50 and 1e-10: a point is converged when every ``|r_i| <= tol``).  Both Newton values are kernel arguments, which
    leaves such a law at most 30 parameters."""

    def __init__(self, source: str, parameters=None, history_dim=None, constraint: StressStrainConstraint = None,
                 name: str = "user_law", tangent: str = "explicit", unknowns: int = None, newton: dict = None, fields=None, *, _rotate=None):
        if not isinstance(tangent, str) or tangent not in TANGENT_MODES:
            raise ValueError(f"UserLaw: tangent={tangent!r}; expected one of {TANGENT_MODES}")
        self.tangent_mode = tangent
        implicit = tangent == "implicit"
        if implicit:
            if isinstance(unknowns, bool) or not hasattr(unknowns, "__index__") or not 1 <= unknowns.__index__() <= MAX_UNKNOWNS:
                raise ValueError(f"UserLaw: unknowns={unknowns!r}; implicit laws need an int from 1 to {MAX_UNKNOWNS}")
            self._unknowns = unknowns.__index__()
            self._newton = _newton_options(newton)
        else:
            if unknowns is not None or newton is not None:
                raise ValueError(f"UserLaw: unknowns and newton belong to tangent='implicit', not to tangent={tangent!r}")
            self._unknowns, self._newton = None, None
        constraint = StressStrainConstraint.FULL if constraint is None else constraint
        if constraint != StressStrainConstraint.FULL:
            raise NotImplementedError(f"UserLaw: constraint {constraint.name}: user laws are FULL (3-D) only; wrap one in "
                                      "UniaxialStrainFrom3D / PlaneStrainFrom3D for lower dimensions")
        self._constraint = constraint
        self.name = str(name)
        params = _items(parameters)
        hist = _items(history_dim)
        flds = _items(fields)
        seen = set()
        for what, pairs in (("parameter", params), ("field", flds), ("history", hist)):
            for n, _ in pairs:
                _check_name(n, what)
                if n in seen:
                    raise ValueError(f"UserLaw: name '{n}' is given more than once")
                seen.add(n)
        if len(params) + len(flds) > (MAX_IMPLICIT_PARAMS if implicit else MAX_PARAMS):
            raise ValueError(f"UserLaw: {len(params) + len(flds)} parameters" + (" and fields" if flds else "")
                             + f"; at most {MAX_IMPLICIT_PARAMS if implicit else MAX_PARAMS}"
                             + (" for an implicit law (max_iter and tol take two slots)" if implicit else ""))
        self._param_names = tuple(n for n, _ in params)
        self._param_values = [_param_value(n, v) for n, v in params]
        # per-point parameter fields: host copies, uploaded once per device on first use (_field_ptrs)
        self._field_names = tuple(n for n, _ in flds)
        self._field_values = [_field_value(n, v) for n, v in flds]
        if len({len(f) for f in self._field_values}) > 1:
            raise ValueError(f"all parameter fields of a law have the same length, got {sorted({len(f) for f in self._field_values})}")
        self._field_dev = {}  # device -> the fields' device copies
        self._history_dim = history_dim
        self._hist = [(n, _dim_value(n, d)) for n, d in hist]
        self.source = source
        # objective.JaumannRate: ((history field, offset), ...) of the Mandel blocks rotated with the stress before the law runs
        self._rotate = None if _rotate is None else tuple((str(f), int(o)) for f, o in _rotate)
        self._directions = None
        self._rung, self._rung_stress = None, None  # implicit laws: the rungs of implicit_ladder kept
        if implicit:
            # two code objects as in autodiff mode, each the first rung of its ladder without scratch
            state = 6 + sum(d for _, d in self._hist)
            for rung in implicit_ladder(self._unknowns, False, state):
                self._compiled_stress = jit.compile_program(self._program_implicit(source, *rung, 0), self.name, KERNEL)
                self._rung_stress = rung
                if not self._compiled_stress.resources.get("scratch_bytes"):
                    break
            for rung in implicit_ladder(self._unknowns, True, state):
                self._compiled = jit.compile_program(self._program_implicit(source, *rung), self.name, KERNEL)
                self._rung = rung
                if not self._compiled.resources.get("scratch_bytes"):
                    break
        elif tangent == "explicit":
            # cut for 4 waves per SIMD (128 VGPRs; the LDS allows no more); a law that spills there is compiled again for fewer waves
            for waves in WAVES_PER_SIMD:
                self._compiled = jit.compile_program(self._program(source, waves), self.name, KERNEL)
                if not self._compiled.resources.get("scratch_bytes"):
                    break
            self._compiled_stress = self._compiled
        else:
            # two code objects: the stress-only kernel (T = double) for tangent=None launches, the tangent kernel (Dual<K>)
            for waves in WAVES_PER_SIMD:
                self._compiled_stress = jit.compile_program(self._program_ad(source, waves, 0), self.name, KERNEL)
                if not self._compiled_stress.resources.get("scratch_bytes"):
                    break
            for waves, k in AD_LADDER:
                self._compiled = jit.compile_program(self._program_ad(source, waves, k), self.name, KERNEL)
                self._directions = k
                if not self._compiled.resources.get("scratch_bytes"):
                    break
        for c in {id(self._compiled): self._compiled, id(self._compiled_stress): self._compiled_stress}.values():
            if c.resources.get("scratch_bytes"):
                warnings.warn(f"UserLaw '{self.name}': the kernel uses {c.resources['scratch_bytes']} bytes of scratch per lane "
                              f"(VGPRs: {c.resources.get('vgprs')}); register spills cost memory bandwidth", UserWarning, stacklevel=2)
        self._counters = {}  # device -> int64 device word (non-converged points of the last launch)
        self._empty = {}  # device -> the last call had no points
        self._args_cls = _args_type(max(1, len(self._hist)), len(self._field_names))
        self._path_compiled = {}  # stress-controlled components -> (code object, rung) of the path kernel, compiled on first use
        self._path_args_cls = _path_args_type(max(1, len(self._hist)), len(self._field_names))
        self._wrapped_compiled = {}  # wrap mode -> (code object, rung) of the wrapped kernel, compiled on first use
        self._wrapped_args_cls = _wrapped_args_type(max(1, len(self._hist)))

    # -- program --------------------------------------------------------------------------------------------------------
    def _program(self, source: str, waves: int, directions: int = None, implicit: tuple = None, path: tuple = None,
                 wrap: int = None) -> str:
        """the generated definitions, the user's source, the kernel template.  ``directions``: autodiff mode's partials per
        Dual (0: the stress-only kernel); None in explicit mode.  ``implicit``: implicit mode's (directions per Jacobian pass,
        directions per tangent pass; 0: the stress-only kernel).  ``path``: the stress-controlled components of the path kernel
        (``evaluate_path``, csrc/jit/user_law_path.hip); None: an evaluate kernel.  ``wrap``: the wrap mode of the wrapped kernel
        (the 1-D / 2-D wrappers, csrc/jit/user_law_wrapped.hip)"""
        ad = directions is not None or implicit is not None
        template = "user_law_implicit.hip" if implicit is not None else "user_law_ad.hip" if ad else "user_law.hip"
        if path is not None:
            template = "user_law_path.hip"
        if wrap is not None:
            template = "user_law_wrapped.hip"
        p, f = self._param_names, self._field_names
        history, scalar = ("template <class T> struct UserHistoryT {", "T") if ad else ("struct UserHistory {", "double")
        mode = [f"#define FCAMD_USER_AD_K {directions}"] if directions is not None else []
        if implicit is not None:
            mode = [f"#define FCAMD_USER_UNKNOWNS {self._unknowns}", f"#define FCAMD_USER_IM_KJ {implicit[0]}",
                    f"#define FCAMD_USER_IM_KT {implicit[1]}", f"#define FCAMD_USER_IM_SLOT {len(p)}"]
        if path is not None:
            mode += [f"#define FCAMD_USER_PATH {3 if implicit is not None else 2 if ad else 1}", f"#define FCAMD_PATH_NCTRL {len(path)}"]
            mode += ["#define FCAMD_PATH_CTRL " + ", ".join(map(str, path))] if path else []
        if wrap is not None:
            mode += [f"#define FCAMD_USER_WRAP {wrap}"]
        lines = ['#include "user_law_implicit.h"' if implicit is not None else '#include "user_law_ad.h"' if ad else '#include "user_law_api.h"',
                 f"#define FCAMD_USER_WAVES {waves}",
                 *mode,
                 f"#define FCAMD_USER_NHIST {len(self._hist)}",
                 "#define FCAMD_USER_HISTORY_FIELDS(X) " + " ".join(f"X({k}, {n}, {d})" for k, (n, d) in enumerate(self._hist)),
                 "struct UserParams {" + "".join(f" double {n};" for n in p + f) + " };",
                 history + "".join(f" {scalar} {n}[{d}];" for n, d in self._hist) + " };"]
        if f:  # per lane: the launch's scalars, then the lane's field values (user_law_fields.h)
            lines += [f"#define FCAMD_USER_NFIELDS {len(f)}",
                      "#define FCAMD_USER_FIELDS(X) " + " ".join(f"X({k}, {n})" for k, n in enumerate(f)),
                      '#include "user_law_fields.h"',
                      "__device__ __forceinline__ UserParams fcamd_user_params(const double* v, const fcamd_user::UserFieldValues& f) {",
                      "    UserParams p;" + "".join(f" p.{n} = v[{k}];" for k, n in enumerate(p))
                      + "".join(f" p.{n} = f.v[{k}];" for k, n in enumerate(f))]
        else:
            lines += ["__device__ __forceinline__ UserParams fcamd_user_params(const double* v) {",
                      "    UserParams p;" + "".join(f" p.{n} = v[{k}];" for k, n in enumerate(p))]
        lines += ["    return p;",
                  "}"]
        if self._rotate is not None:  # the tile prologue (user_law_tile.h) rotates the committed state with rotation.h
            lines += ["#define FCAMD_USER_ROTATE(X) " + " ".join(f"X({f}, {o})" for f, o in self._rotate), '#include "rotation.h"']
        lines.append('#line 1 "' + re.sub(r'[^A-Za-z0-9_.]', '_', self.name) + '"')
        return "\n".join(lines) + "\n" + source + f'\n#include "{template}"\n'

    def _program_ad(self, source: str, waves: int, directions: int) -> str:
        """the program of autodiff mode (``directions``: partials per Dual, 0 for the stress-only kernel)"""
        return self._program(source, waves, directions)

    def _program_implicit(self, source: str, waves: int, jacobian_directions: int, tangent_directions: int) -> str:
        """the program of implicit mode (``tangent_directions``: 0 for the stress-only kernel)"""
        return self._program(source, waves, implicit=(jacobian_directions, tangent_directions))

    def _program_path(self, source: str, waves: int, stress_controlled: tuple, jacobian_directions: int = None) -> str:
        """the program of the path kernel (``jacobian_directions``: implicit mode's, as in its stress-only kernel)"""
        if self.tangent_mode == "implicit":
            return self._program(source, waves, implicit=(jacobian_directions, 0), path=stress_controlled)
        return self._program(source, waves, 0 if self.tangent_mode == "autodiff" else None, path=stress_controlled)

    def _program_wrapped(self, source: str, waves: int, wrap: int) -> str:
        """the program of the wrapped kernel (``wrap``: 1 uniaxial strain, 2 plane strain, 3 plane stress, 4 uniaxial stress)"""
        return self._program(source, waves, 0 if self.tangent_mode == "autodiff" else None, wrap=wrap)

    @property
    def unknowns(self):
        """implicit laws: the number of local unknowns (None in the other modes)"""
        return self._unknowns

    @property
    def newton(self):
        """implicit laws: ``{"max_iter", "tol"}`` of the Newton loop (None in the other modes)"""
        return None if self._newton is None else dict(self._newton)

    @property
    def resources(self) -> dict:
        """``{"vgprs", "sgprs", "scratch_bytes", "waves_per_simd", ...}`` of the compiled kernel (compiler remarks).  Autodiff
        laws: those of the tangent kernel, its ``"directions_per_pass"`` (K of Dual<K>; ceil(6 / K) passes) and under
        ``"stress_only"`` those of the kernel of tangent=None launches.  Implicit laws: ``"unknowns"`` and the rung kept
        (``implicit_ladder``) -- ``"rung_waves_per_simd"`` (the budget the kernel was cut for; ``"waves_per_simd"`` is the occupancy
        the compiler reports, which is higher where the kernel needs less), ``"jacobian_directions_per_pass"`` (K of the
        Dual<K> that J = dr / dx is taken with; ceil(N / K) passes), ``"directions_per_pass"`` of the tangent; ``"stress_only"``
        with its own ``"jacobian_directions_per_pass"``."""
        r = dict(self._compiled.resources)
        if self._rung is not None:
            r.update(unknowns=self._unknowns, rung_waves_per_simd=self._rung[0], jacobian_directions_per_pass=self._rung[1],
                     directions_per_pass=self._rung[2])
            r["stress_only"] = dict(self._compiled_stress.resources, rung_waves_per_simd=self._rung_stress[0],
                                    jacobian_directions_per_pass=self._rung_stress[1])
        if self._directions is not None:
            r["directions_per_pass"] = self._directions
            r["stress_only"] = dict(self._compiled_stress.resources)
        return r

    @property
    def compile_log(self) -> str:
        return self._compiled.log

    # -- interface ------------------------------------------------------------------------------------------------------
    @property
    def constraint(self) -> StressStrainConstraint:
        return self._constraint

    @property
    def history_dim(self):
        return self._history_dim

    @property
    def parameters(self) -> dict:
        """the scalar parameters (the fields: ``fields``)"""
        return dict(zip(self._param_names, self._param_values))

    # -- per-point parameter fields -----------------------------------------------------------------------------------------
    @property
    def field_points(self):
        """number of points of the law's parameter fields (``None``: no fields, every parameter is a scalar)"""
        return len(self._field_values[0]) if self._field_values else None

    @property
    def field_names(self) -> tuple:
        """the parameters given per point, in the order of ``UserParams``"""
        return self._field_names

    @property
    def fields(self) -> dict:
        """name -> a copy of the field's values"""
        return {n: f.copy() for n, f in zip(self._field_names, self._field_values)}

    def _check_field_points(self, n: int) -> None:
        """a call over ``n`` points fits the fields (``DeviceLaw._field_ptrs``' check), before anything is launched or written"""
        if self._field_values and n != self.field_points:
            raise AssertionError(f"{type(self).__name__}: the parameter fields have {self.field_points} points, the call has {n}")

    def _field_ptrs(self, device: int) -> list:
        """the device addresses of the fields on ``device``, uploaded there once"""
        dev = self._field_dev.get(device)
        if dev is None:
            import torch

            from .hostio import to_device

            dev = self._field_dev[device] = [to_device(f, torch.device("cuda", device)) for f in self._field_values]
        return [f.data_ptr() for f in dev]

    def update(self) -> None:
        pass

    # -- refused forms ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _refuse(what: str):
        raise NotImplementedError(f"UserLaw: {what} is not supported for user-defined laws")

    # -- evaluate ---------------------------------------------------------------------------------------------------------
    def evaluate(self, t, del_t, grad_del_u, stress, tangent, history, check: bool = False) -> None:
        """``IncrSmallStrainModel.evaluate``: overwrite ``stress``, ``tangent`` (unless None) and every history array in place.
        NumPy arrays: synchronous; raises the reference's ``RuntimeError`` if a point did not converge (after the results are
        written).  Device tensors: asynchronous on torch's current stream; ``check=True`` synchronises and raises the same
        error, otherwise ``device_stats()`` returns the count."""
        self._refuse_batched()
        hist = self._history_arrays(history)
        n = self._sizes(grad_del_u, stress, tangent, hist)
        self._check_field_points(n)
        if _is_torch(grad_del_u):
            self._evaluate_device(t, del_t, n, grad_del_u, stress, stress, tangent, hist, hist)
            if check:
                self._raise(self.device_stats(grad_del_u.device.index or 0))
            return
        self._evaluate_host(t, del_t, n, grad_del_u, stress, tangent, hist)

    def evaluate_from(self, t, del_t, grad_del_u, stress_prev, stress, tangent, history_prev, history) -> None:
        """Out-of-place device evaluate: reads the committed state (``stress_prev``, ``history_prev``), writes the trial state
        (``stress``, ``history``).  Device tensors only."""
        self._refuse_batched()
        hist, hprev = self._history_arrays(history), self._history_arrays(history_prev)
        n = self._sizes(grad_del_u, stress, tangent, hist, stress_prev, hprev)
        self._check_field_points(n)
        if not _is_torch(grad_del_u):
            raise TypeError("UserLaw.evaluate_from takes device tensors (use evaluate for NumPy arrays)")
        self._evaluate_device(t, del_t, n, grad_del_u, stress_prev, stress, tangent, hprev, hist)

    def _counter(self, device: int):
        c = self._counters.get(device)
        if c is None:
            import torch

            c = self._counters[device] = torch.zeros(1, dtype=torch.int64, device=torch.device("cuda", device))
        return c

    def _check_device_arrays(self, grad, stress_prev, stress, tangent, hist_prev, hist) -> int:
        """every tensor of a call is float64, contiguous, on grad_del_u's device (returned) and 16-byte aligned: the tile code
        moves 16-byte chunks.  Raises before anything is launched (objective.JaumannRate: before anything is rotated)."""
        arrays = [("grad_del_u", grad), ("stress_prev", stress_prev), ("stress", stress)]
        if tangent is not None:
            arrays.append(("tangent", tangent))
        arrays += [(f"history_prev['{n_}']", h) for (n_, _), h in zip(self._hist, hist_prev)]
        arrays += [(f"history['{n_}']", h) for (n_, _), h in zip(self._hist, hist)]
        dev = grad.device.index or 0
        for label, a in arrays:
            _check_torch(label, a)
            if (a.device.index or 0) != dev:
                raise ValueError(f"{label} is on {a.device}, grad_del_u on cuda:{dev}")
            if a.data_ptr() % 16:
                raise ValueError(f"{label}: device arrays must be 16-byte aligned")
        return dev

    def _evaluate_device(self, t, del_t, n, grad, stress_prev, stress, tangent, hist_prev, hist) -> None:
        dev = self._check_device_arrays(grad, stress_prev, stress, tangent, hist_prev, hist)
        self._check_field_points(n)  # the kernel reads n values of every field
        self._empty[dev] = n == 0
        if n == 0:  # nothing is launched (device_stats: 0)
            return
        counter = self._counter(dev)
        counter.zero_()  # on torch's current stream: the launch's stream
        a = self._args_cls()
        a.grad, a.stress_in, a.stress_out = grad.data_ptr(), stress_prev.data_ptr(), stress.data_ptr()
        a.tangent = None if tangent is None else tangent.data_ptr()
        for k, (hp, h) in enumerate(zip(hist_prev, hist)):
            a.h_in[k], a.h_out[k] = hp.data_ptr(), h.data_ptr()
        a.nonconv = counter.data_ptr()
        a.n, a.t, a.del_t, a.factor = n, float(t), float(del_t), FACTOR_PY
        for k, v in enumerate(self._param_values):
            a.params[k] = v
        if self._newton is not None:  # FCAMD_USER_IM_SLOT: behind the law's own parameters
            a.params[len(self._param_values)] = float(self._newton["max_iter"])
            a.params[len(self._param_values) + 1] = self._newton["tol"]
        for k, ptr in enumerate(self._field_ptrs(dev) if self._field_values else ()):
            a.fields[k] = ptr
        blocks = min(((n + 63) // 64 + 3) // 4, 512 * jit.num_cu(dev))  # a wave per 64-point tile, 4 waves per block
        jit.launch(self._compiled if tangent is not None else self._compiled_stress, dev, blocks, a, f"UserLaw '{self.name}' launch")

    # -- evaluate_path ----------------------------------------------------------------------------------------------------
    def _path_kernel(self, stress_controlled: tuple):
        """(code object, rung) of the path kernel for the control set, compiled on first use: the first rung of its ladder
        without scratch (explicit and autodiff laws: ``PATH_WAVES_PER_SIMD``; implicit laws: ``implicit_ladder``'s stress-only
        rungs)"""
        hit = self._path_compiled.get(stress_controlled)
        if hit is not None:
            return hit
        if self._rotate is not None:
            self._refuse("evaluate_path with an objective rate (a Mandel load path has no spin)")
        if self.tangent_mode == "implicit":
            if stress_controlled:
                raise NotImplementedError(f"UserLaw '{self.name}': evaluate_path with stress_controlled={stress_controlled} on an implicit "
                                          "law: implicit laws are driven under strain control only (their in-register tangent is "
                                          "not formed by the path kernel); use the law's explicit or autodiff form")
            rungs = implicit_ladder(self._unknowns, False, 2 * (6 + sum(d for _, d in self._hist)))
        else:
            rungs = tuple((w,) for w in PATH_WAVES_PER_SIMD)
        for rung in rungs:
            code = jit.compile_program(self._program_path(self.source, rung[0], stress_controlled, *rung[1:]), self.name, PATH_KERNEL)
            if not code.resources.get("scratch_bytes"):
                break
        if code.resources.get("scratch_bytes"):
            warnings.warn(f"UserLaw '{self.name}': the path kernel uses {code.resources['scratch_bytes']} bytes of scratch per lane "
                          f"(VGPRs: {code.resources.get('vgprs')}); register spills cost memory bandwidth", UserWarning, stacklevel=3)
        hit = self._path_compiled[stress_controlled] = (code, rung)
        return hit

    def path_resources(self, stress_controlled=()) -> dict:
        """``resources`` of the path kernel for ``stress_controlled`` (compiled on first use; no GPU needed), with
        ``"rung_waves_per_simd"``, the budget the kernel was cut for"""
        code, rung = self._path_kernel(_control_set(stress_controlled))
        r = dict(code.resources, rung_waves_per_simd=rung[0])
        if len(rung) > 1:
            r["jacobian_directions_per_pass"] = rung[1]
        return r

    def evaluate_path(self, t0, del_t, load, stress, history, *, stress_controlled=(), stress_path=None, strain_path=None,
                      newton=None, check: bool = False):
        """Drive every point through a load path of ``S = len(del_t)`` increments in one launch; returns the int32 array (or
        tensor) ``[n]`` of the first step each point failed, -1 for a point that completed.

        ``del_t``: float64 ``[S]`` (an ndarray, or a ROCm tensor, which is used where it lies); step k runs at ``t_k``
        (``t_0 = t0``, ``t_{k+1} = t_k + del_t[k]``, summed in this order in double) with ``del_t[k]``.
        ``load``: float64 ``[S, 6]`` (one path for all points) or ``[S, n, 6]``, Mandel components: the strain increment of the step for a component not in ``stress_controlled``, the total stress the step must reach for one
        in it.  ``stress_controlled``: distinct component indices 0-5, the same for all steps and points.  ``stress`` ``[6 n]`` and
        ``history``: the committed state, updated in place to the state after the last step a point completed.

        ``stress_path``, ``strain_path``: optional float64 ``[S, n, 6]`` records, step-major: the stress after each step and the
        Mandel strain increment each step applied (prescribed and solved components).  A point fails at a step when the point
        function returns non-zero at the step's last evaluation or the control Newton loop (``newton``: ``{"max_iter", "tol"}``,
        default 25 and 1e-10; converged when ``max_c |sigma_c - target_c| <= tol``) does not converge: it keeps its committed
        state, its records are NaN from that step on and it takes no further part.  ``check=True`` synchronises and raises the
        reference's non-convergence ``RuntimeError`` if a point failed, after everything is written.

        Device tensors: asynchronous on torch's current stream.  NumPy arrays: staged through device copies, synchronous.
        Implicit laws: strain control only (``NotImplementedError`` otherwise).  The algorithm: DESIGN.md §17."""
        self._refuse_batched()
        if self._rotate is not None:
            self._refuse("evaluate_path with an objective rate (a Mandel load path has no spin)")
        ctrl = _control_set(stress_controlled)
        opts = _newton_options(newton, PATH_NEWTON_DEFAULTS)
        hist = self._history_arrays(history)
        S, dts_dev, dts = _path_del_t(del_t)
        if _size(stress) % 6:
            raise ValueError(f"stress has {_size(stress)} entries, not a multiple of 6")
        n = _size(stress) // 6
        for (name, dim), h in zip(self._hist, hist):
            assert _size(h) == n * dim, f"history '{name}' has the wrong length"
        shape = tuple(load.shape) if hasattr(load, "shape") else None
        if shape not in ((S, 6), (S, n, 6)):
            raise ValueError(f"load has shape {shape}; expected ({S}, 6) (one path for all points) or ({S}, {n}, 6)")
        per_point = len(shape) == 3
        for label, rec in (("stress_path", stress_path), ("strain_path", strain_path)):
            if rec is not None and _size(rec) != S * n * 6:
                raise ValueError(f"{label} has {_size(rec)} entries; expected {S} x {n} x 6")
        self._check_field_points(n)
        arrays = [("load", load), ("stress", stress)] + [(f"history['{n_}']", h) for (n_, _), h in zip(self._hist, hist)]
        arrays += [(label, rec) for label, rec in (("stress_path", stress_path), ("strain_path", strain_path)) if rec is not None]
        code, _ = self._path_kernel(ctrl)  # an implicit law under stress control is refused here, before any device work
        t0 = float(t0)
        from .hostio import download, to_device, to_host

        if _is_torch(stress):
            dev = stress.device.index or 0
            if dts_dev is not None and (dts_dev.device.index or 0) != dev:
                raise ValueError(f"del_t is on {dts_dev.device}, stress on cuda:{dev}")
            for label, a in arrays:
                _check_torch(label, a)
                if (a.device.index or 0) != dev:
                    raise ValueError(f"{label} is on {a.device}, stress on cuda:{dev}")
                if a.data_ptr() % 16:
                    raise ValueError(f"{label}: device arrays must be 16-byte aligned")
            if dts_dev is None and S and n:
                import torch

                # a small pageable copy on torch's current stream (above 1 MiB: hostio's page-locked one, which waits for the stream)
                dts_dev = torch.from_numpy(dts).to(stress.device) if dts.nbytes < (1 << 20) else to_device(dts, stress.device)
            failed = self._path_device(code, dev, t0, S, dts_dev, n, per_point, load, stress, hist, stress_path, strain_path, opts)
            if check:
                self._raise(int((failed >= 0).sum().item()))
            return failed
        import torch

        for label, a in arrays:
            _check_numpy(label, a)
        if S == 0 or n == 0:
            return np.full(n, -1, dtype=np.int32)
        dev = _capi.default_device()
        d = torch.device("cuda", dev)
        with torch.cuda.device(d):
            s = to_device(stress.reshape(-1), d)
            hd = [to_device(h.reshape(-1), d) for h in hist]
            recs = [None if r is None else torch.empty(S * n * 6, dtype=torch.float64, device=d) for r in (stress_path, strain_path)]
            if dts_dev is None or (dts_dev.device.index or 0) != dev:
                dts_dev = to_device(to_host(dts_dev) if dts is None else dts, d)
            failed = self._path_device(code, dev, t0, S, dts_dev, n, per_point, to_device(load.reshape(-1), d), s, hd, recs[0], recs[1], opts)
            out = to_host(failed)
            download(stress.reshape(-1), s)
            for h, x in zip(hist, hd):
                download(h.reshape(-1), x)
            for r, x in zip((stress_path, strain_path), recs):
                if r is not None:
                    download(r.reshape(-1), x)
        if check:
            self._raise(int((out >= 0).sum()))
        return out

    def _path_device(self, code, dev, t0, S, del_t, n, per_point, load, stress, hist, stress_path, strain_path, opts):
        """the launch on checked device tensors (``del_t``: the [S] tensor of the increments); returns the int32 tensor of failed
        steps"""
        import torch

        with torch.cuda.device(dev):
            failed = torch.full((n,), -1, dtype=torch.int32, device=torch.device("cuda", dev))
        if S == 0 or n == 0:  # nothing is launched
            return failed
        a = self._path_args_cls()
        a.load, a.del_t, a.stress = load.data_ptr(), del_t.data_ptr(), stress.data_ptr()
        for k, h in enumerate(hist):
            a.h[k] = h.data_ptr()
        a.stress_path = None if stress_path is None else stress_path.data_ptr()
        a.strain_path = None if strain_path is None else strain_path.data_ptr()
        a.failed = failed.data_ptr()
        a.n, a.steps, a.per_point, a.max_iter = n, S, int(per_point), opts["max_iter"]
        a.t0, a.tol, a.factor, a.sq2 = t0, opts["tol"], FACTOR_PY, 2 ** 0.5
        for k, v in enumerate(self._param_values):
            a.params[k] = v
        if self._newton is not None:  # FCAMD_USER_IM_SLOT: behind the law's own parameters
            a.params[len(self._param_values)] = float(self._newton["max_iter"])
            a.params[len(self._param_values) + 1] = self._newton["tol"]
        for k, ptr in enumerate(self._field_ptrs(dev) if self._field_values else ()):
            a.fields[k] = ptr
        blocks = min(((n + 63) // 64 + 3) // 4, 512 * jit.num_cu(dev))  # a wave per 64-point tile, 4 waves per block
        jit.launch(code, dev, blocks, a, f"UserLaw '{self.name}' path launch")
        del_t.record_stream(torch.cuda.current_stream(dev))  # a copy made for this call is freed at return; the launch reads it
        return failed

    # -- the 1-D / 2-D wrappers ---------------------------------------------------------------------------------------------
    def _wrapped_kernel(self, wrap: int):
        """(code object, rung) of the wrapped kernel for the wrap mode (1 uniaxial strain, 2 plane strain, 3 plane stress,
        4 uniaxial stress), compiled on first use: the first rung of ``WRAPPED_WAVES_PER_SIMD`` without scratch"""
        hit = self._wrapped_compiled.get(wrap)
        if hit is not None:
            return hit
        if wrap not in WRAP_MODES.values():
            raise ValueError(f"UserLaw: wrap mode {wrap!r}; expected one of {sorted(WRAP_MODES.values())}")
        if self.tangent_mode == "implicit":
            raise NotImplementedError(f"UserLaw '{self.name}': implicit laws have no fused wrapper kernel (their in-register tangent "
                                      "is a pass structure, not a function that returns partials); the wrappers take the generic path")
        if self._rotate is not None:
            self._refuse("the 1-D / 2-D wrappers with an objective rate")
        if self._field_names:
            self._refuse("the 1-D / 2-D wrappers with per-point parameter fields")
        for waves in WRAPPED_WAVES_PER_SIMD:
            code = jit.compile_program(self._program_wrapped(self.source, waves, wrap), self.name, WRAPPED_KERNEL)
            if not code.resources.get("scratch_bytes"):
                break
        if code.resources.get("scratch_bytes"):
            warnings.warn(f"UserLaw '{self.name}': the wrapped kernel (mode {wrap}) uses {code.resources['scratch_bytes']} bytes of "
                          f"scratch per lane (VGPRs: {code.resources.get('vgprs')}); register spills cost memory bandwidth",
                          UserWarning, stacklevel=3)
        hit = self._wrapped_compiled[wrap] = (code, (waves,))
        return hit

    def wrapped_resources(self, constraint) -> dict:
        """``resources`` of the kernel that runs this law under the wrapper of ``constraint`` (UNIAXIAL_STRAIN, PLANE_STRAIN,
        PLANE_STRESS or UNIAXIAL_STRESS; compiled on first use; no GPU needed), with ``"rung_waves_per_simd"``, the budget the
        kernel was cut for.  Implicit laws: ``NotImplementedError`` (the wrappers run them through the generic path)."""
        if constraint not in WRAP_MODES:
            raise ValueError(f"UserLaw: wrapped_resources({constraint!r}); expected one of {[c.name for c in WRAP_MODES]}")
        code, rung = self._wrapped_kernel(WRAP_MODES[constraint])
        return dict(code.resources, rung_waves_per_simd=rung[0])

    def _evaluate_wrapped(self, constraint, t, del_t, grad, stress, tangent, cache3d, history) -> None:
        """The launch of the wrappers (wrappers._From3D.evaluate) on device tensors, in place: the low-dimensional ``grad``,
        ``stress`` and ``tangent`` of ``constraint``, the wrapper's cached 3-D stress rows ``cache3d`` ``[6 n]`` and the law's
        history.  Asynchronous on torch's current stream; ``device_stats`` returns the number of failed points.  Everything is
        validated before anything is launched."""
        self._refuse_batched()
        if constraint not in WRAP_MODES:
            raise ValueError(f"UserLaw: constraint {constraint!r} has no wrapper; expected one of {[c.name for c in WRAP_MODES]}")
        wrap = WRAP_MODES[constraint]
        gd2, sd = constraint.geometric_dim ** 2, constraint.stress_strain_dim
        hist = self._history_arrays(history)
        arrays = [("grad_del_u", grad), ("stress", stress), ("tangent", tangent), ("stress_3d", cache3d)]
        arrays += [(f"history['{n_}']", h) for (n_, _), h in zip(self._hist, hist)]
        for label, a in arrays:
            _check_torch(label, a)
        dev = grad.device.index or 0
        for label, a in arrays:
            if (a.device.index or 0) != dev:
                raise ValueError(f"{label} is on {a.device}, grad_del_u on cuda:{dev}")
            if a.data_ptr() % 16:
                raise ValueError(f"{label}: device arrays must be 16-byte aligned")
        if _size(grad) % gd2:
            raise ValueError(f"grad_del_u has {_size(grad)} entries, not a multiple of {gd2} ({constraint.name})")
        n = _size(grad) // gd2
        if _size(stress) != sd * n or _size(tangent) != sd * sd * n:
            raise ValueError(f"{constraint.name} over {n} points: stress has {_size(stress)} entries (expected {sd * n}), tangent "
                             f"{_size(tangent)} (expected {sd * sd * n})")
        if _size(cache3d) != 6 * n:
            raise ValueError(f"stress_3d has {_size(cache3d)} entries; the cached 3-D stress of {n} points has {6 * n}")
        for (name, dim), h in zip(self._hist, hist):
            if _size(h) != n * dim:
                raise ValueError(f"history '{name}' has {_size(h)} entries; expected {n} x {dim}")
        code, _ = self._wrapped_kernel(wrap)  # an implicit law is refused here
        self._empty[dev] = n == 0
        if n == 0:  # nothing is launched (device_stats: 0)
            return
        counter = self._counter(dev)
        counter.zero_()  # on torch's current stream: the launch's stream
        a = self._wrapped_args_cls()
        a.grad, a.stress, a.tangent, a.cache3d = grad.data_ptr(), stress.data_ptr(), tangent.data_ptr(), cache3d.data_ptr()
        for k, h in enumerate(hist):
            a.h[k] = h.data_ptr()
        a.nonconv = counter.data_ptr()
        a.n, a.t, a.del_t, a.factor = n, float(t), float(del_t), FACTOR_PY
        for k, v in enumerate(self._param_values):
            a.params[k] = v
        blocks = min(((n + 63) // 64 + 3) // 4, 512 * jit.num_cu(dev))  # a wave per 64-point tile, 4 waves per block
        jit.launch(code, dev, blocks, a, f"UserLaw '{self.name}' wrapped launch ({constraint.name})")

    def device_stats(self, device: int = 0) -> int:
        """Synchronise with the last launch on ``device`` and return its number of non-converged points (does not raise)."""
        c = self._counters.get(device)
        if c is None or self._empty.get(device):
            return 0
        from .hostio import to_host

        return int(to_host(c)[0])


def _args_type(nh: int, nf: int = 0):
    """ctypes mirror of UserArgs (user_law_tile.h) for ``nh`` history slots and ``nf`` parameter fields (behind the other members)"""
    vp = C.c_void_p

    class UserArgs(C.Structure):
        _fields_ = [("grad", vp), ("stress_in", vp), ("stress_out", vp), ("tangent", vp), ("h_in", vp * nh), ("h_out", vp * nh),
                    ("nonconv", vp), ("n", C.c_int64), ("t", C.c_double), ("del_t", C.c_double), ("factor", C.c_double),
                    ("params", C.c_double * MAX_PARAMS)] + ([("fields", vp * nf)] if nf else [])

    return UserArgs


def _path_args_type(nh: int, nf: int = 0):
    """ctypes mirror of PathArgs (user_law_path.hip) for ``nh`` history slots and ``nf`` parameter fields (behind the other members)"""
    vp = C.c_void_p

    class PathArgs(C.Structure):
        _fields_ = [("load", vp), ("del_t", vp), ("stress", vp), ("h", vp * nh), ("stress_path", vp), ("strain_path", vp),
                    ("failed", vp), ("n", C.c_int64), ("steps", C.c_int64), ("per_point", C.c_int64), ("max_iter", C.c_int64),
                    ("t0", C.c_double), ("tol", C.c_double), ("factor", C.c_double), ("sq2", C.c_double), ("params", C.c_double * MAX_PARAMS)] \
            + ([("fields", vp * nf)] if nf else [])

    return PathArgs


def _wrapped_args_type(nh: int):
    """ctypes mirror of WrappedArgs (user_law_wrapped.hip) for ``nh`` history slots"""
    vp = C.c_void_p

    class WrappedArgs(C.Structure):
        _fields_ = [("grad", vp), ("stress", vp), ("tangent", vp), ("cache3d", vp), ("h", vp * nh), ("nonconv", vp), ("n", C.c_int64),
                    ("t", C.c_double), ("del_t", C.c_double), ("factor", C.c_double), ("params", C.c_double * MAX_PARAMS)]

    return WrappedArgs
