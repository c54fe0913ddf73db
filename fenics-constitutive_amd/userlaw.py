"""User-defined constitutive laws compiled at run time to HIP kernels for gfx950.

A ``UserLaw`` is one ``__device__`` point function in HIP C++, given as a Python string (the contract: ``csrc/jit/user_law_api.h``,
INTEGRATION.md "Custom laws").  The constructor generates the parameter and history structs from the law's dicts, compiles them
with the user's source and the kernel template ``csrc/jit/user_law.hip`` -- which does all the memory work with the built-in
kernels' tile code (``csrc/kernels/tile_io.h``) -- by hiprtc, and keeps the code object.  The first call on a device loads it
there (``hipModuleLoadData`` of the HIP runtime torch has mapped: the process keeps one runtime) and every call launches it
(``hipModuleLaunchKernel``) on torch's current stream.  Compiling needs no GPU: the arch is fixed.

With ``tangent="autodiff"`` the source defines a stress and history update templated on the scalar type, compiled inside
``csrc/jit/user_law_ad.hip``; the tangent comes from forward-mode automatic differentiation (``csrc/jit/user_law_ad.h``).

FULL constraint, scalar parameters, ``evaluate`` / ``evaluate_from``: the resident, batched, indexed and multi-GPU forms of the
built-in laws are refused with ``NotImplementedError``.
"""

from __future__ import annotations

import ctypes as C
import hashlib
import os
import re
import threading
import warnings

import numpy as np

from . import _capi
from .device import _check_numpy, _check_torch, _current_stream_ptr, _is_torch, _size
from .interfaces import IncrSmallStrainModel, StressStrainConstraint

__all__ = ["UserLaw", "UserLawCompileError", "compile_count"]

JIT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "jit")
KERNEL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "kernels")
ARCH = "gfx950"
OPTIONS = (f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage")
KERNEL = "fcamd_user_law_kernel"
MAX_PARAMS = 32  # UserArgs.params (user_law.hip: kMaxParams)
#: register budgets tried in turn (waves per SIMD: 128 / 168 / 256 VGPRs): the first without scratch is kept
WAVES_PER_SIMD = (4, 3, 2)
#: tangent kernels of autodiff laws: (waves per SIMD, directions per pass) tried in turn, the first without scratch is kept.  One
#: pass (K = 6) at any budget first: it writes the tangent as coalesced 16-byte chunks, while K < 6 writes every pass's columns
#: as 8-byte entries (SpringMaxwellModel: 2.09x the time of K = 6 at 3 instead of 2 waves); then the most waves
#: with the fewest passes
AD_LADDER = tuple((w, 6) for w in WAVES_PER_SIMD) + tuple((w, k) for w in WAVES_PER_SIMD for k in (3, 2, 1))
TANGENT_MODES = ("explicit", "autodiff")
MAX_HISTORY_DIM = 36  # doubles per point of one history field (user_law.hip: kUserMaxDim)
FACTOR_PY = float.fromhex("0x1.6a09e667f3bccp-1")  # the off-diagonal Mandel factor of the Python laws (fcamd_capi.cpp: kFactorPy)
NONCONVERGED_MESSAGE = _capi.status_string(_capi.ERR_NONCONVERGED)

# hiprtc compiles against these in-memory headers instead of the HIP runtime's: the device code needs neither
_STUB_HEADERS = {
    "hip/hip_runtime.h": "#pragma once\ntypedef int hipError_t;\ntypedef struct ihipStream_t* hipStream_t;\n",
    "stdint.h": "#pragma once\n",
}

_CXX_KEYWORDS = frozenset("""
alignas alignof and and_eq asm auto bitand bitor bool break case catch char char8_t char16_t char32_t class compl concept const
consteval constexpr constinit const_cast continue co_await co_return co_yield decltype default delete do double dynamic_cast else
enum explicit export extern false float for friend goto if inline int long mutable namespace new noexcept not not_eq nullptr
operator or or_eq private protected public register reinterpret_cast requires return short signed sizeof static static_assert
static_cast struct switch template this thread_local throw true try typedef typeid typename union unsigned using virtual void
volatile wchar_t while xor xor_eq restrict
""".split())
_IDENT = re.compile(r"[A-Za-z_][A-Za-z0-9_]*\Z")


class UserLawCompileError(ValueError):
    """The user's source does not compile; ``log`` is hiprtc's log."""

    def __init__(self, message: str, log: str = ""):
        super().__init__(message)
        self.log = log


# --------------------------------------------------------------------------------------------------------------------------
# hiprtc and the HIP module API, through ctypes
# --------------------------------------------------------------------------------------------------------------------------
_lock = threading.Lock()
_rtc = None
_hip = None
_cache: dict = {}  # sha256 key -> _Compiled
_compiles = 0


def compile_count() -> int:
    """number of hiprtc compilations this process has made (cache hits do not count)"""
    return _compiles


def _torch_lib_dir():
    import importlib.util

    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return None
    return os.path.join(list(spec.submodule_search_locations)[0], "lib")


def _load_rtc():
    """torch's bundled hiprtc (the same ROCm release as the runtime that loads the code), else the system one"""
    global _rtc
    if _rtc is not None:
        return _rtc
    candidates = []
    d = _torch_lib_dir()
    if d:
        candidates.append(os.path.join(d, "libhiprtc.so"))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    candidates += [os.path.join(rocm, "lib", "libhiprtc.so.7"), "libhiprtc.so.7"]
    err = None
    for path in candidates:
        if os.sep in path and not os.path.exists(path):
            continue
        try:
            lib = C.CDLL(path)
            break
        except OSError as e:
            err = e
    else:
        raise RuntimeError(f"hiprtc (libhiprtc.so.7) not found: {err}")
    vp, sz = C.c_void_p, C.c_size_t
    lib.hiprtcCreateProgram.argtypes = [C.POINTER(vp), C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    lib.hiprtcCompileProgram.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p)]
    lib.hiprtcGetProgramLogSize.argtypes = [vp, C.POINTER(sz)]
    lib.hiprtcGetProgramLog.argtypes = [vp, C.c_char_p]
    lib.hiprtcGetCodeSize.argtypes = [vp, C.POINTER(sz)]
    lib.hiprtcGetCode.argtypes = [vp, C.c_char_p]
    lib.hiprtcDestroyProgram.argtypes = [C.POINTER(vp)]
    lib.hiprtcVersion.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.hiprtcGetErrorString.argtypes = [C.c_int]
    lib.hiprtcGetErrorString.restype = C.c_char_p
    _rtc = lib
    return lib


def _rtc_version() -> str:
    lib = _load_rtc()
    major, minor = C.c_int(), C.c_int()
    lib.hiprtcVersion(C.byref(major), C.byref(minor))
    return f"{major.value}.{minor.value}"


def _load_hip():
    """the HIP runtime already mapped into the process (torch's copy, which libfcamd shares): a second runtime would see no
    device"""
    global _hip
    if _hip is not None:
        return _hip
    _capi.load()  # imports torch first, then maps libfcamd onto torch's runtime
    path = "libamdhip64.so.7"
    try:
        with open("/proc/self/maps") as fh:
            for line in fh:
                if "libamdhip64.so" in line and "/" in line:
                    path = line[line.index("/"):].strip()
                    break
    except OSError:
        pass
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.hipModuleLoadData.argtypes = [C.POINTER(vp), vp]
    lib.hipModuleGetFunction.argtypes = [C.POINTER(vp), vp, C.c_char_p]
    lib.hipModuleLaunchKernel.argtypes = [vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, vp,
                                          C.POINTER(vp), C.POINTER(vp)]
    lib.hipGetErrorString.argtypes = [C.c_int]
    lib.hipGetErrorString.restype = C.c_char_p
    _hip = lib
    return lib


def _hip_check(status: int, what: str) -> None:
    if status != 0:
        raise RuntimeError(f"{what}: {_load_hip().hipGetErrorString(status).decode()} ({status})")


def _read(path: str) -> str:
    with open(path) as fh:
        return fh.read()


def parse_resources(log: str) -> dict:
    """``{"vgprs", "sgprs", "scratch_bytes", "waves_per_simd"}`` of the kernel from the compiler's kernel-resource-usage remarks"""
    keys = {"vgprs": r"\bVGPRs:\s*(\d+)", "sgprs": r"SGPRs:\s*(\d+)", "scratch_bytes": r"ScratchSize \[bytes/lane\]:\s*(\d+)",
            "waves_per_simd": r"Occupancy \[waves/SIMD\]:\s*(\d+)", "agprs": r"\bAGPRs:\s*(\d+)", "lds_bytes": r"LDS Size \[bytes/block\]:\s*(\d+)"}
    out = {}
    for k, pat in keys.items():
        m = re.search(pat, log)
        out[k] = int(m.group(1)) if m else None
    return out


class _Compiled:
    """one code object and its modules (one per device)"""

    def __init__(self, code: bytes, log: str, key: str = "", kernel: str = KERNEL):
        self.code = code
        self.log = log
        self.key = key  # the compile cache key
        self.kernel = kernel
        self.resources = parse_resources(log)
        self._functions = {}  # device -> (module, function)
        self._lock = threading.Lock()

    def function(self, device: int):
        with self._lock:
            f = self._functions.get(device)
            if f is None:
                import torch

                hip = _load_hip()
                module, fn = C.c_void_p(), C.c_void_p()
                with torch.cuda.device(device):
                    _hip_check(hip.hipModuleLoadData(C.byref(module), C.c_char_p(self.code)), "hipModuleLoadData")
                    _hip_check(hip.hipModuleGetFunction(C.byref(fn), module, self.kernel.encode()), "hipModuleGetFunction")
                f = self._functions[device] = (module, fn)
            return f[1]


# the objective-rate hook of the autodiff template (rotation.h); a program that does not define FCAMD_USER_ROTATE never sees it
_ROTATE_HOOK = re.compile(r"#ifdef FCAMD_USER_ROTATE\n.*?#endif\n", re.S)


def _key_text(path: str, program: str) -> str:
    """the text of an included file as the cache key counts it: without the rotation hook when the program has no rotation,
    so that the keys of unrotated laws stay what they were before the hook existed"""
    text = _read(path)
    return text if "FCAMD_USER_ROTATE" in program else _ROTATE_HOOK.sub("", text)


def _compile(program: str, name: str, extra=(), kernel: str = KERNEL) -> _Compiled:
    """hiprtc, cached in process by the sha256 of everything the code object depends on (and on disk in ``FCAMD_JIT_CACHE``).
    ``extra``: further files of ``JIT_DIR`` the program includes (the autodiff template and header, rotation.h).  ``kernel``:
    the name of the program's kernel."""
    global _compiles
    template, api, tile_io = (_read(os.path.join(JIT_DIR, "user_law.hip")), _read(os.path.join(JIT_DIR, "user_law_api.h")),
                              _read(os.path.join(KERNEL_DIR, "tile_io.h")))
    h = hashlib.sha256()
    for part in (template, api, tile_io, *[_key_text(os.path.join(JIT_DIR, f), program) for f in extra], program, " ".join(OPTIONS),
                 _rtc_version()):
        h.update(part.encode() + b"\0")
    key = h.hexdigest()
    with _lock:
        hit = _cache.get(key)
        if hit is not None:
            return hit
        disk = os.environ.get("FCAMD_JIT_CACHE")
        if disk:
            try:
                with open(os.path.join(disk, key + ".co"), "rb") as fh:
                    code = fh.read()
                hit = _cache[key] = _Compiled(code, _read(os.path.join(disk, key + ".log")), key, kernel)
                return hit
            except OSError:
                pass
        lib = _load_rtc()
        names = list(_STUB_HEADERS)
        hdr = (C.c_char_p * len(names))(*[_STUB_HEADERS[n].encode() for n in names])
        inc = (C.c_char_p * len(names))(*[n.encode() for n in names])
        prog = C.c_void_p()
        st = lib.hiprtcCreateProgram(C.byref(prog), program.encode(), b"fcamd_user_law_program.hip", len(names), hdr, inc)
        if st != 0:
            raise RuntimeError(f"hiprtcCreateProgram: {lib.hiprtcGetErrorString(st).decode()}")
        try:
            opts = [*OPTIONS, f"-I{KERNEL_DIR}", f"-I{JIT_DIR}"]
            st = lib.hiprtcCompileProgram(prog, len(opts), (C.c_char_p * len(opts))(*[o.encode() for o in opts]))
            n = C.c_size_t()
            lib.hiprtcGetProgramLogSize(prog, C.byref(n))
            buf = C.create_string_buffer(max(n.value, 1))
            lib.hiprtcGetProgramLog(prog, buf)
            log = buf.value.decode(errors="replace")
            _compiles += 1
            if st != 0:
                raise UserLawCompileError(f"UserLaw '{name}' does not compile ({lib.hiprtcGetErrorString(st).decode()}):\n{log}", log)
            lib.hiprtcGetCodeSize(prog, C.byref(n))
            code = C.create_string_buffer(n.value)
            lib.hiprtcGetCode(prog, code)
            code = code.raw
        finally:
            lib.hiprtcDestroyProgram(C.byref(prog))
        if disk:
            try:
                os.makedirs(disk, exist_ok=True)
                for ext, data in ((".co", code), (".log", log.encode())):
                    tmp = os.path.join(disk, f"{key}{ext}.{os.getpid()}")
                    with open(tmp, "wb") as fh:
                        fh.write(data)
                    os.replace(tmp, os.path.join(disk, key + ext))
            except OSError:
                pass
        hit = _cache[key] = _Compiled(code, log, key, kernel)
        return hit


# --------------------------------------------------------------------------------------------------------------------------
# the law
# --------------------------------------------------------------------------------------------------------------------------
_AD_FILES = ("user_law_ad.h", "user_law_ad.hip")
_ROTATION_FILES = ("rotation.h",)


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


def _dim_value(name, dim) -> int:
    if isinstance(dim, tuple):
        d = int(np.prod([int(x) for x in dim])) if dim else 0
    else:
        d = int(dim)
    if d < 1 or d > MAX_HISTORY_DIM:
        raise ValueError(f"UserLaw: history field '{name}' has {d} doubles per point; 1 to {MAX_HISTORY_DIM} are supported")
    return d


def _refuse(what: str):
    raise NotImplementedError(f"UserLaw: {what} is not supported for user-defined laws")


def refuse_user_law(law, what: str) -> None:
    """the forms of the built-in laws that user laws and objective-rate wrappers do not have (resident and multi-GPU states)"""
    if isinstance(law, UserLaw):
        _refuse(what)
    from .objective import JaumannRate

    if isinstance(law, JaumannRate):
        JaumannRate._refuse(what)


class UserLaw(IncrSmallStrainModel):
    """A constitutive law written by the user as one HIP C++ point function (``source``; contract in
    ``csrc/jit/user_law_api.h``), compiled at construction for gfx950.

    ``parameters``: name -> scalar float, at most 32; the values are kernel arguments, so laws that differ only in them share
    one code object.  ``history_dim``: name -> doubles per point (an int or a tuple, whose product counts), or None.  The
    names are C identifiers, not C++ keywords, and do not repeat.  FULL constraint only.

    ``tangent``: ``"explicit"`` (the source defines ``fcamd_user_point``, which writes the tangent itself) or ``"autodiff"`` (the
    source defines the function template ``fcamd_user_stress<T>``, stress and history only; the tangent comes from forward-mode
    automatic differentiation, contract in ``csrc/jit/user_law_ad.h``)."""

    def __init__(self, source: str, parameters=None, history_dim=None, constraint: StressStrainConstraint = None,
                 name: str = "user_law", tangent: str = "explicit", *, _rotate=None):
        if not isinstance(tangent, str) or tangent not in TANGENT_MODES:
            raise ValueError(f"UserLaw: tangent={tangent!r}; expected one of {TANGENT_MODES}")
        self.tangent_mode = tangent
        constraint = StressStrainConstraint.FULL if constraint is None else constraint
        if constraint != StressStrainConstraint.FULL:
            raise NotImplementedError(f"UserLaw: constraint {constraint.name}: user laws are FULL (3-D) only; wrap one in "
                                      "UniaxialStrainFrom3D / PlaneStrainFrom3D for lower dimensions")
        self._constraint = constraint
        self.name = str(name)
        params = _items(parameters)
        hist = _items(history_dim)
        seen = set()
        for what, pairs in (("parameter", params), ("history", hist)):
            for n, _ in pairs:
                _check_name(n, what)
                if n in seen:
                    raise ValueError(f"UserLaw: name '{n}' is given more than once")
                seen.add(n)
        if len(params) > MAX_PARAMS:
            raise ValueError(f"UserLaw: {len(params)} parameters; at most {MAX_PARAMS}")
        self._param_names = tuple(n for n, _ in params)
        self._param_values = [_param_value(n, v) for n, v in params]
        self._history_dim = history_dim
        self._hist = [(n, _dim_value(n, d)) for n, d in hist]
        self.source = source
        # objective.JaumannRate: ((history field, offset), ...) of the Mandel blocks rotated with the stress before the law runs
        self._rotate = None if _rotate is None else tuple((str(f), int(o)) for f, o in _rotate)
        rot_files = () if self._rotate is None else _ROTATION_FILES
        self._directions = None
        if tangent == "explicit":
            # cut for 4 waves per SIMD (128 VGPRs; the LDS allows no more); a law that spills there is compiled again for fewer waves
            for waves in WAVES_PER_SIMD:
                self._compiled = _compile(self._program(source, waves), self.name, rot_files)
                if not self._compiled.resources.get("scratch_bytes"):
                    break
            self._compiled_stress = self._compiled
        else:
            # two code objects: the stress-only kernel (T = double) for tangent=None launches, the tangent kernel (Dual<K>)
            for waves in WAVES_PER_SIMD:
                self._compiled_stress = _compile(self._program_ad(source, waves, 0), self.name, _AD_FILES + rot_files)
                if not self._compiled_stress.resources.get("scratch_bytes"):
                    break
            for waves, k in AD_LADDER:
                self._compiled = _compile(self._program_ad(source, waves, k), self.name, _AD_FILES + rot_files)
                self._directions = k
                if not self._compiled.resources.get("scratch_bytes"):
                    break
        for c in {id(self._compiled): self._compiled, id(self._compiled_stress): self._compiled_stress}.values():
            if c.resources.get("scratch_bytes"):
                warnings.warn(f"UserLaw '{self.name}': the kernel uses {c.resources['scratch_bytes']} bytes of scratch per lane "
                              f"(VGPRs: {c.resources.get('vgprs')}); register spills cost memory bandwidth", UserWarning, stacklevel=2)
        self._counters = {}  # device -> int64 device word (non-converged points of the last launch)
        self._empty = {}  # device -> the last call had no points
        self._args_cls = _args_type(max(1, len(self._hist)))

    # -- program --------------------------------------------------------------------------------------------------------
    def _rotation_lines(self) -> list:
        """the generated block list and rotation.h (a law with ``_rotate``; none otherwise)"""
        if self._rotate is None:
            return []
        return ["#define FCAMD_USER_ROTATE(X) " + " ".join(f"X({f}, {o})" for f, o in self._rotate), '#include "rotation.h"']

    def _program(self, source: str, waves: int) -> str:
        """the generated definitions, the user's source, the template.  A rotated law renames the user's point function and
        calls it from a generated one that first rotates the committed state (its gradient is an argument already)"""
        p = self._param_names
        lines = ['#include "user_law_api.h"',
                 f"#define FCAMD_USER_WAVES {waves}",
                 f"#define FCAMD_USER_NHIST {len(self._hist)}",
                 "#define FCAMD_USER_HISTORY_FIELDS(X) " + " ".join(f"X({k}, {n}, {d})" for k, (n, d) in enumerate(self._hist)),
                 "struct UserParams {" + "".join(f" double {n};" for n in p) + " };",
                 "struct UserHistory {" + "".join(f" double {n}[{d}];" for n, d in self._hist) + " };",
                 "__device__ __forceinline__ UserParams fcamd_user_params(const double* v) {",
                 "    UserParams p;" + "".join(f" p.{n} = v[{k}];" for k, n in enumerate(p)),
                 "    return p;",
                 "}",
                 '#line 1 "' + re.sub(r'[^A-Za-z0-9_.]', '_', self.name) + '"']
        if self._rotate is None:
            return "\n".join(lines) + "\n" + source + '\n#include "user_law.hip"\n'
        lines[-1:-1] = self._rotation_lines() + ["#define fcamd_user_point fcamd_user_point_unrotated"]
        return "\n".join(lines) + "\n" + source + "\n" + _ROTATED_POINT + '#include "user_law.hip"\n'

    def _program_ad(self, source: str, waves: int, directions: int) -> str:
        """autodiff mode: the generated definitions, the user's template, the autodiff kernel template (``directions``: partials
        per Dual, 0 for the stress-only kernel)"""
        p = self._param_names
        lines = ['#include "user_law_ad.h"',
                 f"#define FCAMD_USER_WAVES {waves}",
                 f"#define FCAMD_USER_AD_K {directions}",
                 f"#define FCAMD_USER_NHIST {len(self._hist)}",
                 "#define FCAMD_USER_HISTORY_FIELDS(X) " + " ".join(f"X({k}, {n}, {d})" for k, (n, d) in enumerate(self._hist)),
                 "struct UserParams {" + "".join(f" double {n};" for n in p) + " };",
                 "template <class T> struct UserHistoryT {" + "".join(f" T {n}[{d}];" for n, d in self._hist) + " };",
                 "__device__ __forceinline__ UserParams fcamd_user_params(const double* v) {",
                 "    UserParams p;" + "".join(f" p.{n} = v[{k}];" for k, n in enumerate(p)),
                 "    return p;",
                 "}",
                 '#line 1 "' + re.sub(r'[^A-Za-z0-9_.]', '_', self.name) + '"']
        lines[-1:-1] = self._rotation_lines()  # (user_law_ad.hip calls fcamd_user_rotate when FCAMD_USER_ROTATE is defined)
        return "\n".join(lines) + "\n" + source + '\n#include "user_law_ad.hip"\n'

    @property
    def resources(self) -> dict:
        """``{"vgprs", "sgprs", "scratch_bytes", "waves_per_simd", ...}`` of the compiled kernel (compiler remarks).  Autodiff
        laws: those of the tangent kernel, its ``"directions_per_pass"`` (K of Dual<K>; ceil(6 / K) passes) and under
        ``"stress_only"`` those of the kernel of tangent=None launches."""
        r = dict(self._compiled.resources)
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
        return dict(zip(self._param_names, self._param_values))

    def update(self) -> None:
        pass

    # -- refused forms ----------------------------------------------------------------------------------------------------
    def use_devices(self, devices):
        _refuse("use_devices (several GPUs in one process)")

    def evaluate_indexed(self, *args, **kwargs):
        _refuse("evaluate_indexed (parent rows)")

    @staticmethod
    def _refuse_batched():
        if getattr(_capi._tls, "batch", None) is not None:
            _refuse("a call inside batched_launches()")

    # -- evaluate ---------------------------------------------------------------------------------------------------------
    def _history_arrays(self, history):
        if not self._hist:
            return []
        if history is None:
            raise ValueError("history must not be None")
        return [history[n] for n, _ in self._hist]

    def _sizes(self, grad, stress, tangent, hist, stress_prev=None, hist_prev=None) -> int:
        n = _size(grad) // 9
        # DeviceLaw.evaluate's checks and messages (the reference's: linear_elasticity_model.py:36-40)
        assert n == _size(stress) // 6 and (tangent is None or n == _size(tangent) // 36), "Stress, strain, and tangent lengths do not match"
        assert _size(grad) == n * 9 and _size(stress) == n * 6, "Input arrays are not of the correct length"
        if stress_prev is not None:
            assert _size(stress_prev) == n * 6, "Stress, strain, and tangent lengths do not match"
        for (name, dim), h in zip(self._hist, hist):
            assert _size(h) == n * dim, f"history '{name}' has the wrong length"
        for (name, dim), h in zip(self._hist, hist_prev or []):
            assert _size(h) == n * dim, f"history '{name}' has the wrong length"
        return n

    def evaluate(self, t, del_t, grad_del_u, stress, tangent, history, check: bool = False) -> None:
        """``IncrSmallStrainModel.evaluate``: overwrite ``stress``, ``tangent`` (unless None) and every history array in place.
        NumPy arrays: synchronous; raises the reference's ``RuntimeError`` if a point did not converge (after the results are
        written).  Device tensors: asynchronous on torch's current stream; ``check=True`` synchronises and raises the same
        error, otherwise ``device_stats()`` returns the count."""
        self._refuse_batched()
        hist = self._history_arrays(history)
        n = self._sizes(grad_del_u, stress, tangent, hist)
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
        if not _is_torch(grad_del_u):
            raise TypeError("UserLaw.evaluate_from takes device tensors (use evaluate for NumPy arrays)")
        self._evaluate_device(t, del_t, n, grad_del_u, stress_prev, stress, tangent, hprev, hist)

    @staticmethod
    def _raise(count: int) -> None:
        if count:
            raise RuntimeError(NONCONVERGED_MESSAGE)

    def _evaluate_host(self, t, del_t, n, grad, stress, tangent, hist) -> None:
        """NumPy arrays: staged through device buffers (hostio.upload / download), the kernel, back in place"""
        import torch

        from .hostio import download, to_device

        _check_numpy("grad_del_u", grad)
        _check_numpy("stress", stress)
        if tangent is not None:
            _check_numpy("tangent", tangent)
        for (name, _), h in zip(self._hist, hist):
            _check_numpy(f"history['{name}']", h)
        if n == 0:
            return
        dev = _capi.default_device()
        d = torch.device("cuda", dev)
        with torch.cuda.device(d):
            g = to_device(grad.reshape(-1), d)
            s = to_device(stress.reshape(-1), d)
            tan = None if tangent is None else torch.empty(36 * n, dtype=torch.float64, device=d)
            hd = [to_device(h.reshape(-1), d) for h in hist]
            self._evaluate_device(t, del_t, n, g, s, s, tan, hd, hd)
            download(stress.reshape(-1), s)
            if tangent is not None:
                download(tangent.reshape(-1), tan)
            for h, x in zip(hist, hd):
                download(h.reshape(-1), x)
            self._raise(self.device_stats(dev))

    def _counter(self, device: int):
        c = self._counters.get(device)
        if c is None:
            import torch

            c = self._counters[device] = torch.zeros(1, dtype=torch.int64, device=torch.device("cuda", device))
        return c

    def _evaluate_device(self, t, del_t, n, grad, stress_prev, stress, tangent, hist_prev, hist) -> None:
        import torch

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
        self._empty[dev] = n == 0
        if n == 0:  # nothing is launched (device_stats: 0)
            return
        counter = self._counter(dev)
        counter.zero_()  # on torch's current stream: the launch's stream
        fn = (self._compiled if tangent is not None else self._compiled_stress).function(dev)
        a = self._args_cls()
        a.grad, a.stress_in, a.stress_out = grad.data_ptr(), stress_prev.data_ptr(), stress.data_ptr()
        a.tangent = None if tangent is None else tangent.data_ptr()
        for k, (hp, h) in enumerate(zip(hist_prev, hist)):
            a.h_in[k], a.h_out[k] = hp.data_ptr(), h.data_ptr()
        a.nonconv = counter.data_ptr()
        a.n, a.t, a.del_t, a.factor = n, float(t), float(del_t), FACTOR_PY
        for k, v in enumerate(self._param_values):
            a.params[k] = v
        tiles = (n + 63) // 64
        blocks = min((tiles + 3) // 4, 512 * _num_cu(dev))
        params = (C.c_void_p * 1)(C.cast(C.pointer(a), C.c_void_p))
        hip = _load_hip()
        with torch.cuda.device(dev):
            _hip_check(hip.hipModuleLaunchKernel(fn, blocks, 1, 1, 256, 1, 1, 0, C.c_void_p(_current_stream_ptr(dev)), params, None),
                       f"UserLaw '{self.name}' launch")

    def device_stats(self, device: int = 0) -> int:
        """Synchronise with the last launch on ``device`` and return its number of non-converged points (does not raise)."""
        c = self._counters.get(device)
        if c is None or self._empty.get(device):
            return 0
        from .hostio import to_host

        return int(to_host(c)[0])


# the point function of a rotated explicit law: rotation.h's fcamd_user_rotate, then the user's (renamed) function
_ROTATED_POINT = """#undef fcamd_user_point
#line 1 "fcamd_objective_rate"
__device__ __forceinline__ int fcamd_user_point(const UserParams& p, double t, double del_t, const double (&grad)[9],
                                                const double (&eps)[6], double (&sigma)[6], double (&D)[36], UserHistory& h) {
    fcamd_user_rotate(grad, sigma, h);
    return fcamd_user_point_unrotated(p, t, del_t, grad, eps, sigma, D, h);
}
"""

_num_cu_cache: dict = {}


def _num_cu(device: int) -> int:
    n = _num_cu_cache.get(device)
    if n is None:
        import torch

        n = _num_cu_cache[device] = int(torch.cuda.get_device_properties(device).multi_processor_count)
    return n


def _args_type(nh: int):
    """ctypes mirror of UserArgs (user_law.hip) for ``nh`` history slots"""
    vp = C.c_void_p

    class UserArgs(C.Structure):
        _fields_ = [("grad", vp), ("stress_in", vp), ("stress_out", vp), ("tangent", vp), ("h_in", vp * nh), ("h_out", vp * nh),
                    ("nonconv", vp), ("n", C.c_int64), ("t", C.c_double), ("del_t", C.c_double), ("factor", C.c_double),
                    ("params", C.c_double * MAX_PARAMS)]

    return UserArgs
