"""Kernels compiled at run time: hiprtc, the compile cache, the code objects and their launches, through ctypes.  The only module
that calls hiprtc and the HIP module API; ``userlaw`` (UserLaw) and ``objective`` (JaumannRate) generate the programs, and
``JitLaw`` is the evaluate plumbing those two laws share.

A program is compiled for gfx950 (no GPU needed: the arch is fixed) against the headers of ``csrc/jit`` and ``csrc/kernels``.
The code object is cached in process and, with ``FCAMD_JIT_CACHE`` set, on disk, under the sha256 of the program, the options,
the hiprtc version and the text of every file the program includes (``include_closure``).  The first launch on a device loads
it there (``hipModuleLoadData`` of the HIP runtime torch has mapped: the process keeps one runtime) and every launch goes to
torch's current stream (``hipModuleLaunchKernel``).
"""

from __future__ import annotations

import ctypes as C
import hashlib
import os
import re
import threading

from . import _capi
from .device import _check_numpy, _current_stream_ptr, _size
from .interfaces import IncrSmallStrainModel

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
JIT_DIR = os.path.join(CSRC, "jit")
KERNEL_DIR = os.path.join(CSRC, "kernels")
#: where an include is looked for after the including file's own directory: the -I options, in order
INCLUDE_DIRS = (JIT_DIR, KERNEL_DIR)
ARCH = "gfx950"
OPTIONS = (f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage")
NONCONVERGED_MESSAGE = _capi.status_string(_capi.ERR_NONCONVERGED)

# hiprtc compiles against these in-memory headers instead of the HIP runtime's: the device code needs neither
_STUB_HEADERS = {
    "hip/hip_runtime.h": "#pragma once\ntypedef int hipError_t;\ntypedef struct ihipStream_t* hipStream_t;\n",
    "stdint.h": "#pragma once\n",
}
_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]*([<"])([^">\n]+)[">]', re.M)


class UserLawCompileError(ValueError):
    """The user's source does not compile; ``log`` is hiprtc's log."""

    def __init__(self, message: str, log: str = ""):
        super().__init__(message)
        self.log = log


_lock = threading.Lock()
_rtc = None
_hip = None
_cache: dict = {}  # sha256 key -> CodeObject
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


def rtc_version() -> str:
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


def hip_check(status: int, what: str) -> None:
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


class CodeObject:
    """one code object and its modules (one per device)"""

    def __init__(self, code: bytes, log: str, key: str, kernel: str):
        self.code = code
        self.log = log
        self.key = key  # the compile cache key
        self.kernel = kernel
        self.resources = parse_resources(log)
        self._modules = {}  # device -> module
        self._functions = {}  # (device, kernel) -> function
        self._lock = threading.Lock()

    def function(self, device: int, kernel: str | None = None):
        """the function of ``kernel`` (default: the code object's own) in the module loaded on ``device``"""
        kernel = kernel or self.kernel
        with self._lock:
            f = self._functions.get((device, kernel))
            if f is None:
                import torch

                hip = _load_hip()
                module = self._modules.get(device)
                fn = C.c_void_p()
                with torch.cuda.device(device):
                    if module is None:
                        module = C.c_void_p()
                        hip_check(hip.hipModuleLoadData(C.byref(module), C.c_char_p(self.code)), "hipModuleLoadData")
                        self._modules[device] = module
                    hip_check(hip.hipModuleGetFunction(C.byref(fn), module, kernel.encode()), "hipModuleGetFunction")
                f = self._functions[(device, kernel)] = fn
            return f


def include_closure(program: str) -> list:
    """the files the program includes, directly or through other files, in first-include order.  As hiprtc resolves them: a
    quoted name in the including file's directory first, then in INCLUDE_DIRS; a bracketed one in INCLUDE_DIRS only (the rest
    are the stub headers)"""
    found = []

    def visit(text, here):
        for kind, name in _INCLUDE.findall(text):
            for d in ((here,) if kind == '"' and here else ()) + INCLUDE_DIRS:
                path = os.path.normpath(os.path.join(d, name))
                if os.path.isfile(path):
                    if path not in found:
                        found.append(path)
                        visit(_read(path), os.path.dirname(path))
                    break

    visit(program, None)
    return found


def cache_key(program: str) -> str:
    """sha256 of everything the code object depends on: the program, the options, the hiprtc version, the stub headers and
    the text of every file of the program's include closure"""
    h = hashlib.sha256()
    for part in (program, " ".join(OPTIONS), rtc_version(), *_STUB_HEADERS.values(), *map(_read, include_closure(program))):
        h.update(part.encode() + b"\0")
    return h.hexdigest()


def compile_program(program: str, name: str, kernel: str) -> CodeObject:
    """hiprtc, cached in process by ``cache_key`` (and on disk in ``FCAMD_JIT_CACHE``).  ``name``: the law's, for the error;
    ``kernel``: the name of the program's kernel."""
    global _compiles
    key = cache_key(program)
    with _lock:
        hit = _cache.get(key)
        if hit is not None:
            return hit
        disk = os.environ.get("FCAMD_JIT_CACHE")
        if disk:
            try:
                with open(os.path.join(disk, key + ".co"), "rb") as fh:
                    code = fh.read()
                hit = _cache[key] = CodeObject(code, _read(os.path.join(disk, key + ".log")), key, kernel)
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
            opts = [*OPTIONS, *(f"-I{d}" for d in INCLUDE_DIRS)]
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
        hit = _cache[key] = CodeObject(code, log, key, kernel)
        return hit


_num_cu_cache: dict = {}


def num_cu(device: int) -> int:
    n = _num_cu_cache.get(device)
    if n is None:
        import torch

        n = _num_cu_cache[device] = int(torch.cuda.get_device_properties(device).multi_processor_count)
    return n


def launch(code: CodeObject, device: int, blocks: int, args, what: str, kernel: str | None = None) -> None:
    """``code``'s kernel (``kernel``: another kernel of the same program) over ``blocks`` blocks of 256 threads, the ctypes
    structure ``args`` its only parameter, on torch's current stream of ``device`` (asynchronous); ``what`` names the launch in an
    error"""
    import torch

    fn = code.function(device, kernel)
    params = (C.c_void_p * 1)(C.cast(C.pointer(args), C.c_void_p))
    with torch.cuda.device(device):
        hip_check(_load_hip().hipModuleLaunchKernel(fn, blocks, 1, 1, 256, 1, 1, 0, C.c_void_p(_current_stream_ptr(device)),
                                                    params, None), what)


class JitLaw(IncrSmallStrainModel):
    """What UserLaw and JaumannRate share: the forms they refuse, the history arrays and size checks of a call, and the NumPy
    path, which stages the arrays through device copies.  A subclass sets ``_hist`` ([(history name, doubles per point)], in
    the law's order) and defines ``_refuse(what)`` and ``_evaluate_device(t, del_t, n, grad, stress_prev, stress, tangent,
    hist_prev, hist)``, the call on device tensors."""

    def use_devices(self, devices):
        self._refuse("use_devices (several GPUs in one process)")

    def evaluate_indexed(self, *args, **kwargs):
        self._refuse("evaluate_indexed (parent rows)")

    def _refuse_batched(self) -> None:
        if getattr(_capi._tls, "batch", None) is not None:
            self._refuse("a call inside batched_launches()")

    def _history_arrays(self, history) -> list:
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

    @staticmethod
    def _raise(count: int) -> None:
        if count:
            raise RuntimeError(NONCONVERGED_MESSAGE)

    def _nonconverged(self, device: int) -> int:
        """the points of the last call on ``device`` that did not converge"""
        return self.device_stats(device)

    def _evaluate_host(self, t, del_t, n, grad, stress, tangent, hist) -> None:
        """NumPy arrays: staged through device copies (hostio.to_device / download), evaluated there in place, back in place;
        non-convergence raises the reference's RuntimeError after the results are written"""
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
            self._raise(self._nonconverged(dev))
