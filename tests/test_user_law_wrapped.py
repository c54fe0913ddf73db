"""The fused kernel of the 1-D / 2-D wrappers around a user law, without a GPU: every explicit and autodiff transcription compiles
its four wrapped kernels without scratch, what is part of the program and what is not, the ctypes mirror of the argument struct,
the branch the wrappers take per tangent mode, and the validation of a launch (all of it before anything is launched)."""

import ctypes
import os
import re

import numpy as np
import pytest

import material_point_cases as cases

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import _capi, jit, userlaw, wrappers
from fenics_constitutive_amd import userlaw_sources as S

C = fc.StressStrainConstraint
LE = {"E": 42.0, "nu": 0.3}
SWIFT = {"p_ka": 175000.0, "p_mu": 80769.0, "K": 2000.0, "eps0": 0.01, "m": 0.2}
WRAPS = {C.UNIAXIAL_STRAIN: 1, C.PLANE_STRAIN: 2, C.PLANE_STRESS: 3, C.UNIAXIAL_STRESS: 4}
WRAPPERS = {C.UNIAXIAL_STRAIN: fc.UniaxialStrainFrom3D, C.PLANE_STRAIN: fc.PlaneStrainFrom3D,
            C.PLANE_STRESS: fc.PlaneStressFrom3D, C.UNIAXIAL_STRESS: fc.UniaxialStressFrom3D}
LAWS = {
    "linear_elasticity": lambda: S.linear_elasticity(LE),
    "spring_maxwell": lambda: S.spring_maxwell(cases.SLS),
    "von_mises_3d": lambda: S.von_mises_3d(cases.VM),
    "linear_elasticity_ad": lambda: S.linear_elasticity_ad(LE),
    "spring_maxwell_ad": lambda: S.spring_maxwell_ad(cases.SLS),
    "von_mises_3d_ad": lambda: S.von_mises_3d_ad(cases.VM),
    "von_mises_swift_ad": lambda: S.von_mises_swift_ad(SWIFT),
}
IMPLICIT = {
    "von_mises_3d_implicit": lambda: S.von_mises_3d_implicit(cases.VM),
    "von_mises_swift_implicit": lambda: S.von_mises_swift_implicit(SWIFT),
}


# --- compilation ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LAWS))
def test_every_law_compiles_its_four_wrapped_kernels_without_scratch(name):
    law = LAWS[name]()
    for constraint in WRAPS:
        r = law.wrapped_resources(constraint)
        assert r["scratch_bytes"] == 0, (name, constraint, r)
        assert r["rung_waves_per_simd"] in userlaw.WRAPPED_WAVES_PER_SIMD and r["vgprs"] > 0
        assert r["waves_per_simd"] >= r["rung_waves_per_simd"]
        assert r["lds_bytes"] == 4 * 64 * 18 * 8  # the wave's region of the other user-law kernels


def test_wrapped_resources_takes_the_four_wrapper_constraints_only():
    law = LAWS["linear_elasticity"]()
    with pytest.raises(ValueError, match="wrapped_resources"):
        law.wrapped_resources(C.FULL)
    with pytest.raises(ValueError, match="wrapped_resources"):
        law.wrapped_resources(2)


def test_laws_that_differ_in_values_share_the_wrapped_code_object():
    a = S.von_mises_3d(cases.VM)
    for constraint in WRAPS:
        a.wrapped_resources(constraint)
    count = userlaw.compile_count()
    b = S.von_mises_3d(dict(cases.VM, p_y0=900.0))
    for constraint, wrap in WRAPS.items():
        b.wrapped_resources(constraint)
        assert b._wrapped_kernel(wrap)[0] is a._wrapped_kernel(wrap)[0]
    assert userlaw.compile_count() == count
    # cached on the law, and the wrap mode is part of the program
    assert a._wrapped_kernel(3) is a._wrapped_kernel(3)
    codes = {id(a._wrapped_kernel(w)[0]) for w in WRAPS.values()}
    assert len(codes) == 4
    assert a._wrapped_kernel(2)[0].kernel == "fcamd_user_law_wrapped_kernel"


def test_the_wrapped_program_names_its_template_and_wrap_mode():
    ad, ex = S.von_mises_3d_ad(cases.VM), S.von_mises_3d(cases.VM)
    for wrap in WRAPS.values():
        prog = ad._program_wrapped(ad.source, 2, wrap)
        assert f"#define FCAMD_USER_WRAP {wrap}" in prog and "#define FCAMD_USER_AD_K 0" in prog and "#define FCAMD_USER_WAVES 2" in prog
        assert prog.rstrip().endswith('#include "user_law_wrapped.hip"')
        assert os.path.join(jit.JIT_DIR, "user_law_wrapped.hip") in jit.include_closure(prog)
        prog = ex._program_wrapped(ex.source, 4, wrap)
        assert f"#define FCAMD_USER_WRAP {wrap}" in prog and "FCAMD_USER_AD_K" not in prog
    # the evaluate kernels' programs do not change
    assert "FCAMD_USER_WRAP" not in ex._program(ex.source, 4) and "FCAMD_USER_WRAP" not in ad._program_ad(ad.source, 4, 6)
    # the tile header leaves its own kernel entry out behind the define, the template brings one of its own
    tile = open(os.path.join(jit.JIT_DIR, "user_law_tile.h")).read()
    assert re.search(r"#if !defined\(FCAMD_USER_PATH\) && !defined\(FCAMD_USER_WRAP\)", tile)
    text = open(os.path.join(jit.JIT_DIR, "user_law_wrapped.hip")).read()
    assert text.count("__global__") == 1 and "fcamd_user_law_wrapped_kernel(" in text


# --- the argument struct -------------------------------------------------------------------------------------------------------

def _declared_members():
    """(type, name, array extent or None) of every member of WrappedArgs as user_law_wrapped.hip declares it"""
    text = open(os.path.join(jit.JIT_DIR, "user_law_wrapped.hip")).read()
    body = text[text.index("struct WrappedArgs {"):]
    body = body[:body.index("};")]
    out = []
    for line in body.splitlines()[1:]:
        line = line.split("//")[0].strip()
        if not line or line.startswith("#"):
            continue
        m = re.match(r"(.*?)(\w+(?:, \w+)*)(\[(\w+)\])?;$", line)
        ctype = m.group(1).strip()
        for name in m.group(2).split(", "):
            out.append((ctype, name, m.group(4)))
    return out


@pytest.mark.parametrize("nh", [1, 2, 3])
def test_ctypes_mirror_of_wrapped_args(nh):
    cls = userlaw._wrapped_args_type(nh)
    members = _declared_members()
    assert [m[1] for m in members] == [f[0] for f in cls._fields_]
    extents = {"kNH": nh, "kMaxParams": userlaw.MAX_PARAMS}
    offset = 0
    for (ctype, name, extent), field in zip(members, cls._fields_):
        width = 8 * (extents[extent] if extent else 1)  # pointers, long long and double: 8 bytes each
        assert "*" in ctype or ctype in ("long long", "double"), ctype
        assert getattr(cls, name).offset == offset and getattr(cls, name).size == width, name
        assert ("*" in ctype) == (field[1] is ctypes.c_void_p or getattr(field[1], "_type_", None) is ctypes.c_void_p), name
        assert (ctype == "double") == (field[1] is ctypes.c_double or getattr(field[1], "_type_", None) is ctypes.c_double), name
        offset += width
    assert ctypes.sizeof(cls) == offset == 8 * (4 + nh + 1 + 1 + 3 + 32)


def test_a_law_keeps_the_mirror_of_its_history_slots():
    assert ctypes.sizeof(S.linear_elasticity(LE)._wrapped_args_cls) == ctypes.sizeof(userlaw._wrapped_args_type(1))
    assert ctypes.sizeof(S.von_mises_3d(cases.VM)._wrapped_args_cls) == ctypes.sizeof(userlaw._wrapped_args_type(2))


# --- stand-ins for device tensors ------------------------------------------------------------------------------------------------

class _Device:
    def __init__(self, index):
        self.index = index

    def __eq__(self, other):
        return isinstance(other, _Device) and other.index == self.index

    def __repr__(self):
        return f"cuda:{self.index}"


class FakeTensor:
    """what a launch's validation reads of a ROCm tensor"""

    def __init__(self, numel, dtype=None, device=0, ptr=4096, contiguous=True, cuda=True):
        import torch

        self._numel, self.dtype, self.device, self._ptr = numel, torch.float64 if dtype is None else dtype, _Device(device), ptr
        self._contiguous, self.is_cuda, self.size = contiguous, cuda, numel

    def numel(self):
        return self._numel

    def data_ptr(self):
        return self._ptr

    def is_contiguous(self):
        return self._contiguous


FakeTensor.__module__ = "torch.stand_in"  # device._is_torch


def _buffers(constraint, n, hist):
    gd2, sd = constraint.geometric_dim ** 2, constraint.stress_strain_dim
    b = {"grad": FakeTensor(gd2 * n), "stress": FakeTensor(sd * n), "tangent": FakeTensor(sd * sd * n), "cache": FakeTensor(6 * n)}
    b["history"] = None if not hist else {k: FakeTensor(d * n) for k, d in hist.items()}
    return b


def _launch(law, constraint, b):
    law._evaluate_wrapped(constraint, 0.0, 1.0, b["grad"], b["stress"], b["tangent"], b["cache"], b["history"])


@pytest.fixture
def no_launch(monkeypatch):
    """a call that got as far as the counter or the launch fails the test"""
    def boom(*a, **k):
        raise AssertionError("device work before the validation finished")

    monkeypatch.setattr(jit, "launch", boom)
    monkeypatch.setattr(userlaw.UserLaw, "_counter", boom)


# --- the branch the wrappers take ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(IMPLICIT))
def test_implicit_laws_have_no_wrapped_kernel(name, no_launch):
    law = IMPLICIT[name]()
    for constraint in WRAPS:
        with pytest.raises(NotImplementedError, match="implicit"):
            law.wrapped_resources(constraint)
        with pytest.raises(NotImplementedError, match="implicit"):
            _launch(law, constraint, _buffers(constraint, 5, {"eps_n": 6, "alpha": 1}))
    assert not wrappers._has_wrapped_kernel(law)


class _GenericBranch(Exception):
    pass


@pytest.mark.parametrize("constraint", list(WRAPS), ids=[c.name for c in WRAPS])
def test_the_wrapper_takes_the_fused_launch_for_explicit_and_autodiff_laws_only(constraint, monkeypatch):
    """the launch patched to fail: an explicit or autodiff law reaches it (unless ``fused`` is off), an implicit law never does"""
    import torch

    def launched(*a, **k):
        raise AssertionError("the fused launch")

    def generic(*a, **k):
        raise _GenericBranch()

    monkeypatch.setattr(userlaw.UserLaw, "_evaluate_wrapped", launched)
    monkeypatch.setattr(_capi, "get_context", generic)
    monkeypatch.setattr(torch, "zeros", lambda numel, dtype=None, device=None: FakeTensor(numel))
    n, hist = 5, {"eps_n": 6, "alpha": 1}

    def call(law, fused=True):
        w = WRAPPERS[constraint](law)
        w.fused = fused
        b = _buffers(constraint, n, hist)
        w.evaluate(0.0, 1.0, b["grad"], b["stress"], b["tangent"], b["history"])

    for make in (LAWS["von_mises_3d"], LAWS["von_mises_3d_ad"]):
        assert wrappers._has_wrapped_kernel(make())
        with pytest.raises(AssertionError, match="the fused launch"):
            call(make())
        with pytest.raises(_GenericBranch):
            call(make(), fused=False)
    with pytest.raises(_GenericBranch):
        call(IMPLICIT["von_mises_3d_implicit"]())


def test_fields_and_objective_rates_stay_refused_by_the_wrappers():
    with pytest.raises(NotImplementedError, match="per-point parameter fields"):
        fc.PlaneStressFrom3D(S.von_mises_3d(dict(cases.VM, p_y0=np.full(4, 1200.0))))
    with pytest.raises(NotImplementedError):
        fc.PlaneStressFrom3D(fc.JaumannRate(S.von_mises_3d(cases.VM)))
    law = S.von_mises_3d(dict(cases.VM, p_y0=np.full(4, 1200.0)))
    with pytest.raises(NotImplementedError, match="per-point parameter fields"):
        law.wrapped_resources(C.PLANE_STRESS)


# --- validation ----------------------------------------------------------------------------------------------------------------

VM_HIST = {"eps_n": 6, "alpha": 1}


@pytest.mark.parametrize("constraint", list(WRAPS), ids=[c.name for c in WRAPS])
def test_every_validation_rule_raises_before_a_launch(constraint, no_launch):
    import torch

    law, n = S.von_mises_3d(cases.VM), 7
    gd2, sd = constraint.geometric_dim ** 2, constraint.stress_strain_dim
    sizes = {"grad": gd2 * n, "stress": sd * n, "tangent": sd * sd * n, "cache": 6 * n}

    def bad(which, **kw):
        b = _buffers(constraint, n, VM_HIST)
        if which in sizes:
            b[which] = FakeTensor(kw.pop("numel", sizes[which]), **kw)
        else:
            b["history"][which] = FakeTensor(kw.pop("numel", VM_HIST[which] * n), **kw)
        return b

    for which in ("grad", "stress", "tangent", "cache", "eps_n", "alpha"):
        with pytest.raises(TypeError, match="float64"):
            _launch(law, constraint, bad(which, dtype=torch.float32))
        with pytest.raises(TypeError, match="contiguous"):
            _launch(law, constraint, bad(which, contiguous=False))
        with pytest.raises(TypeError, match="GPU"):
            _launch(law, constraint, bad(which, cuda=False))
        with pytest.raises(ValueError, match="16-byte aligned"):
            _launch(law, constraint, bad(which, ptr=4096 + 8))
        if which != "grad":
            with pytest.raises(ValueError, match="grad_del_u on cuda:0"):
                _launch(law, constraint, bad(which, device=1))
    # shapes: the low-dimensional arrays, the cache, the history
    if gd2 > 1:
        with pytest.raises(ValueError, match="not a multiple of 4"):
            _launch(law, constraint, bad("grad", numel=gd2 * n + 1))
    with pytest.raises(ValueError, match="stress has"):
        _launch(law, constraint, bad("stress", numel=sd * n + sd))
    with pytest.raises(ValueError, match="tangent"):
        _launch(law, constraint, bad("tangent", numel=sd * sd * n + 1))
    with pytest.raises(ValueError, match="stress_3d has"):
        _launch(law, constraint, bad("cache", numel=6 * n - 6))
    with pytest.raises(ValueError, match="stress_3d has"):
        _launch(law, constraint, bad("cache", numel=9 * n))
    with pytest.raises(ValueError, match="history 'alpha'"):
        _launch(law, constraint, bad("alpha", numel=n + 1))
    with pytest.raises(ValueError, match="history must not be None"):
        b = _buffers(constraint, n, VM_HIST)
        b["history"] = None
        _launch(law, constraint, b)
    with pytest.raises(ValueError, match="no wrapper"):
        law._evaluate_wrapped(C.FULL, 0.0, 1.0, *(_buffers(constraint, n, VM_HIST)[k] for k in ("grad", "stress", "tangent", "cache")), None)
    # and a well-formed call gets as far as the counter
    with pytest.raises(AssertionError, match="device work"):
        _launch(law, constraint, _buffers(constraint, n, VM_HIST))


def test_a_call_inside_batched_launches_is_refused(no_launch):
    law = S.linear_elasticity(LE)
    _capi._tls.batch = object()
    try:
        with pytest.raises(NotImplementedError, match="batched_launches"):
            _launch(law, C.PLANE_STRAIN, _buffers(C.PLANE_STRAIN, 3, None))
    finally:
        _capi._tls.batch = None


@pytest.mark.parametrize("constraint", list(WRAPS), ids=[c.name for c in WRAPS])
def test_an_empty_call_launches_nothing(constraint, no_launch):
    law = S.von_mises_3d(cases.VM)
    _launch(law, constraint, _buffers(constraint, 0, VM_HIST))
    assert law.device_stats(0) == 0


# --- the rule with the zero start, on the inputs of the GPU tests ----------------------------------------------------------------

@pytest.mark.parametrize("lname", ["le", "vm", "maxwell"])
@pytest.mark.parametrize("constraint", ["PLANE_STRESS", "UNIAXIAL_STRESS"])
def test_the_zero_start_converges_on_the_inputs_of_the_gpu_tests(constraint, lname):
    """the NumPy model of the rule (stress_wrapper_util.py) with ``elastic=None``, as the kernel starts: no point fails, at most
    5 evaluations per point, and the result is the elastic-start rule's to 1.2e-12 (the Maxwell law has no elastic start: the
    zero start is the rule it always had)"""
    from stress_wrapper_util import StressFrom3DOracle
    from user_law_wrapped_util import NS, ORACLE, stress_calls

    def rel(a, b):
        return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)

    fn, params, hdims, elastic, _ = ORACLE[lname]
    sd = 4 if constraint == "PLANE_STRESS" else 1
    for n in NS:
        s0, h0, calls = stress_calls(constraint, lname, n)
        zero, start = (StressFrom3DOracle(constraint, "", fn, params, hdims, x) for x in (None, elastic))
        sz, ss, tz, ts = s0.copy(), s0.copy(), np.zeros(sd * sd * n), np.zeros(sd * sd * n)
        hz, hs = ({k: v.copy() for k, v in (h0 or {}).items()} or None for _ in range(2))
        for del_t, g in calls:
            zero.evaluate(0.0, del_t, g, sz, tz, hz)
            start.evaluate(0.0, del_t, g, ss, ts, hs)
            assert not zero.failed.any() and not start.failed.any()
            assert zero.evaluations.max() <= 5
            pairs = [(sz, ss), (tz, ts), (zero.stress_3d, start.stress_3d)] + [(hz[k], hs[k]) for k in (hz or {})]
            assert max(rel(a, b) for a, b in pairs) <= 1.2e-12
