"""User-defined laws (fenics_constitutive_amd.UserLaw), the parts that need no GPU: hiprtc compiles for gfx950 on any machine,
the compiler's resource report, compile errors, name / parameter validation, the compile cache, and that the library's own
kernels are untouched by the feature."""

import os
import subprocess

import numpy as np
import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import _build, userlaw, userlaw_sources as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = fc.StressStrainConstraint.FULL
LE_P = {"E": 42.0, "nu": 0.3}
SLS_P = {"E0": 42.0, "E1": 10.0, "tau": 10.0, "nu": 0.2}
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}

ZERO = r"""
__device__ int fcamd_user_point(const UserParams& p, double t, double del_t, const double (&grad)[9], const double (&eps)[6],
                                double (&sigma)[6], double (&D)[36], UserHistory& h) {
    return 0;
}
"""


@pytest.mark.parametrize("make,p,four_waves", [(S.linear_elasticity, LE_P, True), (S.spring_maxwell, SLS_P, True),
                                               (S.von_mises_3d, VM_P, False)], ids=["le", "maxwell", "von_mises_3d"])
def test_transcriptions_compile_without_gpu(make, p, four_waves):
    law = make(p)
    r = law.resources
    assert r["scratch_bytes"] == 0, r
    assert r["vgprs"] is not None and r["sgprs"] is not None and r["waves_per_simd"] is not None, r
    if four_waves:
        assert r["vgprs"] <= 128 and r["waves_per_simd"] == 4, r
    assert isinstance(law, fc.IncrSmallStrainModel)
    assert law.constraint == FULL and law.stress_strain_dim == 6 and law.geometric_dim == 3


def test_history_dim_is_returned_as_given():
    hd = {"F": (3, 3), "alpha": 1}
    law = fc.UserLaw(ZERO, {"a": 1.0}, hd, name="tuple_history")
    assert law.history_dim is hd
    assert "double F[9];" in law._program(ZERO, 4)
    assert fc.UserLaw(ZERO, {}, None).history_dim is None


def test_compile_error_carries_the_source_line():
    bad = ZERO.replace("return 0;", "double x = ;  // the offending line\n    return 0;")
    with pytest.raises(fc.UserLawCompileError) as ei:
        fc.UserLaw(bad, {"E": 1.0}, None, name="broken_law")
    assert isinstance(ei.value, ValueError)
    assert "double x = ;" in str(ei.value) and "broken_law" in str(ei.value)
    assert "error" in ei.value.log


@pytest.mark.parametrize("params,hist", [
    ({"1E": 1.0}, None),              # not an identifier
    ({"E-1": 1.0}, None),
    ({"double": 1.0}, None),          # C++ keyword
    ({"E": 1.0}, {"class": 6}),
    ({"E": 1.0}, {"E": 6}),           # repeated across the two dicts
    ([("E", 1.0), ("E", 2.0)], None),  # repeated in one list of pairs
    ({"E": 1.0}, {"a": 0}),           # empty history field
    ({f"p{k}": 1.0 for k in range(33)}, None),  # more than 32 parameters
])
def test_bad_names_raise_value_error(params, hist):
    with pytest.raises(ValueError):
        fc.UserLaw(ZERO, params, hist)


@pytest.mark.parametrize("value", [np.array([1.0, 2.0]), np.array([1.0]), [1.0, 2.0]])
def test_array_parameter_is_not_implemented(value):
    with pytest.raises(NotImplementedError):
        fc.UserLaw(ZERO, {"E": value}, None)


@pytest.mark.parametrize("c", [c for c in fc.StressStrainConstraint if c.name != "FULL"], ids=lambda c: c.name)
def test_non_full_constraint_is_not_implemented(c):
    with pytest.raises(NotImplementedError):
        fc.UserLaw(ZERO, {"E": 1.0}, None, constraint=c)


def test_same_source_other_values_compiles_once():
    src = ZERO.replace("return 0;", "sigma[0] = sigma[0] + p.k * eps[0];\n    return 0;  // cache probe")
    before = userlaw.compile_count()
    a = fc.UserLaw(src, {"k": 1.0}, None, name="cache_probe")
    after_first = userlaw.compile_count()
    b = fc.UserLaw(src, {"k": 2.0}, None, name="cache_probe")
    assert after_first == before + 1 and userlaw.compile_count() == after_first
    assert a._compiled is b._compiled and a.parameters == {"k": 1.0} and b.parameters == {"k": 2.0}


def test_disk_cache(tmp_path, monkeypatch):
    monkeypatch.setenv("FCAMD_JIT_CACHE", str(tmp_path))
    src = ZERO.replace("return 0;", "return 0;  // disk cache probe")
    fc.UserLaw(src, {"k": 1.0}, None)
    assert any(f.endswith(".co") for f in os.listdir(tmp_path))
    userlaw._cache.clear()
    n = userlaw.compile_count()
    law = fc.UserLaw(src, {"k": 1.0}, None)
    assert userlaw.compile_count() == n and law.resources["scratch_bytes"] == 0


def test_refused_forms_need_no_gpu():
    law = S.linear_elasticity(LE_P)
    with pytest.raises(NotImplementedError):
        law.use_devices([0, 1])
    with pytest.raises(NotImplementedError):
        law.evaluate_indexed(0.0, 1.0, None, None, None, None, None, None, None)
    from fenics_constitutive_amd.multidevice import MultiDeviceResidentState
    from fenics_constitutive_amd.problem import ResidentProblemState
    from fenics_constitutive_amd.resident import ResidentState

    for make in (lambda: ResidentState(law, 64), lambda: ResidentProblemState(law, 64), lambda: ResidentProblemState([(law, None)], 64),
                 lambda: MultiDeviceResidentState(law, 64, devices=[0])):
        with pytest.raises(NotImplementedError):
            make()


#: _build.kernel_hash() of the library's device code before user laws existed
KERNEL_HASH = "57647943a97f66b65595976e1ec392b7a6092bb53105291a5e50215da09c0a78"


def test_library_kernels_untouched():
    """the feature adds no device code to libfcamd: the kernel sources and their hash are unchanged"""
    assert _build.kernel_hash() == KERNEL_HASH
    paths = ["fenics-constitutive_amd/csrc/kernels", "fenics-constitutive_amd/csrc/fcamd_kernels.hip",
             "fenics-constitutive_amd/csrc/fcamd_internal.h"]
    r = subprocess.run(["git", "rev-parse", "--verify", "-q", "main"], cwd=ROOT, capture_output=True, text=True)
    if r.returncode == 0:  # (a checkout with the main branch: the sources themselves)
        d = subprocess.run(["git", "diff", "main", "--", *paths], cwd=ROOT, capture_output=True, text=True, check=True)
        assert d.stdout == ""
