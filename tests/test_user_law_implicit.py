"""User laws in implicit mode (UserLaw(..., tangent="implicit", unknowns=N)), the parts that need no GPU: the three implicit laws
of userlaw_sources and the linear probes of every size compile for gfx950 without scratch, the resource report, the validation of
``unknowns`` and ``newton``, compile errors, the include closure, shared code objects and the refused forms."""

import os

import numpy as np
import pytest
from implicit_law_util import PROBE_P, SWIFT_P, VM_P, probe_history, probe_matrices, probe_source

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import jit, userlaw, userlaw_sources as S

N_MAX = userlaw.MAX_UNKNOWNS

ZERO_IM = r"""
template <class T>
__device__ int fcamd_user_start(const UserParams& p, double t, double del_t, const T (&eps)[6], const double (&sigma_n)[6],
                                const UserHistoryT<double>& h_n, T (&x)[1]) {
    x[0] = 0.0;
    return 0;
}
template <class T>
__device__ void fcamd_user_residual(const UserParams& p, double t, double del_t, const T (&eps)[6], const double (&sigma_n)[6],
                                    const UserHistoryT<double>& h_n, const T (&x)[1], T (&r)[1]) {
    r[0] = x[0];
}
template <class T>
__device__ void fcamd_user_update(const UserParams& p, double t, double del_t, const T (&eps)[6], const T (&x)[1], T (&sigma)[6],
                                  UserHistoryT<T>& h) {
}
"""


def zero_law(**kw):
    kw.setdefault("tangent", "implicit")
    kw.setdefault("unknowns", 1)
    return fc.UserLaw(ZERO_IM, kw.pop("parameters", {"k": 1.0}), None, **kw)


def check_resources(law, unknowns):
    r = law.resources
    assert law.tangent_mode == "implicit" and law.unknowns == unknowns == r["unknowns"]
    assert r["scratch_bytes"] == 0 and r["stress_only"]["scratch_bytes"] == 0, r
    assert r["waves_per_simd"] in userlaw.IMPLICIT_BUDGETS and r["stress_only"]["waves_per_simd"] in userlaw.IMPLICIT_BUDGETS, r
    assert r["directions_per_pass"] in (1, 2, 3, 6), r
    # the budget the kernel was cut for; the compiler reports the occupancy it reached, at least that
    for d in (r, r["stress_only"]):
        assert d["rung_waves_per_simd"] in userlaw.IMPLICIT_BUDGETS and d["waves_per_simd"] >= d["rung_waves_per_simd"], r
    for k in (r["jacobian_directions_per_pass"], r["stress_only"]["jacobian_directions_per_pass"]):
        assert k in userlaw.jacobian_directions(unknowns), r
    assert r["vgprs"] is not None and "directions_per_pass" not in r["stress_only"]


@pytest.mark.parametrize("make,p,unknowns", [(S.von_mises_3d_implicit, VM_P, 1), (S.von_mises_swift_implicit, SWIFT_P, 1),
                                             (S.von_mises_swift_general, SWIFT_P, 8)], ids=["von_mises_3d", "swift", "swift_general"])
def test_implicit_laws_compile_without_scratch(make, p, unknowns):
    law = make(p)
    check_resources(law, unknowns)
    assert isinstance(law, fc.IncrSmallStrainModel) and law.stress_strain_dim == 6
    assert law.history_dim == {"eps_n": 6, "alpha": 1}


def test_factory_newton_defaults_and_overrides():
    assert S.von_mises_swift_implicit(SWIFT_P).newton == {"max_iter": 50, "tol": 1e-13}
    assert S.von_mises_swift_general(SWIFT_P).newton == {"max_iter": 50, "tol": 1e-13}
    assert S.von_mises_swift_general(SWIFT_P, newton={"max_iter": 1, "tol": 1e-13}).newton["max_iter"] == 1
    assert zero_law().newton == {"max_iter": 50, "tol": 1e-10}
    assert S.linear_elasticity_ad({"E": 1.0, "nu": 0.2}).newton is None and S.linear_elasticity_ad({"E": 1.0, "nu": 0.2}).unknowns is None


@pytest.mark.parametrize("unknowns", range(1, N_MAX + 1))
def test_linear_probes_compile_without_scratch(unknowns):
    A, B, c, M = probe_matrices(unknowns)
    law = fc.UserLaw(probe_source(A, B, c, M), PROBE_P, probe_history(unknowns), name=f"probe{unknowns}", tangent="implicit",
                     unknowns=unknowns)
    check_resources(law, unknowns)


def test_max_unknowns_is_eight():
    assert N_MAX == 8 and "implicit" in userlaw.TANGENT_MODES


@pytest.mark.parametrize("unknowns", [None, 0, N_MAX + 1, -1, 1.0, True, "2"])
def test_bad_unknowns_raise_value_error(unknowns):
    with pytest.raises(ValueError, match="unknowns"):
        fc.UserLaw(ZERO_IM, {"k": 1.0}, None, tangent="implicit", unknowns=unknowns)


@pytest.mark.parametrize("mode", ["explicit", "autodiff"])
@pytest.mark.parametrize("kw", [{"unknowns": 1}, {"newton": {"max_iter": 5, "tol": 1e-8}}])
def test_unknowns_and_newton_belong_to_implicit_mode(mode, kw):
    with pytest.raises(ValueError, match="implicit"):
        fc.UserLaw(S.LINEAR_ELASTICITY if mode == "explicit" else S.LINEAR_ELASTICITY_AD, {"E": 1.0, "nu": 0.2}, None, tangent=mode, **kw)


@pytest.mark.parametrize("newton", [{"max_iter": 5}, {"tol": 1e-8}, {"max_iter": 5, "tol": 1e-8, "damping": 0.5}, {}, [("max_iter", 5)],
                                    {"max_iter": -1, "tol": 1e-8}, {"max_iter": 2.5, "tol": 1e-8}, {"max_iter": True, "tol": 1e-8},
                                    {"max_iter": 5, "tol": 0.0}, {"max_iter": 5, "tol": -1e-8}, {"max_iter": 5, "tol": float("nan")},
                                    {"max_iter": 5, "tol": float("inf")}, {"max_iter": 5, "tol": "1e-8"}, 5])
def test_bad_newton_raises_value_error(newton):
    with pytest.raises(ValueError, match="newton"):
        zero_law(newton=newton)


def test_newton_values_are_accepted():
    assert zero_law(newton={"max_iter": 0, "tol": 1}).newton == {"max_iter": 0, "tol": 1.0}
    assert zero_law(newton={"max_iter": np.int64(7), "tol": np.float64(1e-9)}).newton == {"max_iter": 7, "tol": 1e-9}


def test_parameter_limit_is_thirty():
    assert userlaw.MAX_IMPLICIT_PARAMS == 30
    src = ZERO_IM
    assert fc.UserLaw(src, {f"q{k}": float(k) for k in range(30)}, None, tangent="implicit", unknowns=1).unknowns == 1
    with pytest.raises(ValueError, match="30"):
        fc.UserLaw(src, {f"q{k}": float(k) for k in range(31)}, None, tangent="implicit", unknowns=1)


@pytest.mark.parametrize("fn", ["fcamd_user_start", "fcamd_user_residual", "fcamd_user_update"])
def test_missing_function_raises_compile_error_that_names_it(fn):
    with pytest.raises(fc.UserLawCompileError) as ei:
        fc.UserLaw(ZERO_IM.replace(fn, "my_function"), {"k": 1.0}, None, name="lacks_one", tangent="implicit", unknowns=1)
    assert fn in ei.value.log and "lacks_one" in str(ei.value)


def test_include_closure_of_an_implicit_program():
    csrc = os.path.dirname(jit.JIT_DIR)
    common = {"jit/user_law_api.h", "jit/user_law_tile.h", "kernels/tile_io.h", "kernels/param_source.h", "fcamd_internal.h"}
    law = zero_law()
    for program in (law._program_implicit(law.source, 4, 1, 0), law._program_implicit(law.source, 2, 1, 6)):
        files = {os.path.relpath(f, csrc) for f in jit.include_closure(program)}
        assert files == common | {"jit/user_law_ad.h", "jit/user_law_implicit.h", "jit/user_law_implicit.hip"}
        assert "user_law.hip" not in program and "user_law_ad.hip" not in program
        assert program.rstrip().endswith('#include "user_law_implicit.hip"')
    keys = {law._compiled.key, law._compiled_stress.key}
    assert len(keys) == 2
    assert law._compiled.key == jit.cache_key(law._program_implicit(law.source, law.resources["rung_waves_per_simd"],
                                                                    law.resources["jacobian_directions_per_pass"],
                                                                    law.resources["directions_per_pass"]))


def test_implicit_program_text():
    law = fc.UserLaw(ZERO_IM, {"a": 1.0, "b": 2.0}, {"F": (3, 3), "alpha": 1}, name="im_text", tangent="implicit", unknowns=1)
    prog = law._program_implicit(ZERO_IM, 3, 1, 2)
    assert "template <class T> struct UserHistoryT { T F[9]; T alpha[1]; };" in prog
    for line in ("#define FCAMD_USER_UNKNOWNS 1", "#define FCAMD_USER_IM_KJ 1", "#define FCAMD_USER_IM_KT 2", "#define FCAMD_USER_IM_SLOT 2",
                 "#define FCAMD_USER_WAVES 3"):
        assert line in prog


def test_parameter_values_and_newton_share_one_code_object():
    a = S.von_mises_swift_implicit(SWIFT_P)
    n = userlaw.compile_count()
    b = S.von_mises_swift_implicit(dict(SWIFT_P, K=900.0, m=0.3), newton={"max_iter": 3, "tol": 1e-6})
    assert userlaw.compile_count() == n
    assert b._compiled is a._compiled and b._compiled_stress is a._compiled_stress
    assert b.newton == {"max_iter": 3, "tol": 1e-6} and b.parameters["K"] == 900.0


def test_ladder_rungs():
    assert userlaw.jacobian_directions(8) == (8, 4, 1) and userlaw.jacobian_directions(1) == (1,) and userlaw.jacobian_directions(3) == (3, 2, 1)
    small = userlaw.implicit_ladder(1, True, 13)
    assert small[0] == (4, 1, 6) and small[-1] == (1, 1, 1)
    # an 8 x 8 Jacobian with six right-hand sides cannot stay in 256 registers: those rungs are not compiled
    big = userlaw.implicit_ladder(8, True, 13)
    assert all(userlaw.IMPLICIT_BUDGETS[w] >= userlaw.implicit_register_floor(8, kt, 13) for w, _, kt in big)
    assert (2, 8, 6) not in big and (1, 8, 6) in big
    assert userlaw.implicit_ladder(8, False, 10 ** 6) == ((1, 1),)


def test_refused_forms_in_implicit_mode_need_no_gpu():
    law = zero_law()
    with pytest.raises(NotImplementedError):
        law.use_devices([0, 1])
    with pytest.raises(NotImplementedError):
        law.evaluate_indexed(0.0, 1.0, None, None, None, None, None, None, None)
    with pytest.raises(NotImplementedError):
        zero_law(parameters={"k": [1.0, 2.0]})
    for c in fc.StressStrainConstraint:
        if c.name != "FULL":
            with pytest.raises(NotImplementedError):
                zero_law(constraint=c)
    from fenics_constitutive_amd import _capi
    from fenics_constitutive_amd.multidevice import MultiDeviceResidentState
    from fenics_constitutive_amd.problem import ResidentProblemState
    from fenics_constitutive_amd.resident import ResidentState

    for make in (lambda: ResidentState(law, 64), lambda: ResidentProblemState(law, 64),
                 lambda: ResidentProblemState([(law, np.arange(64))], 64), lambda: MultiDeviceResidentState(law, 64, devices=[0])):
        with pytest.raises(NotImplementedError):
            make()
    with _capi.batched_launches():
        with pytest.raises(NotImplementedError):
            law.evaluate(0.0, 1.0, np.zeros(9), np.zeros(6), None, None)


def test_jaumann_rate_of_an_implicit_law_is_fused():
    law = S.von_mises_swift_implicit(SWIFT_P, newton={"max_iter": 7, "tol": 1e-12})
    j = fc.JaumannRate(law, {"eps_n": [0]})
    assert j._fused is not None and j.path == "fused"
    assert j._fused.tangent_mode == "implicit" and j._fused.unknowns == 1 and j._fused.newton == {"max_iter": 7, "tol": 1e-12}
    assert j._fused._compiled.key != law._compiled.key  # the rotation is compiled in
    assert j.resources["scratch_bytes"] == 0 and j.resources["unknowns"] == 1
