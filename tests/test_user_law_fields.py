"""Per-point parameter fields of user laws (UserLaw(..., fields=...), csrc/jit/user_law_fields.h), the parts that need no GPU:
the validation of ``fields``, the generated program text and its include closure, shared code objects, the compiler's resource
report of the shipped transcriptions with every parameter a field (pinned as observed), the wrappers, and the
inputs of tests/test_gpu_user_law_fields.py checked with the CPU ports."""

import os
import shutil

import numpy as np
import pytest
from user_law_fields_util import (GROUPS, LAWS, PLASTIC_FAMILIES, assert_mixed, constant_fields, grads, group_fields, group_of,
                                  lognormal_fields, make, port_steps, scalars)

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import jit, userlaw
from fenics_constitutive_amd import userlaw_sources as S

FULL = fc.StressStrainConstraint.FULL
SRC = S.LINEAR_ELASTICITY
F5 = np.full(5, 42.0)
COMMON = {"jit/user_law_api.h", "jit/user_law_tile.h", "kernels/tile_io.h", "kernels/param_source.h", "fcamd_internal.h"}
MODE_FILES = {"explicit": {"jit/user_law.hip"}, "autodiff": {"jit/user_law_ad.h", "jit/user_law_ad.hip"},
              "implicit": {"jit/user_law_ad.h", "jit/user_law_implicit.h", "jit/user_law_implicit.hip"}}


def le(parameters, fields, **kw):
    return fc.UserLaw(SRC, parameters, None, fields=fields, name="le_fields", **kw)


def program(law, waves=4):
    if law.tangent_mode == "explicit":
        return law._program(law.source, waves)
    if law.tangent_mode == "autodiff":
        return law._program_ad(law.source, waves, 6)
    return law._program_implicit(law.source, waves, 1, 6)


# --- validation ---------------------------------------------------------------------------------------------------------------
def test_properties_with_and_without_fields():
    e = np.linspace(1.0, 5.0, 5)
    law = le({"nu": 0.3}, {"E": e})
    assert law.field_points == 5 and law.field_names == ("E",) and law.parameters == {"nu": 0.3}
    assert list(law.fields) == ["E"] and np.array_equal(law.fields["E"], e)
    # copies in, copies out: the law's values are immutable
    e[0] = -1.0
    assert law.fields["E"][0] == 1.0
    law.fields["E"][1] = -1.0
    assert law.fields["E"][1] == 2.0
    plain = le({"E": 42.0, "nu": 0.3}, None)
    assert plain.field_points is None and plain.field_names == () and plain.fields == {}
    assert plain.parameters == {"E": 42.0, "nu": 0.3}
    # a list of pairs; the order of UserParams is the scalars', then the fields'
    law = le([("nu", 0.3)], [("E", F5)])
    assert law.field_names == ("E",)
    assert "struct UserParams { double nu; double E; };" in program(law)


def test_a_one_element_array_is_a_field_over_one_point():
    law = le({"nu": 0.3}, {"E": np.array([42.0])})
    assert law.field_points == 1 and law.field_names == ("E",) and "E" not in law.parameters


def test_arrays_in_parameters_stay_refused():
    for bad in (F5, np.array([42.0]), [42.0, 43.0]):
        with pytest.raises(NotImplementedError, match="scalar parameters only"):
            le({"E": bad, "nu": 0.3}, None)
    with pytest.raises(NotImplementedError, match="scalar parameters only"):
        le({"nu": F5}, {"E": F5})


def test_field_values_are_checked():
    with pytest.raises(ValueError, match=r"all parameter fields of a law have the same length, got \[5, 6\]"):
        le({}, {"E": F5, "nu": np.full(6, 0.3)})
    with pytest.raises(TypeError, match="parameter field 'E' must be float64, got float32"):
        le({"nu": 0.3}, {"E": F5.astype(np.float32)})
    with pytest.raises(TypeError, match="parameter field 'E' must be float64, got int64"):
        le({"nu": 0.3}, {"E": np.arange(5)})
    with pytest.raises(ValueError, match=r"parameter field 'E' must be 1-D, got shape \(5, 1\)"):
        le({"nu": 0.3}, {"E": F5.reshape(5, 1)})
    with pytest.raises(ValueError, match=r"parameter field 'E' must be 1-D, got shape \(\)"):
        le({"nu": 0.3}, {"E": np.array(42.0)})
    with pytest.raises(ValueError, match="empty"):
        le({"nu": 0.3}, {"E": np.zeros(0)})
    for scalar in (42.0, [42.0] * 5, None):
        with pytest.raises(TypeError, match="field 'E' must be a 1-D float64 NumPy array or ROCm tensor"):
            le({"nu": 0.3}, {"E": scalar})


def test_torch_tensors_are_fields():
    torch = pytest.importorskip("torch")
    law = le({"nu": 0.3}, {"E": torch.linspace(1.0, 5.0, 5, dtype=torch.float64)})
    assert law.field_points == 5 and np.array_equal(law.fields["E"], np.linspace(1.0, 5.0, 5))
    with pytest.raises(TypeError, match="must be float64"):
        le({"nu": 0.3}, {"E": torch.ones(5, dtype=torch.float32)})
    with pytest.raises(ValueError, match="must be 1-D"):
        le({"nu": 0.3}, {"E": torch.ones(5, 1, dtype=torch.float64)})


def test_field_names_follow_the_rules_of_parameter_names():
    for bad, msg in (("2E", "not a C identifier"), ("E-mod", "not a C identifier"), (3, "not a C identifier"), ("double", "C\\+\\+ keyword")):
        with pytest.raises(ValueError, match=msg):
            fc.UserLaw(SRC, {"nu": 0.3}, None, fields=[(bad, F5)])
    with pytest.raises(ValueError, match="'E' is given more than once"):
        le({"E": 1.0, "nu": 0.3}, {"E": F5})
    with pytest.raises(ValueError, match="'E' is given more than once"):
        le({"nu": 0.3}, [("E", F5), ("E", F5)])
    with pytest.raises(ValueError, match="'E' is given more than once"):
        fc.UserLaw(SRC, {"nu": 0.3}, {"E": 6}, fields={"E": F5})


def test_parameters_and_fields_share_the_limit():
    names = [f"q{k}" for k in range(userlaw.MAX_PARAMS)]
    p = dict({n: 1.0 for n in names[:20]}, E=42.0, nu=0.3)
    with pytest.raises(ValueError, match="33 parameters and fields; at most 32"):
        le(p, {n: F5 for n in names[20:31]})
    law = le(p, {n: F5 for n in names[20:30]})  # 22 + 10
    assert len(law.parameters) + len(law.field_names) == userlaw.MAX_PARAMS and law.resources["scratch_bytes"] == 0
    with pytest.raises(ValueError, match="31 parameters and fields; at most 30 for an implicit law"):
        fc.UserLaw(S.VON_MISES_SWIFT_IMPLICIT, {n: 1.0 for n in names[:26]}, {"eps_n": 6, "alpha": 1},
                   fields={k: F5 for k in scalars("von_mises_swift_implicit")}, tangent="implicit", unknowns=1)


def test_implicit_newton_slot_stays_behind_the_scalars():
    p = scalars("von_mises_swift_implicit")
    law = make("von_mises_swift_implicit", constant_fields(p, 5, names=("K",)))
    assert law.field_names == ("K",) and list(law.parameters) == ["p_ka", "p_mu", "eps0", "m"]
    assert "#define FCAMD_USER_IM_SLOT 4\n" in program(law, 2)
    assert law.newton == {"max_iter": 50, "tol": 1e-13}


def test_size_mismatch_raises_before_anything_is_staged():
    law = le({"nu": 0.3}, {"E": F5})
    n = 6
    s, t = np.full(6 * n, 7.0), np.full(36 * n, 7.0)
    with pytest.raises(AssertionError, match="UserLaw: the parameter fields have 5 points, the call has 6"):
        law.evaluate(0.0, 1.0, np.zeros(9 * n), s, t, None)
    assert (s == 7.0).all() and (t == 7.0).all()


@pytest.mark.parametrize("name", list(LAWS) + ["von_mises_swift_ad"])
def test_helpers_route_arrays_to_fields(name):
    p = dict(GROUPS["swift"][0]) if name == "von_mises_swift_ad" else scalars(name)
    plain = getattr(S, name)(p)
    assert plain.field_points is None and list(plain.parameters)[:len(p)] == list(p)
    last = list(p)[-1]
    one = getattr(S, name)(constant_fields(p, 5, names=(last,)))
    assert one.field_names == (last,) and one.field_points == 5
    assert list(one.parameters)[:len(p) - 1] == list(p)[:-1] and np.array_equal(one.fields[last], np.full(5, p[last]))
    every = make(name, constant_fields(p, 7))
    assert every.field_names == tuple(p) and every.field_points == 7
    assert set(every.parameters) <= {"max_iter"}
    assert every.tangent_mode == plain.tangent_mode and every.history_dim == plain.history_dim and every.name == plain.name
    assert every.newton == plain.newton and every.unknowns == plain.unknowns


# --- program text -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LAWS))
def test_a_law_without_fields_has_the_program_it_had(name):
    law = getattr(S, name)(scalars(name))
    prog = program(law)
    assert "FCAMD_USER_FIELDS" not in prog and "FCAMD_USER_NFIELDS" not in prog and "user_law_fields.h" not in prog
    assert "UserParams fcamd_user_params(const double* v) {" in prog
    csrc = os.path.dirname(jit.JIT_DIR)
    files = {os.path.relpath(f, csrc) for f in jit.include_closure(prog)}
    assert files == COMMON | MODE_FILES[law.tangent_mode]
    assert "fields" not in [f for f, _ in law._args_cls._fields_]


@pytest.mark.parametrize("name", ["von_mises_3d", "von_mises_3d_ad", "von_mises_swift_implicit"])
def test_program_and_include_closure_of_a_field_law(name):
    p = scalars(name)
    law = make(name, constant_fields(p, 5, names=list(p)[2:4]))
    prog = program(law)
    a, b = list(p)[2:4]
    rest = [k for k in p if k not in (a, b)]
    assert "#define FCAMD_USER_NFIELDS 2\n" in prog and f"#define FCAMD_USER_FIELDS(X) X(0, {a}) X(1, {b})\n" in prog
    assert "struct UserParams {" + "".join(f" double {k};" for k in rest + [a, b]) + " };" in prog
    assert "UserParams fcamd_user_params(const double* v, const fcamd_user::UserFieldValues& f) {" in prog
    assert "".join(f" p.{k} = v[{i}];" for i, k in enumerate(rest)) + f" p.{a} = f.v[0]; p.{b} = f.v[1];" in prog
    assert "fcamd_user_params(const double* v) {" not in prog
    csrc = os.path.dirname(jit.JIT_DIR)
    files = {os.path.relpath(f, csrc) for f in jit.include_closure(prog)}
    assert files == COMMON | MODE_FILES[law.tangent_mode] | {"jit/user_law_fields.h"}
    # the pointers travel behind the existing members
    members = [f for f, _ in law._args_cls._fields_]
    plain = [f for f, _ in getattr(S, name)(p)._args_cls._fields_]
    assert members == plain + ["fields"]
    assert law._args_cls.fields.offset == getattr(S, name)(p)._args_cls.params.offset + 8 * userlaw.MAX_PARAMS
    assert law._args_cls.fields.size == 16


def test_cache_key_follows_the_fields_header(tmp_path, monkeypatch):
    """in a copy of the source tree, one changed byte in user_law_fields.h changes the key of a field program and leaves the key
    of a program without fields alone"""
    p = scalars("von_mises_3d_ad")
    with_fields, without = make("von_mises_3d_ad", constant_fields(p, 5, names=("p_y0",))), S.von_mises_3d_ad(p)
    pf, pw = program(with_fields), program(without)
    csrc = tmp_path / "csrc"
    shutil.copytree(os.path.dirname(jit.JIT_DIR), csrc)
    monkeypatch.setattr(jit, "INCLUDE_DIRS", (str(csrc / "jit"), str(csrc / "kernels")))
    kf, kw = jit.cache_key(pf), jit.cache_key(pw)
    assert kf != kw
    header = csrc / "jit" / "user_law_fields.h"
    data = header.read_bytes()
    header.write_bytes(bytes([data[0] ^ 1]) + data[1:])
    assert jit.cache_key(pf) != kf and jit.cache_key(pw) == kw
    header.write_bytes(data)
    assert jit.cache_key(pf) == kf


# --- code objects ---------------------------------------------------------------------------------------------------------
def test_laws_that_differ_in_field_values_or_lengths_compile_once():
    p = scalars("von_mises_3d")
    first = make("von_mises_3d", constant_fields(p, 5, names=("p_y0", "p_w")))
    count = userlaw.compile_count()
    rng = np.random.default_rng(0)
    other = S.von_mises_3d(dict(p, p_mu=1.0, p_y0=rng.uniform(1.0, 2.0, size=977), p_w=rng.uniform(1.0, 2.0, size=977)))
    assert userlaw.compile_count() == count
    assert other._compiled is first._compiled and other.field_points == 977
    # other field names: another program
    third = S.von_mises_3d(constant_fields(p, 5, names=("p_y0", "p_y00")))
    assert third._compiled is not first._compiled


# --- resources --------------------------------------------------------------------------------------------------------------
#: observed, every parameter a field: law -> (VGPRs, waves per SIMD) of the tangent kernel and, where the mode has one, of the
#: stress-only kernel; implicit laws: the rungs kept (waves, Jacobian directions per pass, tangent directions per pass).  Next to
#: the scalar law's: a derived constant that was wave-uniform is a per-lane value here.
ALL_FIELDS = {
    "linear_elasticity": ((56, 4), None, None),
    "spring_maxwell": ((112, 4), None, None),
    "von_mises_3d": ((154, 3), None, None),
    "linear_elasticity_ad": ((72, 4), (52, 4), 6),
    "spring_maxwell_ad": ((144, 3), (96, 4), 6),
    "von_mises_3d_ad": ((248, 2), (136, 3), 6),
    "von_mises_3d_implicit": ((190, 2), (144, 3), ((2, 1, 6), (3, 1))),
    "von_mises_swift_implicit": ((209, 2), (174, 2), ((2, 1, 6), (2, 1))),
    "von_mises_swift_general": ((256, 1), (256, 1), ((1, 8, 6), (1, 8))),
}


@pytest.mark.parametrize("name", list(LAWS))
def test_resources_with_every_parameter_a_field(name):
    law = make(name, constant_fields(scalars(name), 7))
    r = law.resources
    tangent, stress_only, rungs = ALL_FIELDS[name]
    print(name, {k: v for k, v in r.items() if k != "stress_only"}, r.get("stress_only"))
    assert r["scratch_bytes"] == 0, r
    assert (r["vgprs"], r["waves_per_simd"]) == tangent, r
    if stress_only is None:
        assert "stress_only" not in r
        return
    assert r["stress_only"]["scratch_bytes"] == 0, r
    assert (r["stress_only"]["vgprs"], r["stress_only"]["waves_per_simd"]) == stress_only, r
    if law.tangent_mode == "autodiff":
        assert r["directions_per_pass"] == rungs
    else:
        assert (r["rung_waves_per_simd"], r["jacobian_directions_per_pass"], r["directions_per_pass"]) == rungs[0], r
        assert (r["stress_only"]["rung_waves_per_simd"], r["stress_only"]["jacobian_directions_per_pass"]) == rungs[1], r


# --- wrappers ---------------------------------------------------------------------------------------------------------------
def test_jaumann_rate_carries_the_fields():
    law = make("von_mises_3d", group_fields("vm", 100, names=("p_y0", "p_w")))
    j = fc.JaumannRate(law, {"eps_n": [0]})
    assert j.path == "fused" and j.field_points == 100
    fused = j._fused
    assert fused.field_names == ("p_y0", "p_w") and fused.parameters == law.parameters
    assert all(np.array_equal(fused.fields[k], law.fields[k]) for k in law.field_names)
    prog = program(fused)
    assert "FCAMD_USER_ROTATE" in prog and "FCAMD_USER_FIELDS" in prog
    assert j.resources["scratch_bytes"] == 0
    # the wrapped law is what it was
    assert law._rotate is None and "FCAMD_USER_ROTATE" not in program(law)
    # an implicit law keeps its Newton options and its fields
    sw = make("von_mises_swift_implicit", constant_fields(scalars("von_mises_swift_implicit"), 9, names=("K",)))
    fused = fc.JaumannRate(sw, {"eps_n": [0]})._fused
    assert fused.field_names == ("K",) and fused.newton == sw.newton and fused.unknowns == 1


@pytest.mark.parametrize("wrapper", ["PlaneStrainFrom3D", "UniaxialStrainFrom3D", "PlaneStressFrom3D", "UniaxialStressFrom3D"])
def test_from3d_wrappers_refuse_a_field_law(wrapper):
    law = le({"nu": 0.3}, {"E": F5})
    with pytest.raises(NotImplementedError):
        getattr(fc, wrapper)(law)
    with pytest.raises(NotImplementedError):
        getattr(fc, wrapper)(fc.JaumannRate(law))


def test_refused_forms_stay_refused():
    from fenics_constitutive_amd.resident import ResidentState

    law = le({"nu": 0.3}, {"E": F5})
    with pytest.raises(NotImplementedError):
        ResidentState(law, 5)
    with pytest.raises(NotImplementedError):
        law.use_devices([0])
    with pytest.raises(NotImplementedError):
        law.evaluate_indexed()
    with pytest.raises(NotImplementedError):
        fc.UserLaw(SRC, {"nu": 0.3}, None, fc.StressStrainConstraint.PLANE_STRAIN, fields={"E": F5})


# --- the inputs of the GPU tests --------------------------------------------------------------------------------------------
# grads(n) is the first n points of one set, so the first 63 points decide for every n >= 63; 1000 is checked as well.
@pytest.mark.parametrize("n", [63, 1000])
@pytest.mark.parametrize("spin", [0.0, 0.05], ids=["as_drawn", "spinning"])
@pytest.mark.parametrize("family", PLASTIC_FAMILIES)
def test_gpu_inputs_mix_elastic_and_plastic_points_in_every_group(family, spin, n):
    """every parameter set on the whole arrays (the reference runs of the constant-field and scattered tests) leaves elastic and
    plastic points among each group's points in the last step.  Spinning gradients (the Jaumann tests): the port rotates the
    committed stress and eps_n before every step"""
    gs = grads(n, spin)
    group = group_of(n)
    for gi, p in enumerate(GROUPS[family]):
        *_, plastic, status = port_steps(family, p, gs, rotate=spin != 0.0)
        assert not status.any()
        assert_mixed(plastic, group, f"{family} set {gi}")


@pytest.mark.parametrize("family", PLASTIC_FAMILIES)
def test_gpu_inputs_of_the_continuous_fields(family):
    n = 63
    *_, plastic, status = port_steps(family, lognormal_fields(family, n), grads(n))
    assert not status.any()
    assert_mixed(plastic, None, family)


def test_gpu_inputs_of_the_non_convergence_count():
    """one Newton step converges no plastic point of the Swift law: the count of the GPU test is the number of plastic points"""
    n = 1000
    p = lognormal_fields("swift", n, names=("K",))
    *_, plastic, status = port_steps("swift", p, grads(n), max_iter_last=1)
    assert plastic.any() and (~plastic).any()
    assert np.array_equal(status != 0, plastic)
