"""``UserLaw.evaluate_path`` without a GPU: every transcription compiles its path kernel without scratch, the ctypes mirror of the
argument struct, the validation of a call (all of it before any device work) and the NumPy model of the driver
(path_driver_util.py) on the CPU oracle against the reference-generated material-point curves."""

import ctypes
import os
import re

import numpy as np
import pytest

import material_point_cases as cases
import path_driver_util as P
from material_point import OracleLaw
from oracle import numpy_oracle as O

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import hostio, jit, userlaw
from fenics_constitutive_amd import userlaw_sources as S

LE = {"E": 42.0, "nu": 0.3}
SWIFT = {"p_ka": 175000.0, "p_mu": 80769.0, "K": 2000.0, "eps0": 0.01, "m": 0.2}
CONTROL_SETS = ((), (1, 2), (1, 2, 3, 4, 5))
LAWS = {
    "linear_elasticity": lambda: S.linear_elasticity(LE),
    "spring_maxwell": lambda: S.spring_maxwell(cases.SLS),
    "von_mises_3d": lambda: S.von_mises_3d(cases.VM),
    "linear_elasticity_ad": lambda: S.linear_elasticity_ad(LE),
    "spring_maxwell_ad": lambda: S.spring_maxwell_ad(cases.SLS),
    "von_mises_3d_ad": lambda: S.von_mises_3d_ad(cases.VM),
    "von_mises_swift_ad": lambda: S.von_mises_swift_ad(SWIFT),
    "von_mises_3d_implicit": lambda: S.von_mises_3d_implicit(cases.VM),
    "von_mises_swift_implicit": lambda: S.von_mises_swift_implicit(SWIFT),
    "von_mises_swift_general": lambda: S.von_mises_swift_general(SWIFT),
}


# --- compilation ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LAWS))
def test_every_law_compiles_its_path_kernels_without_scratch(name):
    law = LAWS[name]()
    for ctrl in CONTROL_SETS:
        if law.tangent_mode == "implicit" and ctrl:  # the documented decision: strain control only
            with pytest.raises(NotImplementedError, match="strain control"):
                law.path_resources(ctrl)
            continue
        r = law.path_resources(ctrl)
        assert r["scratch_bytes"] == 0, (name, ctrl, r)
        assert r["rung_waves_per_simd"] in userlaw.IMPLICIT_BUDGETS and r["vgprs"] > 0
        assert r["waves_per_simd"] >= r["rung_waves_per_simd"]


def test_laws_that_differ_in_values_share_the_path_code_object():
    S.von_mises_3d(cases.VM).path_resources((1, 2))
    S.von_mises_3d(dict(cases.VM, p_y0=np.full(7, 1200.0))).path_resources((1, 2))
    count = userlaw.compile_count()
    a = S.von_mises_3d(dict(cases.VM, p_y0=900.0))
    b = S.von_mises_3d(dict(cases.VM, p_y0=np.linspace(900.0, 1500.0, 33)))
    c = S.von_mises_3d(dict(cases.VM, p_y0=np.linspace(100.0, 200.0, 5)))
    for law in (a, b, c):
        law.path_resources((1, 2))
    assert userlaw.compile_count() == count
    assert b._path_kernel((1, 2))[0] is c._path_kernel((1, 2))[0]
    assert a._path_kernel((1, 2))[0] is not b._path_kernel((1, 2))[0]  # a field changes the program
    # and the control set is part of the program
    assert a._path_kernel(())[0] is not a._path_kernel((1, 2))[0]


def test_the_path_program_names_its_template_and_control_set():
    law = S.von_mises_3d_ad(cases.VM)
    prog = law._program_path(law.source, 2, (1, 2, 5))
    assert "#define FCAMD_USER_PATH 2" in prog and "#define FCAMD_PATH_NCTRL 3" in prog and "#define FCAMD_PATH_CTRL 1, 2, 5" in prog
    assert prog.rstrip().endswith('#include "user_law_path.hip"')
    assert os.path.join(jit.JIT_DIR, "user_law_path.hip") in jit.include_closure(prog)
    assert "FCAMD_PATH_CTRL" not in law._program_path(law.source, 2, ())
    assert "#define FCAMD_USER_PATH 1" in S.von_mises_3d(cases.VM)._program_path(law.source, 4, ())
    im = S.von_mises_3d_implicit(cases.VM)
    assert "#define FCAMD_USER_PATH 3" in im._program_path(im.source, 3, (), 1)


# --- the argument struct -------------------------------------------------------------------------------------------------------

def _declared_members():
    """(type, name, array extent or None) of every member of PathArgs as user_law_path.hip declares it"""
    text = open(os.path.join(jit.JIT_DIR, "user_law_path.hip")).read()
    body = text[text.index("struct PathArgs {"):]
    body = body[:body.index("};")]
    out = []
    for line in body.splitlines()[1:]:
        line = line.split("//")[0].strip()
        if not line or line.startswith("#"):
            continue
        m = re.match(r"(.*?)(\w+)(\[(\w+)\])?;$", line)
        names = [m.group(2)]
        out.append((m.group(1).strip(), names[0], m.group(4)))
    return out


@pytest.mark.parametrize("nh,nf", [(1, 0), (2, 0), (3, 2)])
def test_ctypes_mirror_of_path_args(nh, nf):
    cls = userlaw._path_args_type(nh, nf)
    members = _declared_members()
    if not nf:
        members = [m for m in members if m[1] != "fields"]
    assert [m[1] for m in members] == [f[0] for f in cls._fields_]
    extents = {"kNH": nh, "kMaxParams": userlaw.MAX_PARAMS, "kNF": nf}
    offset = 0
    for (ctype, name, extent), field in zip(members, cls._fields_):
        width = 8 * (extents[extent] if extent else 1)  # pointers, long long and double: 8 bytes each
        assert "*" in ctype or ctype in ("long long", "double"), ctype
        assert getattr(cls, name).offset == offset and getattr(cls, name).size == width, name
        assert ("*" in ctype) == (field[1] is ctypes.c_void_p or getattr(field[1], "_type_", None) is ctypes.c_void_p), name
        offset += width
    assert ctypes.sizeof(cls) == offset == 8 * (3 + nh + 3 + 4 + 4 + 32 + nf)


# --- validation ----------------------------------------------------------------------------------------------------------------

def _call(law=None, n=3, S_=2, **kw):
    law = S.von_mises_3d(cases.VM) if law is None else law
    args = dict(t0=0.0, del_t=np.ones(S_), load=np.zeros((S_, 6)), stress=np.zeros(6 * n),
                history={"eps_n": np.zeros(6 * n), "alpha": np.zeros(n)})
    args.update(kw)
    opts = {k: args.pop(k) for k in list(args) if k in ("stress_controlled", "stress_path", "strain_path", "newton", "check")}
    return law.evaluate_path(args["t0"], args["del_t"], args["load"], args["stress"], args["history"], **opts)


@pytest.fixture
def no_device_work(monkeypatch):
    """a call that got as far as staging or launching fails the test"""
    def boom(*a, **k):
        raise AssertionError("device work before the validation finished")

    monkeypatch.setattr(jit, "launch", boom)
    monkeypatch.setattr(hostio, "to_device", boom)
    monkeypatch.setattr(userlaw.UserLaw, "_path_device", boom)


@pytest.mark.parametrize("ctrl", [(1, 1), (1, 2, 1), (6,), (-1,), (1.0,), ("1",), (True,), 1, "12", (None,)])
def test_bad_control_sets_raise(ctrl, no_device_work):
    with pytest.raises(ValueError, match="stress_controlled"):
        _call(stress_controlled=ctrl)


@pytest.mark.parametrize("shape", [(2,), (12,), (3, 6), (2, 5), (2, 4, 6), (2, 3, 5), (2, 3, 6, 1), (3, 3, 6)])
def test_load_of_the_wrong_shape_raises(shape, no_device_work):
    with pytest.raises(ValueError, match="load has shape"):
        _call(load=np.zeros(shape))


def test_record_arrays_of_the_wrong_size_raise(no_device_work):
    for key in ("stress_path", "strain_path"):
        with pytest.raises(ValueError, match=key):
            _call(**{key: np.zeros(2 * 3 * 6 + 6)})
        with pytest.raises(ValueError, match=key):
            _call(**{key: np.zeros((1, 3, 6))})


@pytest.mark.parametrize("newton", [{"max_iter": 5}, {"max_iter": 5, "tol": 1e-8, "x": 1}, {"max_iter": -1, "tol": 1e-8},
                                    {"max_iter": 2.0, "tol": 1e-8}, {"max_iter": 5, "tol": 0.0}, {"max_iter": 5, "tol": float("nan")},
                                    {"max_iter": True, "tol": 1e-8}, [5, 1e-8]])
@pytest.mark.parametrize("ctrl", [(), (1, 2)])
def test_malformed_newton_raises_also_under_strain_control(newton, ctrl, no_device_work):
    with pytest.raises(ValueError, match="newton"):
        _call(newton=newton, stress_controlled=ctrl)


def test_state_and_time_arrays_are_checked(no_device_work):
    with pytest.raises(ValueError, match="multiple of 6"):
        _call(stress=np.zeros(17))
    with pytest.raises(AssertionError, match="history 'alpha'"):
        _call(history={"eps_n": np.zeros(18), "alpha": np.zeros(4)})
    with pytest.raises(TypeError, match="del_t"):
        _call(del_t=[1.0, 1.0])
    with pytest.raises(TypeError, match="del_t must be float64"):
        _call(del_t=np.ones(2, dtype=np.float32))
    with pytest.raises(ValueError, match="del_t must be 1-D"):
        _call(del_t=np.ones((2, 1)))
    with pytest.raises(TypeError, match="load must be float64"):
        _call(load=np.zeros((2, 6), dtype=np.float32))
    with pytest.raises(TypeError, match="stress_path must be C-contiguous"):
        _call(stress_path=np.zeros((6, 3, 2)).T)
    with pytest.raises(ValueError, match="history must not be None"):
        _call(history=None)


def test_field_length_must_equal_the_points(no_device_work):
    law = S.von_mises_3d(dict(cases.VM, p_y0=np.full(4, 1200.0)))
    with pytest.raises(AssertionError, match="parameter fields have 4 points, the call has 3"):
        _call(law)


def test_jaumann_rate_refuses_the_form(no_device_work):
    rate = fc.JaumannRate(S.von_mises_3d(cases.VM))
    with pytest.raises(NotImplementedError, match="evaluate_path"):
        rate.evaluate_path(0.0, np.ones(2), np.zeros((2, 6)), np.zeros(18), {"eps_n": np.zeros(18), "alpha": np.zeros(3)})
    if rate._fused is not None:  # the law with the rotation compiled in is no path law either
        with pytest.raises(NotImplementedError, match="evaluate_path"):
            _call(rate._fused)


def test_implicit_laws_refuse_stress_control_before_any_device_work(no_device_work):
    with pytest.raises(NotImplementedError, match="strain control"):
        _call(S.von_mises_3d_implicit(cases.VM), stress_controlled=(1, 2))


def test_empty_calls_launch_nothing(no_device_work):
    out = _call(S_=0, del_t=np.ones(0), load=np.zeros((0, 6)))
    assert out.dtype == np.int32 and out.tolist() == [-1, -1, -1]
    out = _call(n=0, stress=np.zeros(0), history={"eps_n": np.zeros(0), "alpha": np.zeros(0)})
    assert out.dtype == np.int32 and out.shape == (0,)


# --- the host model of the driver on the CPU oracle ----------------------------------------------------------------------------

def _oracle_law(kind):
    if kind == "spring_maxwell":
        return OracleLaw(O.MODELS_C["maxwell"], P.PARAMS[kind], P.HISTORY[kind], "FULL", pass_constraint=True)
    return OracleLaw(O.MODELS[kind], P.PARAMS[kind], P.HISTORY[kind])


@pytest.mark.parametrize("key,tol", [("uniaxial_stress_3d.load", 1e-9), ("uniaxial_cyclic_strain_3d.load", 1e-9),
                                     ("relaxation.spring_maxwell.FULL", 1e-11), ("creep.spring_maxwell.FULL", 1e-11)])
def test_host_model_on_the_oracle_matches_the_reference_curves(key, tol):
    kind, path, n, curve = P.SCENARIOS[key]
    dts, load, ctrl = path(n)
    stress = np.zeros(6 * n)
    history = {name: np.zeros(d * n) for name, d in P.HISTORY[kind].items()}
    sp, ep = np.zeros((len(dts), n, 6)), np.zeros((len(dts), n, 6))
    failed = P.drive_path(_oracle_law(kind), 0.0, dts, load, stress, history, ctrl, tol=1e-11, stress_path=sp, strain_path=ep)
    assert np.all(failed == -1)
    cases.assert_matches_reference_curve(key, curve(sp, ep), tol)
    assert np.array_equal(stress.reshape(n, 6), sp[-1])  # the committed state is the last record


def test_host_model_failure_semantics():
    """no update allowed and a non-zero target: every point fails at step 0, keeps its state and records NaN"""
    kind, path, n, _ = P.SCENARIOS["creep.spring_maxwell.FULL"]
    dts, load, ctrl = path(n)
    stress = np.zeros(6 * n)
    history = {name: np.full(d * n, 0.25) for name, d in P.HISTORY[kind].items()}
    sp = np.zeros((len(dts), n, 6))
    failed = P.drive_path(_oracle_law(kind), 0.0, dts[:3], load[:3], stress, history, ctrl, max_iter=0, stress_path=sp[:3])
    assert np.all(failed == 0) and np.all(np.isnan(sp[:3])) and not stress.any()
    assert all(np.all(h == 0.25) for h in history.values())
