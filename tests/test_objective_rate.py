"""Objective-rate wrapper (fenics_constitutive_amd.JaumannRate), the parts that need no GPU: the NumPy Hughes-Winget oracle,
the rotated programs compile for gfx950 without scratch, unrotated programs are what they were, the compile cache key
follows every file a program includes, and the validation of ``rotatable`` and the refused forms."""

import hashlib
import os
import shutil

import numpy as np
import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import jit, objective, userlaw, userlaw_sources as S
from objective_rate_util import hughes_winget, hughes_winget_closed, rotate, to_tensor

FULL = fc.StressStrainConstraint.FULL
LE_P = {"E": 42.0, "nu": 0.3}
SLS_P = {"E0": 42.0, "E1": 10.0, "tau": 10.0, "nu": 0.2}
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
SWIFT_P = {"p_ka": 175000.0, "p_mu": 80769.0, "K": 1500.0, "eps0": 1e-3, "m": 0.2}
RS_P = {"mu": np.array([80769.0]), "kappa": np.array([175000.0]), "y_0": np.array([1200.0]), "h": np.array([200.0])}
DP_P = {"mu": np.array([80769.0]), "kappa": np.array([175000.0]), "a": np.array([100.0]), "b": np.array([0.05]),
        "d": np.array([40.0]), "b_flow": np.array([0.02])}

# sha256 of the programs of the shipped transcriptions (waves 4; autodiff: K = 6) before objective rates existed
UNROTATED_PROGRAMS = {
    "linear_elasticity": "4c2b64c42d1dd54b787d7853339b56539fa0a76e262344be8d3dff69f36e9057",
    "spring_maxwell": "dc697402d52f21973142d7ddef18506f120e8031e9334a3242e35304f26fa731",
    "von_mises_3d": "fd29ac77934010451a3e7636c3cbefd67e2c1f725ab53e4502814877dd114da1",
    "linear_elasticity_ad": "23d2a334b0304ff51cc8bec992d979096a65b33c9fec768a3491391b31487945",
    "spring_maxwell_ad": "4b0f206f78cbcb651c25522b97fec847d518db36942d28f8a4c12ceba588f9c3",
    "von_mises_3d_ad": "40d7de666aa32ab31fab3a47bad24289ad2f64cfbc0550ca7ce79681fe787530",
}


# --- the NumPy oracle -----------------------------------------------------------------------------------------------------
def test_hughes_winget_is_a_proper_rotation():
    rng = np.random.default_rng(1)
    for scale in (1e-6, 1e-2, 0.3, 2.0):
        for _ in range(20):
            G = scale * rng.standard_normal((3, 3))
            R = hughes_winget(G)
            assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 * 4
            assert abs(np.linalg.det(R) - 1.0) <= 1e-15 * 4
            assert np.abs(hughes_winget_closed(G) - R).max() <= 1e-15 * 4


def test_mandel_rotation_is_r_s_rt():
    rng = np.random.default_rng(2)
    for _ in range(50):
        R = hughes_winget(0.5 * rng.standard_normal((3, 3)))
        S_ = rng.standard_normal((3, 3))
        S_ = S_ + S_.T
        v = np.array([S_[0, 0], S_[1, 1], S_[2, 2], np.sqrt(2) * S_[0, 1], np.sqrt(2) * S_[0, 2], np.sqrt(2) * S_[1, 2]])
        np.testing.assert_allclose(to_tensor(rotate(R, v)), R @ S_ @ R.T, rtol=0, atol=1e-14 * np.abs(S_).max())
    # a symmetric gradient has no spin: R = I
    G = rng.standard_normal((3, 3))
    assert np.array_equal(hughes_winget_closed(G + G.T), np.eye(3))


# --- compilation ------------------------------------------------------------------------------------------------------------
ROTATED = [(S.linear_elasticity, LE_P, None), (S.spring_maxwell, SLS_P, {"strain_visco": [0], "strain": [0]}),
           (S.von_mises_3d, VM_P, {"eps_n": [0]}), (S.linear_elasticity_ad, LE_P, None),
           (S.spring_maxwell_ad, SLS_P, {"strain_visco": [0], "strain": [0]}), (S.von_mises_3d_ad, VM_P, {"eps_n": [0]}),
           (S.von_mises_swift_ad, SWIFT_P, {"eps_n": [0]})]


@pytest.mark.parametrize("make,p,rot", ROTATED, ids=["le", "maxwell", "von_mises_3d", "le_ad", "maxwell_ad", "von_mises_3d_ad",
                                                    "swift_ad"])
def test_rotated_transcriptions_compile_without_scratch(make, p, rot):
    law = make(p)
    j = fc.JaumannRate(law, rot)
    assert j.path == "fused"
    r = j.resources
    assert r["scratch_bytes"] == 0, r
    assert r["waves_per_simd"] in userlaw.WAVES_PER_SIMD, r
    if law.tangent_mode == "autodiff":
        assert r["stress_only"]["scratch_bytes"] == 0, r
    # the rotated law is compiled separately: its program has the rotation, the law's own has not
    fused = j._fused
    assert fused._compiled.key != law._compiled.key
    assert "FCAMD_USER_ROTATE" in (fused._program(fused.source, 4) if law.tangent_mode == "explicit"
                                   else fused._program_ad(fused.source, 4, 6))


@pytest.mark.parametrize("model", [
    lambda: fc.LinearElasticityModel(LE_P, FULL), lambda: fc.SpringMaxwellModel(SLS_P, FULL), lambda: fc.VonMises3D(VM_P)],
    ids=["le", "maxwell", "von_mises_3d"])
def test_builtin_transcribed_laws_take_the_fused_path(model):
    j = fc.JaumannRate(model())
    assert j.path == "fused" and j.resources["scratch_bytes"] == 0


@pytest.mark.parametrize("model,rot", [
    (lambda: fc.SpringKelvinModel(SLS_P, FULL), {"strain_visco": [0], "strain": [0]}),
    (lambda: fc.MisesPlasticityLinearHardening3D(RS_P), {"history": [1]}),
    (lambda: fc.DruckerPrager3D(DP_P), {"history": [1]}),
    (lambda: fc.DruckerPragerHyperbolic3D(DP_P), {"history": [1]}),
    (lambda: fc.LinearElasticity3D({"mu": np.array([80769.0]), "kappa": np.array([175000.0])}), {}),
    (lambda: fc.VonMises3D({**VM_P, "p_y0": np.full(5, 1200.0)}), {"eps_n": [0]}),
], ids=["kelvin", "comfe_mises", "drucker_prager", "dp_hyperbolic", "comfe_le", "von_mises_fields"])
def test_array_level_laws_and_the_rotation_kernel(model, rot):
    j = fc.JaumannRate(model())
    assert j.path == "array" and j.rotatable == rot
    r = j.resources
    assert r["scratch_bytes"] == 0 and r["vgprs"] is not None, r


def test_forced_array_path_for_a_user_law():
    j = fc.JaumannRate(S.von_mises_3d(VM_P), {"eps_n": [0]})
    j.fused = False
    assert j.path == "array" and j.resources["scratch_bytes"] == 0


# --- unrotated laws are untouched -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make,p", [(S.linear_elasticity, LE_P), (S.spring_maxwell, SLS_P), (S.von_mises_3d, VM_P),
                                    (S.linear_elasticity_ad, LE_P), (S.spring_maxwell_ad, SLS_P), (S.von_mises_3d_ad, VM_P)],
                         ids=lambda x: getattr(x, "__name__", ""))
def test_unrotated_programs_are_byte_identical(make, p):
    law = make(p)
    prog = law._program(law.source, 4) if law.tangent_mode == "explicit" else law._program_ad(law.source, 4, 6)
    assert hashlib.sha256(prog.encode()).hexdigest() == UNROTATED_PROGRAMS[law.name]
    assert "ROTATE" not in prog and "rotation.h" not in prog


def test_cache_key_changes_with_every_included_file(tmp_path, monkeypatch):
    """in a copy of the source tree, one changed byte in any file of a rotated autodiff law's include closure changes the key;
    a file outside the closure does not"""
    fused = fc.JaumannRate(S.linear_elasticity_ad(LE_P))._fused
    program = fused._program_ad(fused.source, 4, 6)
    csrc = tmp_path / "csrc"
    shutil.copytree(os.path.dirname(jit.JIT_DIR), csrc)
    monkeypatch.setattr(jit, "INCLUDE_DIRS", (str(csrc / "jit"), str(csrc / "kernels")))
    key = jit.cache_key(program)
    assert key == fused._compiled.key  # the copy holds the same text
    files = jit.include_closure(program)
    assert {os.path.relpath(f, csrc) for f in files} == {
        "jit/user_law_ad.h", "jit/user_law_api.h", "kernels/tile_io.h", "fcamd_internal.h", "kernels/param_source.h",
        "jit/rotation.h", "jit/user_law_ad.hip", "jit/user_law_tile.h"}
    for f in files:
        with open(f, "rb") as fh:
            data = fh.read()
        with open(f, "wb") as fh:
            fh.write(bytes([data[0] ^ 1]) + data[1:])
        assert jit.cache_key(program) != key, f
        with open(f, "wb") as fh:
            fh.write(data)
    assert jit.cache_key(program) == key
    for other in ("jit/user_law.hip", "jit/rotate_state.hip", "kernels/law_sls.h"):
        with open(csrc / other, "a") as fh:
            fh.write(" ")
    assert jit.cache_key(program) == key


def test_wrapping_does_not_change_the_wrapped_law():
    law = S.von_mises_3d(VM_P)
    code, key = law._compiled.code, law._compiled.key
    fc.JaumannRate(law)
    assert law._compiled.code is code and law._compiled.key == key and law._rotate is None


# --- rotatable and the refusals ---------------------------------------------------------------------------------------------
def test_defaults():
    assert fc.JaumannRate(fc.VonMises3D(VM_P)).rotatable == {"eps_n": [0]}
    assert fc.JaumannRate(fc.SpringMaxwellModel(SLS_P, FULL)).rotatable == {"strain_visco": [0], "strain": [0]}
    assert fc.JaumannRate(fc.SpringKelvinModel(SLS_P, FULL)).rotatable == {"strain_visco": [0], "strain": [0]}
    assert fc.JaumannRate(fc.MisesPlasticityLinearHardening3D(RS_P)).rotatable == {"history": [1]}
    assert fc.JaumannRate(fc.LinearElasticityModel(LE_P, FULL)).rotatable == {}
    assert fc.JaumannRate(S.von_mises_3d(VM_P)).rotatable == {}
    assert isinstance(fc.JaumannRate(fc.VonMises3D(VM_P)), fc.IncrSmallStrainModel)


@pytest.mark.parametrize("rot", [
    {"alpha_typo": [0]},       # unknown name
    {"alpha": [0]},            # a 1-double field holds no 6-vector
    {"eps_n": [1]},            # runs past the end
    {"eps_n": [-1]},
    {"eps_n": [0.0]},          # not an integer
    {"eps_n": 0},              # not a list
    [("eps_n", 0)],            # not a mapping
])
def test_bad_rotatable_raises_value_error(rot):
    with pytest.raises(ValueError):
        fc.JaumannRate(fc.VonMises3D(VM_P), rot)


def test_bad_rotatable_for_user_and_comfe_laws():
    with pytest.raises(ValueError):
        fc.JaumannRate(S.linear_elasticity(LE_P), {"eps_n": [0]})
    with pytest.raises(ValueError):
        fc.JaumannRate(fc.MisesPlasticityLinearHardening3D(RS_P), {"history": [2]})
    with pytest.raises(ValueError):
        fc.JaumannRate(fc.MisesPlasticityLinearHardening3D(RS_P), {"history": [0, 1]})  # overlapping blocks
    assert fc.JaumannRate(fc.MisesPlasticityLinearHardening3D(RS_P), {"history": [0]}).rotatable == {"history": [0]}


def test_refused_forms():
    from fenics_constitutive_amd import _capi
    from fenics_constitutive_amd.multidevice import MultiDeviceResidentState
    from fenics_constitutive_amd.problem import ResidentProblemState
    from fenics_constitutive_amd.resident import ResidentState

    for law in (fc.JaumannRate(fc.VonMises3D(VM_P)), fc.JaumannRate(fc.SpringKelvinModel(SLS_P, FULL)),
                fc.JaumannRate(S.linear_elasticity_ad(LE_P))):
        with pytest.raises(NotImplementedError):
            ResidentState(law, 64)
        with pytest.raises(NotImplementedError):
            ResidentProblemState(law, 64)
        with pytest.raises(NotImplementedError):
            MultiDeviceResidentState(law, 64)
        with pytest.raises(NotImplementedError):
            law.evaluate_indexed(0.0, 1.0, None, None, None, None, None, None, None)
        with pytest.raises(NotImplementedError):
            law.use_devices([0, 1])
        for wrapper in (fc.PlaneStrainFrom3D, fc.UniaxialStrainFrom3D, fc.PlaneStressFrom3D, fc.UniaxialStressFrom3D):
            with pytest.raises(NotImplementedError):
                wrapper(law)
        _capi._tls.batch = object()  # what batched_launches() sets while its block runs
        try:
            with pytest.raises(NotImplementedError):
                law.evaluate(0.0, 1.0, np.zeros(9), np.zeros(6), np.zeros(36), None)
            with pytest.raises(NotImplementedError):
                law.evaluate_from(0.0, 1.0, None, None, None, None, None, None)
        finally:
            _capi._tls.batch = None


def test_refused_models():
    with pytest.raises(NotImplementedError):
        fc.JaumannRate(fc.LinearElasticityModel(LE_P, fc.StressStrainConstraint.PLANE_STRAIN))
    with pytest.raises(NotImplementedError):
        fc.JaumannRate(fc.PlaneStrainFrom3D(fc.LinearElasticityModel(LE_P, FULL)))
    with pytest.raises(ValueError):
        fc.JaumannRate(fc.JaumannRate(fc.VonMises3D(VM_P)))
    assert objective.default_rotatable(fc.LinearElasticity3D({"mu": np.array([1.0]), "kappa": np.array([2.0])})) == {}
