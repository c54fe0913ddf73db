"""Per-point parameter fields without a GPU: the field kernels exist in the device code and pass the resource guards of
tests/test_kernel_resources.py, and the constructors tell fields from scalars and refuse what they must."""

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd.interfaces import StressStrainConstraint as S  # noqa: E402

FIELD_KERNELS = ["evaluate_fields_kernel<1, 0>", "evaluate_fields_kernel<5, 0>", "evaluate_fields_kernel<6, 0>",
                 "evaluate_fields_kernel<2, 0>", "evaluate_fields_kernel<2, 1>", "evaluate_fields_kernel<2, 2>"]


@pytest.fixture(scope="module")
def field_rows():
    import kernel_resources

    return [r for r in kernel_resources.kernel_resources(["fcamd_kernels.hip"]) if "evaluate_fields" in r["name"]]


def test_field_kernels_exist_for_the_four_laws(field_rows):
    names = [r["name"] for r in field_rows]
    for k in FIELD_KERNELS:
        assert any(n.startswith("void " + k) for n in names), (k, names)
        assert any(n.startswith("void " + k.replace("fields_kernel", "fields_tail_kernel")) for n in names), (k, names)


def test_field_kernels_no_scratch_no_spill_three_waves(field_rows):
    assert len(field_rows) == 12
    for r in field_rows:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["occupancy"] >= 3, r


Y0 = np.linspace(200.0, 300.0, 100)
VM = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 250.0, "p_y00": 2500.0, "p_w": 200.0}
CM = {"mu": np.array([80769.0]), "kappa": np.array([175000.0]), "y_0": np.array([250.0]), "h": np.array([1000.0])}


def test_what_is_a_field():
    law = fc.VonMises3D(dict(VM, p_y0=Y0))
    assert law.field_points == 100 and law.field_names == ("p_y0",)
    assert fc.VonMises3D(VM).field_points is None and fc.VonMises3D(VM).field_names == ()
    law = fc.MisesPlasticityLinearHardening3D(dict(CM, y_0=Y0, h=np.full(100, 3.0)))
    assert law.field_points == 100 and law.field_names == ("y_0", "h")
    # one-element arrays and scalars keep their meaning
    assert fc.MisesPlasticityLinearHardening3D(CM).field_points is None
    assert fc.LinearElasticityModel({"E": np.array([1.0]), "nu": 0.3}, S.FULL).field_points is None
    le = fc.LinearElasticityModel({"E": Y0, "nu": 0.3}, S.FULL)
    assert le.field_points == 100 and le.D is None
    assert fc.LinearElasticity3D({"mu": Y0, "kappa": np.array([3.0])}).field_names == ("mu",)


def test_fields_are_copied_at_construction():
    y0 = Y0.copy()
    law = fc.VonMises3D(dict(VM, p_y0=y0))
    y0[:] = -1.0
    assert law._fields[2][0] == 200.0


def test_mixed_lengths_wrong_dtype_wrong_shape():
    with pytest.raises(ValueError, match="same length"):
        fc.VonMises3D(dict(VM, p_y0=Y0, p_mu=np.full(7, 80769.0)))
    with pytest.raises(TypeError, match="float64"):
        fc.VonMises3D(dict(VM, p_y0=Y0.astype(np.float32)))
    with pytest.raises(ValueError, match="1-D"):
        fc.LinearElasticity3D({"mu": Y0.reshape(10, 10), "kappa": np.array([1.0])})


def test_per_point_validation_like_the_scalar_law():
    with pytest.raises(ZeroDivisionError):
        fc.LinearElasticityModel({"E": 1.0, "nu": 0.5}, S.FULL)
    nu = np.full(100, 0.3)
    nu[17] = 0.5
    with pytest.raises(ZeroDivisionError):
        fc.LinearElasticityModel({"E": 1.0, "nu": nu}, S.FULL)
    nu[17] = -1.0
    with pytest.raises(ZeroDivisionError):
        fc.LinearElasticityModel({"E": Y0, "nu": nu}, S.FULL)


def test_laws_and_constraints_without_field_kernels_refuse():
    with pytest.raises(NotImplementedError):
        fc.LinearElasticityModel({"E": Y0, "nu": 0.3}, S.PLANE_STRAIN)
    for cls in (fc.SpringMaxwellModel, fc.SpringKelvinModel):
        with pytest.raises(NotImplementedError):
            cls({"E0": Y0, "E1": 1.0, "tau": 1.0, "nu": 0.3}, S.FULL)
    dp = {"mu": np.array([1.0]), "kappa": np.array([1.0]), "a": np.array([1.0]), "b": np.array([0.1]), "b_flow": np.array([0.1])}
    with pytest.raises(NotImplementedError):
        fc.DruckerPrager3D(dict(dp, a=Y0))
    with pytest.raises(NotImplementedError):
        fc.DruckerPragerHyperbolic3D(dict(dp, d=np.array([0.1]), mu=Y0))
    # a law without fields refuses malformed values as it always did
    with pytest.raises(ValueError, match="exactly one entry"):
        fc.DruckerPrager3D(dict(dp, a=np.ones((2, 2))))


def test_wrappers_refuse_a_field_law():
    law = fc.VonMises3D(dict(VM, p_y0=Y0))
    for w in (fc.UniaxialStrainFrom3D, fc.PlaneStrainFrom3D, fc.PlaneStressFrom3D, fc.UniaxialStressFrom3D):
        with pytest.raises(NotImplementedError):
            w(law)


def test_header_declares_the_field_flag():
    with open(os.path.join(ROOT, "include", "fcamd.h")) as fh:
        h = fh.read()
    assert "#define FCAMD_VERSION_MINOR 5" in h
    assert "#define FCAMD_EVAL_PARAM_FIELDS 16" in h and "fcamd_eval_args_set_param_fields" in h
    from fenics_constitutive_amd import _capi

    assert _capi.EVAL_PARAM_FIELDS == 16
