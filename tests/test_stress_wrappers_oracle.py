"""CPU checks of the plane-stress / uniaxial-stress wrapper rule (tests/stress_wrapper_util.py, the NumPy model of
PlaneStressFrom3D / UniaxialStressFrom3D around the oracle's 3-D laws) and of the package's public classes: the rule
reproduces the native low-dimensional elastic laws, the reference's uniaxial-stress plasticity curves without an outer
Newton iteration, and its condensed tangent is the derivative of its stress."""

import os

import numpy as np
import pytest
from golden_util import GOLDEN
from material_point import HostState, MaterialPoints
from stress_wrapper_util import VM_P, StressFrom3DOracle, fused_recipe
from wrappers_util import load_constraint_calls


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize("constraint", ["PLANE_STRESS", "UNIAXIAL_STRESS"])
def test_linear_elasticity_equals_native_constraint(constraint):
    """LinearElasticityModel(FULL) behind the wrapper rule == LinearElasticityModel(PLANE_STRESS / UNIAXIAL_STRESS)
    on the golden inputs (committed sigma_zz taken as 0: the native plane-stress law leaves it as it is, the wrapper
    holds it at 0)."""
    calls = [c for c in load_constraint_calls() if c["law"] == "le" and c["constraint"] == constraint]
    assert calls
    for c in calls:
        w = StressFrom3DOracle(constraint, "le")
        s = c["stress_in"].copy()
        if constraint == "PLANE_STRESS":
            s.reshape(-1, 4)[:, 2] = 0.0
        t = np.full_like(c["tangent_out"], np.nan)
        w.evaluate(0.0, c["del_t"], c["grad"], s, t, None)
        assert np.all(w.evaluations == 1)  # the elastic start is the answer
        if constraint == "PLANE_STRESS":
            keep = [0, 1, 3]
            assert _rel(s.reshape(-1, 4)[:, keep], c["stress_out"].reshape(-1, 4)[:, keep]) <= 1e-13
            assert np.all(s.reshape(-1, 4)[:, 2] == 0.0)
            tt = t.reshape(-1, 4, 4)
            assert np.all(tt[:, 2, :] == 0.0) and np.all(tt[:, :, 2] == 0.0)
        else:
            assert _rel(s, c["stress_out"]) <= 1e-13
        assert _rel(t, c["tangent_out"]) <= 1e-13


@pytest.mark.parametrize("case", ["uniaxial_stress_3d", "uniaxial_cyclic_strain_3d"])
def test_von_mises_uniaxial_stress_curves(case):
    """material_point.npz: the FULL law with the lateral strains found by the material-point Newton iteration;
    here the wrapper finds them per point, and the harness prescribes eps_xx alone (no outer iteration)."""
    z = np.load(os.path.join(GOLDEN, "material_point.npz"))
    disp, load = z[case + ".disp"], z[case + ".load"]
    n = disp.shape[1]
    law = StressFrom3DOracle("UNIAXIAL_STRESS", "vm")
    mp = MaterialPoints(HostState(law, n), "UNIAXIAL_STRESS")
    out = [np.zeros(n)]
    for k in range(1, disp.shape[0]):
        out.append(mp.increment(1.0, {0: disp[k] - disp[k - 1]})[:, 0].copy())
        assert not law.failed.any() and law.evaluations.max() <= 6
    assert max(mp.iterations) == 0
    assert np.max(np.abs(np.array(out) - load)) <= 1e-9 * VM_P["p_y0"]


def _grad_of(constraint, k, h):
    """gradient increment of Mandel strain component k (of the low-dimensional layout) by h"""
    if constraint == "UNIAXIAL_STRESS":
        return np.array([h])
    g = np.zeros(4)
    if k == 0:
        g[0] = h
    elif k == 1:
        g[3] = h
    else:  # Mandel shear: (g01 + g10) / sqrt(2)
        g[1] = g[2] = h / np.sqrt(2.0)
    return g


@pytest.mark.parametrize("lname", ["vm", "dp", "dp_hyper"])
@pytest.mark.parametrize("constraint", ["PLANE_STRESS", "UNIAXIAL_STRESS"])
def test_condensed_tangent_is_the_derivative(constraint, lname):
    """central differences of the wrapper's stress with respect to the mapped strains == its condensed tangent (the laws
    with a consistent 3-D tangent; comfe-rs MisesPlasticity3D's is not, see tests/material_point_cases.py)"""
    sd = 4 if constraint == "PLANE_STRESS" else 1
    s0, h0, grads = fused_recipe(constraint, lname, 200)
    n = s0.size // sd
    w = StressFrom3DOracle(constraint, lname)

    def run(g):
        s, t = s0.copy(), np.zeros(sd * sd * n)
        h = None if h0 is None else {k: v.copy() for k, v in h0.items()}
        w.stress_3d = None
        w.evaluate(0.0, 1.0, g, s, t, h)
        assert not w.failed.any()
        return s.reshape(n, sd), t.reshape(n, sd, sd)

    g = grads[3]
    _, t = run(g)
    comps = [0, 1, 3] if sd == 4 else [0]
    eps = 1e-8
    checked = 0
    for k in comps:
        dg = np.tile(_grad_of(constraint, k, eps), n)
        sp, _ = run(g + dg)
        sm, _ = run(g - dg)
        fd = (sp - sm) / (2 * eps)
        # points whose plastic/elastic state flips inside the stencil have no derivative: skip them.  Absolute floor: the
        # stresses carry the laws' own stopping rules (Drucker-Prager: 1e-8), and a perfectly plastic uniaxial tangent is ~0
        ok = np.abs(fd - t[:, :, k]).max(axis=1) <= 1e-4 * np.abs(t[:, :, k]).max(axis=1) + 1e-2
        assert ok.mean() > 0.95, (k, np.sort(np.abs(fd - t[:, :, k]).max(axis=1))[-5:])
        checked += ok.sum()
        if sd == 4:
            assert np.all(t[:, 2, :] == 0.0) and np.all(t[:, :, 2] == 0.0)
    assert checked > 0


def test_package_exposes_the_stress_wrappers():
    import fenics_constitutive_amd as fc

    C = fc.StressStrainConstraint
    assert "PlaneStressFrom3D" in fc.__all__ and "UniaxialStressFrom3D" in fc.__all__
    vm = fc.VonMises3D(VM_P)
    for W, c, gd, sd in ((fc.PlaneStressFrom3D, C.PLANE_STRESS, 2, 4), (fc.UniaxialStressFrom3D, C.UNIAXIAL_STRESS, 1, 1)):
        w = W(vm)
        assert w.constraint == c and w.geometric_dim == gd and w.stress_strain_dim == sd
        assert w.history_dim == vm.history_dim and w.stress_3d is None and w.fused
        with pytest.raises(AssertionError):
            W(fc.LinearElasticityModel({"E": 42.0, "nu": 0.3}, c))
    # the reference has no such classes: its import-path mirror does not carry them
    from fenics_constitutive_amd.models import utils as ref_utils

    assert not hasattr(ref_utils, "PlaneStressFrom3D") and not hasattr(ref_utils, "UniaxialStressFrom3D")
