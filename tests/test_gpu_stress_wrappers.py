"""GPU checks of PlaneStressFrom3D / UniaxialStressFrom3D: the fused kernel (wrap modes 3 / 4 of
fcamd_evaluate_device_ex's wrapper form) and the generic path against the NumPy model of the rule
(tests/stress_wrapper_util.py), the native low-dimensional elastic laws, the reference's uniaxial-stress plasticity
curves, the material-point harness, and the error paths of the C ABI."""

import ctypes as C
import os
import warnings

import numpy as np
import pytest
from golden_util import GOLDEN
from material_point import HostState, MaterialPoints
from oracle import numpy_oracle as O
from stress_wrapper_util import DP_P, DPH_P, LE_P, RS_P, VM_P, StressFrom3DOracle, fused_recipe, isotropic

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import _capi  # noqa: E402

FULL = fc.StressStrainConstraint.FULL
SLS_P = {"E0": 42.0, "E1": 10.0, "tau": 10.0, "nu": 0.2}
# bounds of the 3-D parity tests per law (tests/test_gpu_wrappers.py, test_gpu_parity.py)
TOL = {"le": 1e-10, "vm": 1e-6, "comfe_mises": 1e-6, "dp": 1e-6, "dp_hyper": 1e-6}
WRAPPERS = {"PLANE_STRESS": fc.PlaneStressFrom3D, "UNIAXIAL_STRESS": fc.UniaxialStressFrom3D}
os.environ.setdefault("FCAMD_SMALL_CALL_WARNING", "0")


def law_of(lname):
    a = lambda p: {k: np.array([v]) for k, v in p.items()}  # noqa: E731
    return {"le": lambda: fc.LinearElasticityModel(LE_P, FULL), "vm": lambda: fc.VonMises3D(VM_P),
            "comfe_mises": lambda: fc.MisesPlasticityLinearHardening3D(a(RS_P)), "dp": lambda: fc.DruckerPrager3D(a(DP_P)),
            "dp_hyper": lambda: fc.DruckerPragerHyperbolic3D(a(DPH_P))}[lname]()


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def d(x):
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def h(x):
    return x.cpu().numpy()


# --- 1. the reference's uniaxial-stress curves: no outer Newton iteration -------------------------------------------
@pytest.mark.parametrize("path", ["host", "torch"])
@pytest.mark.parametrize("case", ["uniaxial_stress_3d", "uniaxial_cyclic_strain_3d"])
def test_von_mises_uniaxial_stress_curves(case, path):
    z = np.load(os.path.join(GOLDEN, "material_point.npz"))
    disp, load = z[case + ".disp"], z[case + ".load"]
    n = disp.shape[1]
    w = fc.UniaxialStressFrom3D(fc.VonMises3D(VM_P))
    out = [np.zeros(n)]
    if path == "host":
        mp = MaterialPoints(HostState(w, n), "UNIAXIAL_STRESS")
        for k in range(1, disp.shape[0]):
            out.append(mp.increment(1.0, {0: disp[k] - disp[k - 1]})[:, 0].copy())
        assert max(mp.iterations) == 0
    else:
        s_c, s_t, t = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(3))
        h_c = {"eps_n": torch.zeros(6 * n, dtype=torch.float64, device="cuda"), "alpha": torch.zeros(n, dtype=torch.float64, device="cuda")}
        for k in range(1, disp.shape[0]):
            s_t.copy_(s_c)
            h_t = {key: v.clone() for key, v in h_c.items()}
            w.evaluate(0.0, 1.0, d(disp[k] - disp[k - 1]), s_t, t, h_t)
            assert w.model.device_stats().n_nonconverged == 0
            s_c.copy_(s_t)
            h_c = h_t
            out.append(h(s_t))
    assert np.max(np.abs(np.array(out) - load)) <= 1e-9 * VM_P["p_y0"]


# --- 2. LinearElasticityModel(FULL) wrapped == the native plane-stress / uniaxial-stress law --------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("constraint", ["PLANE_STRESS", "UNIAXIAL_STRESS"])
def test_linear_elasticity_equals_native_constraint(constraint, fused):
    C_ = getattr(fc.StressStrainConstraint, constraint)
    sd = C_.stress_strain_dim
    n = 64 * 3 + 11
    rng = np.random.default_rng(5)
    g = rng.normal(scale=1e-2, size=C_.geometric_dim**2 * n)
    s0 = rng.normal(size=sd * n)
    if sd == 4:
        s0.reshape(n, 4)[:, 2] = 0.0
    native = fc.LinearElasticityModel(LE_P, C_)
    s_n, t_n = s0.copy(), np.zeros(sd * sd * n)
    native.evaluate(0.0, 1.0, g, s_n, t_n, None)
    w = WRAPPERS[constraint](fc.LinearElasticityModel(LE_P, FULL))
    w.fused = fused
    s_w, t_w = s0.copy(), np.full(sd * sd * n, np.nan)
    w.evaluate(0.0, 1.0, g, s_w, t_w, None)
    assert rel(s_w, s_n) <= 1e-13 and rel(t_w, t_n) <= 1e-13
    if sd == 4:
        assert np.all(s_w.reshape(n, 4)[:, 2] == 0.0)
        tt = t_w.reshape(n, 4, 4)
        assert np.all(tt[:, 2, :] == 0.0) and np.all(tt[:, :, 2] == 0.0)
    s3 = h(w.stress_3d).reshape(n, 6)
    assert np.all(np.abs(s3[:, 2]) <= 1e-12 * np.linalg.norm(s3, axis=1))


# --- 3. the five fused laws against the NumPy rule, and against the generic path ------------------------------------
def _residual_ok(constraint, s3):
    b = [2] if constraint == "PLANE_STRESS" else [1, 2]
    r = np.max(np.abs(s3[:, b]), axis=1)
    return np.all((r == 0) | (r <= 1e-12 * np.linalg.norm(s3, axis=1) * (1 + 1e-9)))


@pytest.mark.parametrize("lname", ["le", "vm", "comfe_mises", "dp", "dp_hyper"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4097])
@pytest.mark.parametrize("constraint", ["PLANE_STRESS", "UNIAXIAL_STRESS"])
def test_fused_stress_wrapper(constraint, n, lname):
    W = WRAPPERS[constraint]
    sd = 4 if constraint == "PLANE_STRESS" else 1
    s0, h0, grads = fused_recipe(constraint, lname, n)
    a, b = W(law_of(lname)), W(law_of(lname))
    b.fused = False
    o = StressFrom3DOracle(constraint, lname)
    sa, sb, so = d(s0), d(s0), s0.copy()
    ha = None if h0 is None else {k: d(v) for k, v in h0.items()}
    hb = None if h0 is None else {k: d(v) for k, v in h0.items()}
    ho = None if h0 is None else {k: v.copy() for k, v in h0.items()}
    ta = torch.zeros(sd * sd * n, dtype=torch.float64, device="cuda")
    tb = torch.zeros_like(ta)
    to = np.zeros(sd * sd * n)
    tol = TOL[lname]
    for call, g in enumerate(grads):
        a.evaluate(0.0, 1.0, d(g), sa, ta, ha)
        if lname != "le":
            assert a.model.device_stats().n_nonconverged == 0
        b.evaluate(0.0, 1.0, d(g), sb, tb, hb)
        o.evaluate(0.0, 1.0, g, so, to, ho)
        assert not o.failed.any()
        assert rel(h(sa), so) <= tol and rel(h(ta), to) <= tol, (call, rel(h(sa), so), rel(h(ta), to))
        assert rel(h(a.stress_3d).reshape(n, 6), o.stress_3d) <= tol
        for k in (ha or {}):
            assert rel(h(ha[k]), ho[k]) <= tol, k
        assert _residual_ok(constraint, h(a.stress_3d).reshape(n, 6))
        if sd == 4:
            assert np.all(h(sa).reshape(n, 4)[:, 2] == 0.0)
            tt = h(ta).reshape(n, 4, 4)
            assert np.all(tt[:, 2, :] == 0.0) and np.all(tt[:, :, 2] == 0.0)
        # fused == generic (two runs of the same rule)
        assert rel(h(sa), h(sb)) <= 1e-10 and rel(h(ta), h(tb)) <= 1e-10, (call, rel(h(sa), h(sb)), rel(h(ta), h(tb)))
        for k in (ha or {}):
            assert rel(h(ha[k]), h(hb[k])) <= 1e-10, k
    assert a.grad_del_u_3d is None and a.tangent_3d is None and b.tangent_3d is not None
    assert lname == "le" or a.model.device_stats().n_plastic > 0 or n < 10


# --- 4. the generic path: laws without a fused tile ----------------------------------------------------------------
@pytest.mark.parametrize("lname", ["maxwell", "kelvin", "comfe_le"])
@pytest.mark.parametrize("constraint", ["PLANE_STRESS", "UNIAXIAL_STRESS"])
def test_generic_path(constraint, lname):
    W = WRAPPERS[constraint]
    sd = 4 if constraint == "PLANE_STRESS" else 1
    n = 300
    rng = np.random.default_rng(11)
    if lname == "comfe_le":
        p = {"mu": 80769.0, "kappa": 175000.0}
        model = fc.LinearElasticity3D({k: np.array([v]) for k, v in p.items()})
        o = StressFrom3DOracle(constraint, "", O.comfe_linear_elasticity, p, None, isotropic(p["kappa"], p["mu"]))
        hist = None
    else:
        model = (fc.SpringMaxwellModel if lname == "maxwell" else fc.SpringKelvinModel)(SLS_P, FULL)
        fn = O.spring_maxwell if lname == "maxwell" else O.spring_kelvin
        o = StressFrom3DOracle(constraint, "", fn, SLS_P, {"strain_visco": 6, "strain": 6}, None)
        hist = {"strain_visco": rng.normal(scale=1e-3, size=6 * n), "strain": rng.normal(scale=1e-3, size=6 * n)}
    w = W(model)
    s = rng.normal(size=sd * n)
    if sd == 4:
        s.reshape(n, 4)[:, 2] = 0.0
    so = s.copy()
    hw = None if hist is None else {k: v.copy() for k, v in hist.items()}
    ho = None if hist is None else {k: v.copy() for k, v in hist.items()}
    t, to = np.zeros(sd * sd * n), np.zeros(sd * sd * n)
    for call, del_t in enumerate((1e-8, 2.0, 0.1)):
        g = rng.normal(scale=1e-3, size=(4 if sd == 4 else 1) * n)
        w.evaluate(0.0, del_t, g, s, t, hw)
        o.evaluate(0.0, del_t, g, so, to, ho)
        assert rel(s, so) <= 1e-10 and rel(t, to) <= 1e-10, call
        for k in (hw or {}):
            assert rel(hw[k], ho[k]) <= 1e-10, k
        assert _residual_ok(constraint, h(w.stress_3d).reshape(n, 6))


# --- 5. consistency triangle: FULL + free (1, 2), plane stress + free (1), uniaxial stress --------------------------
def test_consistency_triangle_von_mises():
    n = 6
    amp = 0.05 * np.linspace(0.6, 1.0, n)
    setups = [(fc.VonMises3D(VM_P), "FULL", (1, 2)), (fc.PlaneStressFrom3D(fc.VonMises3D(VM_P)), "PLANE_STRESS", (1,)),
              (fc.UniaxialStressFrom3D(fc.VonMises3D(VM_P)), "UNIAXIAL_STRESS", ())]
    loads = []
    for law, constraint, free in setups:
        mp = MaterialPoints(HostState(law, n), constraint, tol=1e-10)
        prev, load = np.zeros(n), []
        for s in np.linspace(0, 1, 41)[1:]:
            cur = s * amp
            load.append(mp.increment(1.0, {0: cur - prev}, free=free)[:, 0].copy())
            prev = cur
        assert max(mp.iterations) <= 6, (constraint, mp.iterations)
        loads.append(np.array(load))
    assert np.max(loads[0]) > VM_P["p_y0"]  # the plastic range is reached
    for other in loads[1:]:
        assert np.max(np.abs(other - loads[0])) <= 1e-9 * VM_P["p_y0"]


# --- 6. error paths --------------------------------------------------------------------------------------------------
def test_non_full_model_is_refused():
    for W, c in ((fc.PlaneStressFrom3D, fc.StressStrainConstraint.PLANE_STRESS),
                 (fc.UniaxialStressFrom3D, fc.StressStrainConstraint.UNIAXIAL_STRESS)):
        with pytest.raises(AssertionError):
            W(fc.LinearElasticityModel(LE_P, c))


def _raw_args(n, sd, wrapper_constraint, g, s, t, s3, hist):
    arr = (C.c_void_p * max(1, len(hist)))(*[x.data_ptr() for x in hist])
    x = _capi.EvalArgs(g.data_ptr(), s.data_ptr(), s.data_ptr(), t.data_ptr(), C.cast(arr, C.POINTER(C.c_void_p)),
                       C.cast(arr, C.POINTER(C.c_void_p)), len(hist), None, None, 0, None, None, None, None, wrapper_constraint,
                       s3.data_ptr())
    return x, arr


def test_abi_wrapper_constraint_values():
    n = 100
    law = fc.VonMises3D(VM_P)
    m = law._handle(0)
    z = lambda k: torch.zeros(k * n, dtype=torch.float64, device="cuda")  # noqa: E731
    g, s, t, s3, hist = z(4), z(4), z(16), z(6), [z(6), z(1)]
    lib = m._lib
    for wc, expect in ((5, _capi.ERR_BAD_ARG), (9, _capi.ERR_BAD_ARG), (-1, _capi.ERR_BAD_ARG),
                       (4, _capi.OK), (2, _capi.OK)):
        x, keep = _raw_args(n, 4, wc, g, s, t, s3, hist)
        st = lib.fcamd_evaluate_device_ex(m.handle, 0.0, 1.0, n, C.byref(x))
        assert st == expect, (wc, st)
    torch.cuda.synchronize()
    # laws without a fused tile keep refusing the wrapper form
    sls = fc.SpringMaxwellModel(SLS_P, FULL)
    ms = sls._handle(0)
    x, keep = _raw_args(n, 4, 4, g, s, t, s3, [z(6), z(6)])
    assert ms._lib.fcamd_evaluate_device_ex(ms.handle, 0.0, 1.0, n, C.byref(x)) == _capi.ERR_UNSUPPORTED
    # the batch entry refuses every wrapper form
    for wc in (2, 4):
        x, keep = _raw_args(n, 4, wc, g, s, t, s3, hist)
        models = (C.c_void_p * 1)(m.handle)
        ns = (C.c_int64 * 1)(n)
        args = (_capi.EvalArgs * 1)(x)
        st = lib.fcamd_evaluate_batch(1, C.cast(models, C.POINTER(C.c_void_p)), ns, args, 0.0, 1.0)
        assert st == _capi.ERR_UNSUPPORTED, st


def test_drucker_prager_nonconvergence_surfaces():
    """inputs on which the Drucker-Prager law's own Newton iteration fails (the NumPy rule raises on them) surface
    through the fused wrapper as the law's non-convergence"""
    rng = np.random.default_rng(7)
    n = 600
    s = rng.uniform(-2000.0, 900.0, size=n)
    g = rng.normal(size=n) * 10 ** rng.uniform(-5.0, -1.0, size=n)
    o = StressFrom3DOracle("UNIAXIAL_STRESS", "dp_hyper")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(O.DruckerPragerNotConverged):
            o.evaluate(0.0, 1.0, g, s.copy(), np.zeros(n), {"history": np.zeros(7 * n)})
    w = fc.UniaxialStressFrom3D(law_of("dp_hyper"))
    with pytest.raises(RuntimeError, match="did not converge"):
        w.evaluate(0.0, 1.0, g.copy(), s.copy(), np.zeros(n), {"history": np.zeros(7 * n)})
    assert w.model._handle(0).last_stats().n_nonconverged > 0
