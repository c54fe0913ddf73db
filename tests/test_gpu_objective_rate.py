"""The objective-rate wrapper (fenics_constitutive_amd.JaumannRate) on the GPU: bit parity with the unwrapped laws for a
symmetric gradient, fused against array-level runs, the NumPy oracle, a rigidly rotated plastic state, Dienes' simple shear,
the out-of-place form and non-convergence."""

import numpy as np
import pytest
from objective_rate_util import hughes_winget, rotate, rotate_state, to_tensor

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import _capi  # noqa: E402
from fenics_constitutive_amd import userlaw_sources as S  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402

FULL = fc.StressStrainConstraint.FULL
DEV = "cuda"
LE_P = {"E": 42.0, "nu": 0.3}
SLS_P = {"E0": 42.0, "E1": 10.0, "tau": 10.0, "nu": 0.2}
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
RS_P = {"mu": np.array([80769.0]), "kappa": np.array([175000.0]), "y_0": np.array([1200.0]), "h": np.array([200.0])}
DP_P = {"mu": np.array([80769.0]), "kappa": np.array([175000.0]), "a": np.array([100.0]), "b": np.array([0.05]),
        "d": np.array([40.0]), "b_flow": np.array([0.02])}
VM_ROT = {"eps_n": [0]}
SLS_ROT = {"strain_visco": [0], "strain": [0]}


def dev(a):
    return to_device(np.ascontiguousarray(a), DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def inputs(n, seed, hist, symmetric=False, gscale=2e-3, sscale=300.0):
    """a random increment gradient, committed stress (inside the yield surfaces for sscale <= 300) and history"""
    rng = np.random.default_rng(seed)
    g = rng.normal(scale=gscale, size=(n, 3, 3))
    if symmetric:
        g = g + g.transpose(0, 2, 1)
    s = rng.normal(scale=sscale, size=6 * n)
    h = None if hist is None else {k: rng.normal(scale=1e-3, size=d * n) for k, d in hist.items()}
    if h is not None and "alpha" in h:
        h["alpha"] = np.abs(h["alpha"])
    if h is not None and "history" in h:
        h["history"].reshape(n, -1)[:, 0] = np.abs(h["history"].reshape(n, -1)[:, 0])
    return g.reshape(-1), s, h


def run(law, g, s0, h0, form, tangent=True):
    """stress, tangent, history (NumPy) after one call of ``law`` in ``form``: "ndarray", "in_place" (tensors) or "from"
    (evaluate_from on tensors; the committed arrays are checked to be untouched)"""
    n = g.size // 9
    if form == "ndarray":
        s, t = s0.copy(), (np.full(36 * n, np.nan) if tangent else None)
        h = None if h0 is None else {k: v.copy() for k, v in h0.items()}
        law.evaluate(0.0, 1.0, g, s, t, h)
        return s, t, h
    gd, td = dev(g), (torch.full((36 * n,), float("nan"), dtype=torch.float64, device=DEV) if tangent else None)
    if form == "in_place":
        sd = dev(s0)
        hd = None if h0 is None else {k: dev(v) for k, v in h0.items()}
        law.evaluate(0.0, 1.0, gd, sd, td, hd)
    else:
        sp, sd = dev(s0), torch.full((6 * n,), float("nan"), dtype=torch.float64, device=DEV)
        hp = None if h0 is None else {k: dev(v) for k, v in h0.items()}
        hd = None if h0 is None else {k: torch.full_like(v, float("nan")) for k, v in hp.items()}
        law.evaluate_from(0.0, 1.0, gd, sp, sd, td, hp, hd)
        assert same(to_host(sp), s0)
        for k in h0 or {}:
            assert same(to_host(hp[k]), h0[k]), k
    torch.cuda.synchronize()
    return (to_host(sd), None if td is None else to_host(td), None if hd is None else {k: to_host(v) for k, v in hd.items()})


def assert_same(a, b):
    assert same(a[0], b[0]), "stress"
    if a[1] is not None:
        assert same(a[1], b[1]), "tangent"
    for k in a[2] or {}:
        assert same(a[2][k], b[2][k]), k


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# (name, wrapped law, the unwrapped law it must match bit for bit with a symmetric gradient, history, rotatable)
def _cases():
    return {
        "le_builtin": (lambda: fc.LinearElasticityModel(LE_P, FULL), lambda: fc.LinearElasticityModel(LE_P, FULL), None, None),
        "maxwell_fused": (lambda: fc.SpringMaxwellModel(SLS_P, FULL), lambda: S.spring_maxwell(SLS_P),
                          {"strain_visco": 6, "strain": 6}, None),
        "von_mises_fused": (lambda: fc.VonMises3D(VM_P), lambda: S.von_mises_3d(VM_P), {"eps_n": 6, "alpha": 1}, None),
        "von_mises_ad": (lambda: S.von_mises_3d_ad(VM_P), lambda: S.von_mises_3d_ad(VM_P), {"eps_n": 6, "alpha": 1}, VM_ROT),
        "kelvin_array": (lambda: fc.SpringKelvinModel(SLS_P, FULL), lambda: fc.SpringKelvinModel(SLS_P, FULL),
                         {"strain_visco": 6, "strain": 6}, None),
        "comfe_mises_array": (lambda: fc.MisesPlasticityLinearHardening3D(RS_P), lambda: fc.MisesPlasticityLinearHardening3D(RS_P),
                              {"history": 7}, None),
        "dp_hyperbolic_array": (lambda: fc.DruckerPragerHyperbolic3D(DP_P), lambda: fc.DruckerPragerHyperbolic3D(DP_P),
                                {"history": 7}, None),
    }


CASES = _cases()


# 1. a symmetric gradient has no spin: the wrapper is the unwrapped law, bit for bit
@pytest.mark.parametrize("form", ["ndarray", "in_place", "from"])
@pytest.mark.parametrize("case", list(CASES))
def test_symmetric_gradient_is_bit_identical(case, form):
    make, make_ref, hist, rot = CASES[case]
    j = fc.JaumannRate(make(), rot)
    assert j.path == ("array" if case.endswith("_array") else "fused")
    n = 1000
    g, s0, h0 = inputs(n, 11, hist, symmetric=True, sscale=2000.0)  # some points yield
    if case.startswith("dp_"):  # Drucker-Prager: a small spread around a compressive prestress (benchlib.workloads)
        g, s0, h0 = inputs(n, 11, hist, symmetric=True, gscale=3e-4, sscale=50.0)
        s0.reshape(n, 6)[:, :3] -= 1000.0
    assert_same(run(j, g, s0, h0, form), run(make_ref(), g, s0, h0, form))


# 2. fused and array-level runs of the same transcription agree bit for bit with a finite spin
@pytest.mark.parametrize("form", ["in_place", "from", "ndarray"])
@pytest.mark.parametrize("make,hist,rot", [
    (lambda: S.von_mises_3d(VM_P), {"eps_n": 6, "alpha": 1}, VM_ROT),
    (lambda: S.spring_maxwell(SLS_P), {"strain_visco": 6, "strain": 6}, SLS_ROT),
    (lambda: S.von_mises_3d_ad(VM_P), {"eps_n": 6, "alpha": 1}, VM_ROT),
    (lambda: S.linear_elasticity_ad(LE_P), None, None),
], ids=["von_mises", "maxwell", "von_mises_ad", "le_ad"])
@pytest.mark.parametrize("n", [1, 65, 70_003])
def test_fused_equals_array_level(make, hist, rot, form, n):
    g, s0, h0 = inputs(n, n, hist, gscale=0.02, sscale=2000.0)
    fused = fc.JaumannRate(make(), rot)
    arr = fc.JaumannRate(make(), rot)
    arr.fused = False
    assert fused.path == "fused" and arr.path == "array"
    a, b = run(fused, g, s0, h0, form), run(arr, g, s0, h0, form)
    assert_same(a, b)
    assert not same(a[0], run(make(), g, s0, h0, form)[0])  # the rotation did something
    # stress-only launches too
    assert_same(run(fused, g, s0, h0, form, tangent=False), run(arr, g, s0, h0, form, tangent=False))


# 3. both paths: the NumPy rotation followed by the law
_ORACLE = {
    "von_mises": (lambda: fc.VonMises3D(VM_P), {"eps_n": 6, "alpha": 1}, VM_ROT),
    "maxwell": (lambda: fc.SpringMaxwellModel(SLS_P, FULL), {"strain_visco": 6, "strain": 6}, SLS_ROT),
    "le": (lambda: fc.LinearElasticityModel(LE_P, FULL), None, {}),
    "von_mises_ad": (lambda: S.von_mises_3d_ad(VM_P), {"eps_n": 6, "alpha": 1}, VM_ROT),
    "kelvin": (lambda: fc.SpringKelvinModel(SLS_P, FULL), {"strain_visco": 6, "strain": 6}, SLS_ROT),
    "comfe_mises": (lambda: fc.MisesPlasticityLinearHardening3D(RS_P), {"history": 7}, {"history": [1]}),
}


@pytest.mark.parametrize("case,path", [(c, p) for c in _ORACLE for p in ("fused", "array") if p == "array" or c not in
                                       ("kelvin", "comfe_mises")])
def test_matches_numpy_oracle(case, path):
    make, hist, rot = _ORACLE[case]
    n = 500
    g, s0, h0 = inputs(n, 3, hist, gscale=0.02, sscale=2000.0)
    j = fc.JaumannRate(make(), rot)
    if path == "array":
        j.fused = False
    assert j.path == path
    s, t, h = run(j, g, s0, h0, "ndarray")
    sr, hr = rotate_state(g, s0, h0, rot)
    # the law the path runs: the fused built-ins are their userlaw_sources transcriptions
    transcription = {"von_mises": lambda: S.von_mises_3d(VM_P), "maxwell": lambda: S.spring_maxwell(SLS_P),
                     "le": lambda: S.linear_elasticity(LE_P)}
    ref = run((transcription[case] if path == "fused" and case in transcription else make)(), g, sr, hr, "ndarray")
    assert rel(s, ref[0]) <= 1e-12 and rel(t, ref[1]) <= 1e-12
    for k in h0 or {}:
        assert rel(h[k], ref[2][k]) <= 1e-12, k
    # and the rotation itself: a law that does nothing shows the rotated committed state
    zero_g = g.reshape(n, 3, 3)
    zero_g = (zero_g - zero_g.transpose(0, 2, 1)).reshape(-1)  # a pure spin: no strain
    if hist is None:
        s2, _, _ = run(j, zero_g, s0, h0, "ndarray")
        assert rel(s2, rotate_state(zero_g, s0, None, {})[0]) <= 1e-12


# 4. rigid rotation of a pre-stressed plastic state: Q sigma_0 Q^T, Q eps_p Q^T; equivalent stress and alpha unchanged
@pytest.mark.parametrize("path", ["fused", "array"])
def test_rigid_rotation_of_plastic_state(path):
    n, steps = 256, 40
    rng = np.random.default_rng(7)
    s0 = rng.normal(scale=150.0, size=(n, 6))  # deviatoric norm below sqrt(2/3) p_y0: stays elastic under a pure spin
    eps0 = rng.normal(scale=1e-3, size=(n, 6))
    alpha0 = np.abs(rng.normal(scale=1e-3, size=n))
    j = fc.JaumannRate(fc.VonMises3D(VM_P))
    if path == "array":
        j.fused = False
    assert j.path == path
    sd, hd = dev(s0.reshape(-1)), {"eps_n": dev(eps0.reshape(-1)), "alpha": dev(alpha0)}
    Q = np.tile(np.eye(3), (n, 1, 1))
    td = torch.empty(36 * n, dtype=torch.float64, device=DEV)
    for _ in range(steps):
        w = rng.normal(scale=0.1, size=(n, 3))
        G = np.zeros((n, 3, 3))
        G[:, 0, 1], G[:, 0, 2], G[:, 1, 2] = -w[:, 2], w[:, 1], -w[:, 0]
        G = G - G.transpose(0, 2, 1)
        j.evaluate(0.0, 1.0, dev(G.reshape(-1)), sd, td, hd, check=True)
        Q = np.stack([hughes_winget(G[p]) for p in range(n)]) @ Q
    s, eps, alpha = to_host(sd).reshape(n, 6), to_host(hd["eps_n"]).reshape(n, 6), to_host(hd["alpha"])
    for p in range(n):
        assert rel(s[p], rotate(Q[p], s0[p])) <= 1e-12
        assert rel(eps[p], rotate(Q[p], eps0[p])) <= 1e-12

    def mises(v):
        d = to_tensor(v)
        d = d - np.trace(d) / 3 * np.eye(3)
        return np.sqrt(1.5 * np.sum(d * d))

    for p in range(n):
        assert abs(mises(s[p]) - mises(s0[p])) <= 1e-12 * mises(s0[p])
    assert np.array_equal(alpha, alpha0)


# 5. Dienes' simple shear with linear elasticity: second-order convergence to the Jaumann solution
def test_dienes_simple_shear():
    E, nu = LE_P["E"], LE_P["nu"]
    mu = E / (2 * (1 + nu))
    gam, n = 2 * np.pi, 64

    def error(steps):
        j = fc.JaumannRate(fc.LinearElasticityModel(LE_P, FULL))
        G = np.zeros((n, 3, 3))
        G[:, 0, 1] = gam / steps
        gd, sd = dev(G.reshape(-1)), torch.zeros(6 * n, dtype=torch.float64, device=DEV)
        for _ in range(steps):
            j.evaluate(0.0, 1.0, gd, sd, None, None)
        s = to_host(sd).reshape(n, 6)
        assert np.array_equal(s, np.tile(s[0], (n, 1)))
        exact = np.array([mu * (1 - np.cos(gam)), -mu * (1 - np.cos(gam)), 0.0, np.sqrt(2) * mu * np.sin(gam)])
        return np.abs(s[0, :4] - exact).max()

    e1, e2 = error(200), error(400)
    assert e1 < 1e-3 * mu
    assert 3.5 < e1 / e2 < 4.5, (e1, e2)


# 6. evaluate_from leaves the committed arrays untouched (run() checks it) and equals evaluate
@pytest.mark.parametrize("case", ["von_mises_fused", "kelvin_array", "comfe_mises_array", "maxwell_fused"])
def test_evaluate_from_equals_evaluate(case):
    make, _, hist, rot = CASES[case]
    g, s0, h0 = inputs(1000, 5, hist, gscale=0.02, sscale=2000.0)
    j = fc.JaumannRate(make(), rot)
    assert_same(run(j, g, s0, h0, "from"), run(j, g, s0, h0, "in_place"))


# 7. non-convergence still raises
REFUSE_STRETCH = r"""
__device__ int fcamd_user_point(const UserParams& p, double t, double del_t, const double (&grad)[9], const double (&eps)[6],
                                double (&sigma)[6], double (&D)[36], UserHistory& h) {
    for (int i = 0; i < 6; ++i) sigma[i] = sigma[i] + p.k * eps[i];
    h.count[0] = h.count[0] + 1.0;
    return grad[0] > 0.0 ? 1 : 0;
}
"""


@pytest.mark.parametrize("path", ["fused", "array"])
def test_non_convergence_raises(path):
    n = 1000
    j = fc.JaumannRate(fc.UserLaw(REFUSE_STRETCH, {"k": 2.0}, {"count": 1}, name="refuse_stretch"))
    if path == "array":
        j.fused = False
    g, s0, _ = inputs(n, 5, None, gscale=0.1)
    expected = int(np.count_nonzero(g.reshape(-1, 9)[:, 0] > 0))
    assert expected > 0
    hd = {"count": torch.zeros(n, dtype=torch.float64, device=DEV)}
    j.evaluate(0.0, 1.0, dev(g), dev(s0), None, hd)
    assert j.device_stats(0) == expected
    with pytest.raises(RuntimeError, match=_capi.status_string(_capi.ERR_NONCONVERGED)):
        j.evaluate(0.0, 1.0, dev(g), dev(s0), None, {"count": torch.zeros(n, dtype=torch.float64, device=DEV)}, check=True)
    h = {"count": np.zeros(n)}
    with pytest.raises(RuntimeError, match=_capi.status_string(_capi.ERR_NONCONVERGED)):
        j.evaluate(0.0, 1.0, g, s0.copy(), None, h)
    assert np.array_equal(h["count"], np.ones(n))  # the results are written before the error


def test_simple_shear_example_runs():
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "simple_shear_jaumann.py"), "256", "400"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Dienes" in r.stdout
