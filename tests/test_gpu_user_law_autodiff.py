"""User laws in autodiff mode on the GPU (fenics_constitutive_amd.userlaw_sources *_AD): the forward-mode tangent against the
built-in laws, the explicit transcriptions, the golden fixtures and finite differences; stress and history bit for bit against the
explicit forms; both tangent modes of one law; the Swift law against a NumPy port; the 3-D wrappers; the refused forms."""

import numpy as np
import pytest
from golden_util import load_calls, rel_err
from swift_law_util import SWIFT_P, swift_evaluate

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import _capi  # noqa: E402
from fenics_constitutive_amd import userlaw_sources as S  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402
from fenics_constitutive_amd.userlaw import FACTOR_PY  # noqa: E402

FULL = fc.StressStrainConstraint.FULL
LE_P = {"E": 42.0, "nu": 0.3}
SLS_P = {"E0": 42.0, "E1": 10.0, "tau": 10.0, "nu": 0.2}
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
TOL = {"le": 1e-10, "sls": 1e-10, "pl": 1e-6}
DEV = "cuda"
VM_H = {"eps_n": 6, "alpha": 1}
SLS_H = {"strain_visco": 6, "strain": 6}
_laws = {}


def law(name, p=None):
    """one instance per (factory, parameters) for the module"""
    key = (name, tuple(sorted((p or {}).items())))
    if key not in _laws:
        _laws[key] = getattr(S, name)(p)
    return _laws[key]


def dev(a):
    return to_device(np.ascontiguousarray(a), DEV)


def inputs(n, seed, hist=None, gscale=1e-3, sscale=1.0):
    rng = np.random.default_rng(seed)
    g = rng.normal(scale=gscale, size=9 * n)
    s = rng.normal(scale=sscale, size=6 * n)
    h = None if hist is None else {k: rng.normal(scale=1e-3, size=d * n) for k, d in hist.items()}
    if h is not None and "alpha" in h:
        h["alpha"] = np.abs(h["alpha"])
    return g, s, h


def run(m, g, s0, h0, tangent=True):
    """ndarray evaluate on copies: (stress, tangent or None, history)"""
    n = g.size // 9
    s = s0.copy()
    t = np.full(36 * n, np.nan) if tangent else None
    h = None if h0 is None else {k: v.copy() for k, v in h0.items()}
    m.evaluate(0.0, 1.0, g, s, t, h)
    return s, t, h


def same_hist(a, b):
    return (a is None and b is None) or all(np.array_equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. linear elasticity: stress and tangent are the built-in kernel's, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 70_003])
def test_le_bits_ndarray(n):
    builtin = fc.LinearElasticityModel(LE_P, FULL)
    g, s0, _ = inputs(n, n)
    s_ref, t_ref, _ = run(builtin, g, s0, None)
    s, t, _ = run(law("linear_elasticity_ad", LE_P), g, s0, None)
    assert np.array_equal(s, s_ref) and np.array_equal(t, t_ref)
    D = t.reshape(n, 6, 6)
    assert np.array_equal(D, D.transpose(0, 2, 1))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 70_003])
@pytest.mark.parametrize("form", ["in_place", "evaluate_from"])
def test_le_bits_tensor(n, form):
    builtin = fc.LinearElasticityModel(LE_P, FULL)
    m = law("linear_elasticity_ad", LE_P)
    g, s0, _ = inputs(n, 7 * n)
    gd = dev(g)
    s_ref, t_ref = dev(s0), torch.full((36 * n,), float("nan"), dtype=torch.float64, device=DEV)
    builtin.evaluate(0.0, 1.0, gd, s_ref, t_ref, None)
    t = torch.full((36 * n,), float("nan"), dtype=torch.float64, device=DEV)
    if form == "in_place":
        s = dev(s0)
        m.evaluate(0.0, 1.0, gd, s, t, None, check=True)
    else:
        s_prev, s = dev(s0), torch.full((6 * n,), float("nan"), dtype=torch.float64, device=DEV)
        m.evaluate_from(0.0, 1.0, gd, s_prev, s, t, None, None)
        assert np.array_equal(to_host(s_prev), s0)
    torch.cuda.synchronize()
    assert torch.equal(s, s_ref) and torch.equal(t, t_ref)
    assert m.device_stats(0) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 2. Maxwell: tangent against the built-in law, stress and history against the explicit transcription
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 4099])
def test_maxwell(n):
    g, s0, h0 = inputs(n, 21, SLS_H)
    s_ad, t_ad, h_ad = run(law("spring_maxwell_ad", SLS_P), g, s0, h0)
    s_ex, t_ex, h_ex = run(law("spring_maxwell", SLS_P), g, s0, h0)
    s_bi, t_bi, h_bi = run(fc.SpringMaxwellModel(SLS_P, FULL), g, s0, h0)
    assert np.array_equal(s_ad, s_ex) and same_hist(h_ad, h_ex)
    assert rel_err(t_ad, t_bi) <= 1e-12, rel_err(t_ad, t_bi)
    assert rel_err(t_ad, t_ex) <= 1e-12, rel_err(t_ad, t_ex)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. VonMises3D
# ---------------------------------------------------------------------------------------------------------------------------
def vm_inputs(n, seed):
    g, s0, h0 = inputs(n, seed, VM_H, gscale=3e-3)
    return g, 30.0 * s0, h0


@pytest.mark.parametrize("n", [65, 4099, 70_003])
def test_von_mises_values_bitwise_and_tangent(n):
    g, s0, h0 = vm_inputs(n, 11)
    s_ad, t_ad, h_ad = run(law("von_mises_3d_ad", VM_P), g, s0, h0)
    s_ex, t_ex, h_ex = run(law("von_mises_3d", VM_P), g, s0, h0)
    s_bi, t_bi, h_bi = run(fc.VonMises3D(VM_P), g, s0, h0)
    assert np.array_equal(s_ad, s_ex) and same_hist(h_ad, h_ex)
    assert np.count_nonzero(h_ad["alpha"] != h0["alpha"]) > 0  # some points were plastic
    assert rel_err(t_ad, t_ex) <= TOL["pl"], rel_err(t_ad, t_ex)
    # the built-in call's stress and history too: a wrong built-in tangent with these right lies in the tangent path alone
    assert rel_err(s_bi, s_ex) <= TOL["pl"], rel_err(s_bi, s_ex)
    for k in h_ex:
        assert rel_err(h_bi[k], h_ex[k]) <= TOL["pl"], (k, rel_err(h_bi[k], h_ex[k]))
    assert rel_err(t_ad, t_bi) <= TOL["pl"], rel_err(t_ad, t_bi)


GOLDEN = [(f, c) for f in ("von_mises_3d.npz", "random_parameters_von_mises_3d.npz") for c in load_calls(f)]


@pytest.mark.parametrize("fname,c", GOLDEN, ids=[f"{f[:-4]}-{c.name}" for f, c in GOLDEN])
def test_von_mises_golden(fname, c):
    m = law("von_mises_3d_ad", c.params)
    s, t, h = c.fresh()
    m.evaluate(0.0, c.del_t, c.grad.copy(), s, t, h)
    assert rel_err(s, c.stress_out) <= TOL["pl"]
    assert not np.isnan(t).any() and rel_err(t, c.tangent_out) <= TOL["pl"], rel_err(t, c.tangent_out)
    for k in c.hist_out:
        assert rel_err(h[k], c.hist_out[k]) <= TOL["pl"]


def test_von_mises_zero_point_has_the_elastic_tangent():
    n = 3
    g, s0, h0 = np.zeros(9 * n), np.zeros(6 * n), {"eps_n": np.zeros(6 * n), "alpha": np.zeros(n)}
    s, t, h = run(law("von_mises_3d_ad", VM_P), g, s0, h0)
    _, t_bi, _ = run(fc.VonMises3D(VM_P), g, s0, h0)
    assert np.isfinite(t).all() and np.array_equal(s, s0)
    assert rel_err(t, t_bi) <= 1e-14, rel_err(t, t_bi)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. Swift hardening: NumPy port, finite differences, non-convergence
# ---------------------------------------------------------------------------------------------------------------------------
def swift_inputs(n, seed):
    return inputs(n, seed, VM_H, gscale=3e-3, sscale=30.0)


def mandel(g):
    g = g.reshape(-1, 9)
    return np.stack([g[:, 0], g[:, 4], g[:, 8], FACTOR_PY * (g[:, 1] + g[:, 3]), FACTOR_PY * (g[:, 2] + g[:, 6]),
                     FACTOR_PY * (g[:, 5] + g[:, 7])], axis=1)


@pytest.mark.parametrize("n", [1, 65, 1000])
def test_swift_matches_numpy_port(n):
    g, s0, h0 = swift_inputs(n, 31 + n)
    s, _, h = run(law("von_mises_swift_ad", SWIFT_P), g, s0, h0, tangent=False)
    s_np, e_np, a_np, status = swift_evaluate(SWIFT_P, mandel(g), s0.reshape(n, 6), h0["eps_n"].reshape(n, 6), h0["alpha"])
    assert not status.any()
    assert rel_err(s, s_np.reshape(-1)) <= 1e-12, rel_err(s, s_np.reshape(-1))
    assert rel_err(h["eps_n"], e_np.reshape(-1)) <= 1e-12 and rel_err(h["alpha"], a_np) <= 1e-12
    if n >= 65:
        assert np.count_nonzero(a_np != h0["alpha"]) > 0  # some points were plastic


def test_swift_tangent_matches_finite_differences():
    """central differences of the law's own tangent=None launches: grad entries that change one Mandel strain at a time"""
    n = 257
    m = law("von_mises_swift_ad", SWIFT_P)
    g, s0, h0 = swift_inputs(n, 41)
    _, t, h_ref = run(m, g, s0, h0)
    D = t.reshape(n, 6, 6)
    plastic = h_ref["alpha"] != h0["alpha"]
    assert plastic.any() and (~plastic).any()
    # a change of eps_j: grad entry (and for shear, both symmetric entries scaled by the Mandel factor)
    entries = {0: [(0, 1.0)], 1: [(4, 1.0)], 2: [(8, 1.0)], 3: [(1, 0.5 / FACTOR_PY), (3, 0.5 / FACTOR_PY)],
               4: [(2, 0.5 / FACTOR_PY), (6, 0.5 / FACTOR_PY)], 5: [(5, 0.5 / FACTOR_PY), (7, 0.5 / FACTOR_PY)]}
    hstep = 1e-7
    fd = np.zeros((n, 6, 6))
    for j, ents in entries.items():
        cols = []
        for sign in (1.0, -1.0):
            gp = g.reshape(n, 9).copy()
            for e, w in ents:
                gp[:, e] += sign * hstep * w
            s, _, _ = run(m, gp.reshape(-1), s0, h0, tangent=False)
            cols.append(s.reshape(n, 6))
        fd[:, :, j] = (cols[0] - cols[1]) / (2.0 * hstep)
    assert rel_err(D, fd) <= 1e-5, rel_err(D, fd)


@pytest.mark.parametrize("n", [64, 1000])
def test_swift_non_convergence_count_is_exact(n):
    p = dict(SWIFT_P, max_iter=1)
    m = law("von_mises_swift_ad", p)
    g, s0, h0 = swift_inputs(n, 51)
    _, _, _, status = swift_evaluate(SWIFT_P, mandel(g), s0.reshape(n, 6), h0["eps_n"].reshape(n, 6), h0["alpha"], max_iter=1)
    expected = int(status.sum())
    assert expected > 0
    for tangent in (None, torch.empty(36 * n, dtype=torch.float64, device=DEV)):
        hd = {k: dev(v) for k, v in h0.items()}
        m.evaluate(0.0, 1.0, dev(g), dev(s0), tangent, hd)
        assert m.device_stats(0) == expected
    with pytest.raises(RuntimeError, match=_capi.status_string(_capi.ERR_NONCONVERGED)):
        run(m, g, s0, h0)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. both tangent modes of one law give the same values
# ---------------------------------------------------------------------------------------------------------------------------
CASES = [("linear_elasticity_ad", LE_P, None), ("spring_maxwell_ad", SLS_P, SLS_H), ("von_mises_3d_ad", VM_P, VM_H),
         ("von_mises_swift_ad", SWIFT_P, VM_H)]


@pytest.mark.parametrize("name,p,hist", CASES, ids=[c[0] for c in CASES])
def test_tangent_none_gives_the_same_values(name, p, hist):
    n = 70_003
    g, s0, h0 = inputs(n, 61, hist, gscale=3e-3, sscale=30.0)
    m = law(name, p)
    s1, _, h1 = run(m, g, s0, h0)
    s2, _, h2 = run(m, g, s0, h0, tangent=False)
    assert np.array_equal(s1, s2) and same_hist(h1, h2)
    # tensors, out of place
    gd, sp = dev(g), dev(s0)
    hp = None if h0 is None else {k: dev(v) for k, v in h0.items()}
    outs = []
    for tangent in (torch.empty(36 * n, dtype=torch.float64, device=DEV), None):
        s = torch.empty_like(sp)
        h = None if hp is None else {k: torch.empty_like(v) for k, v in hp.items()}
        m.evaluate_from(0.0, 1.0, gd, sp, s, tangent, hp, h)
        outs.append((to_host(s), None if h is None else {k: to_host(v) for k, v in h.items()}))
    assert np.array_equal(outs[0][0], s1) and np.array_equal(outs[1][0], s1)
    assert same_hist(outs[0][1], h1) and same_hist(outs[1][1], h1)
    assert np.array_equal(to_host(sp), s0)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the 3-D wrappers
# ---------------------------------------------------------------------------------------------------------------------------
def wrapped_run(w, n, seed, hist0=None):
    rng = np.random.default_rng(seed)
    gd, sd = w.geometric_dim, w.stress_strain_dim
    g = rng.normal(scale=3e-3, size=gd * gd * n)
    s0 = 30.0 * rng.normal(size=sd * n)
    s, t = s0.copy(), np.full(sd * sd * n, np.nan)
    hd = w.history_dim
    h = None if not hd else {k: np.zeros(n * (int(np.prod(d)) if isinstance(d, tuple) else int(d))) for k, d in hd.items()}
    w.evaluate(0.0, 1.0, g, s, t, h)
    return s, t, h


def test_plane_strain_of_le_autodiff_is_bitwise():
    n = 1000
    a = wrapped_run(fc.PlaneStrainFrom3D(law("linear_elasticity_ad", LE_P)), n, 71)
    b = wrapped_run(fc.PlaneStrainFrom3D(law("linear_elasticity", LE_P)), n, 71)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_plane_stress_of_von_mises_autodiff():
    n = 1000
    a = wrapped_run(fc.PlaneStressFrom3D(law("von_mises_3d_ad", VM_P)), n, 81)
    b = wrapped_run(fc.PlaneStressFrom3D(law("von_mises_3d", VM_P)), n, 81)
    assert rel_err(a[0], b[0]) <= 1e-8 and rel_err(a[1], b[1]) <= 1e-8, (rel_err(a[0], b[0]), rel_err(a[1], b[1]))
    for k in a[2]:
        assert rel_err(a[2][k], b[2][k]) <= 1e-8


# ---------------------------------------------------------------------------------------------------------------------------
# 7. refused forms: NotImplementedError in autodiff mode too
# ---------------------------------------------------------------------------------------------------------------------------
def test_refused_forms_in_autodiff_mode():
    from fenics_constitutive_amd.multidevice import MultiDeviceResidentState
    from fenics_constitutive_amd.problem import ResidentProblemState
    from fenics_constitutive_amd.resident import ResidentState

    m = law("linear_elasticity_ad", LE_P)
    n = 256
    g, s0, _ = inputs(n, 9)
    gd = dev(g)
    s, sp, t = dev(s0), dev(s0), torch.full((36 * n,), float("nan"), dtype=torch.float64, device=DEV)
    with _capi.batched_launches():
        with pytest.raises(NotImplementedError):
            m.evaluate(0.0, 1.0, gd, s, t, None)
        with pytest.raises(NotImplementedError):
            m.evaluate_from(0.0, 1.0, gd, sp, s, t, None, None)
    rows = torch.arange(n, dtype=torch.int32, device=DEV)
    with pytest.raises(NotImplementedError):
        m.evaluate_indexed(0.0, 1.0, gd, sp, s, t, rows, None, None)
    with pytest.raises(NotImplementedError):
        m.use_devices([0])
    for make in (lambda: ResidentState(m, n), lambda: ResidentProblemState(m, n), lambda: ResidentProblemState([(m, np.arange(n))], n),
                 lambda: MultiDeviceResidentState(m, n, devices=[0])):
        with pytest.raises(NotImplementedError):
            make()
    torch.cuda.synchronize()
    assert np.array_equal(to_host(s), s0) and np.array_equal(to_host(sp), s0) and torch.isnan(t).all()
