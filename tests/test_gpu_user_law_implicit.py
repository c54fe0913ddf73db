"""User laws in implicit mode on the GPU (fenics_constitutive_amd.userlaw_sources *_IMPLICIT / *_GENERAL and generated linear probes):
the golden fixtures, the Swift forms against the NumPy port, pivoting at every size, the consistent tangent against finite
differences and the autodiff law, bit identities, non-convergence and the wrappers."""

import numpy as np
import pytest
from golden_util import load_calls, rel_err
from implicit_law_util import (PROBE_P, SWIFT_P, VM_H, VM_P, mandel, probe_expected, probe_history, probe_matrices, probe_source,
                               swift_inputs)
from objective_rate_util import rotate_state
from swift_law_util import swift_evaluate
from wrappers_util import load_sequences

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import _capi, userlaw  # noqa: E402
from fenics_constitutive_amd import userlaw_sources as S  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402
from fenics_constitutive_amd.userlaw import FACTOR_PY  # noqa: E402

DEV = "cuda"
TOL = {"pl": 1e-6, "tight": 1e-10, "port": 1e-12}
SIZES = [1, 63, 64, 65, 1000]
N_MAX = userlaw.MAX_UNKNOWNS
SWIFT_FORMS = ["von_mises_swift_implicit", "von_mises_swift_general"]
_laws = {}


def law(name, p, **newton):
    """one instance per (factory, parameters, newton) for the module"""
    key = (name, tuple(sorted(p.items())), tuple(sorted(newton.items())))
    if key not in _laws:
        _laws[key] = getattr(S, name)(p, **({"newton": dict({"max_iter": 50, "tol": 1e-13}, **newton)} if newton else {}))
    return _laws[key]


def probe(unknowns, start="return 1;", zero_jacobian=False):
    key = ("probe", unknowns, start, zero_jacobian)
    if key not in _laws:
        A, B, c, M = probe_matrices(unknowns)
        src = probe_source(np.zeros_like(A) if zero_jacobian else A, B, c, M, start)
        _laws[key] = (fc.UserLaw(src, PROBE_P, probe_history(unknowns), name=f"probe{unknowns}", tangent="implicit", unknowns=unknowns),
                      (A, B, c, M))
    return _laws[key]


def dev(a):
    return to_device(np.ascontiguousarray(a), DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def run(m, g, s0, h0, tangent=True):
    """ndarray evaluate on copies: (stress, tangent or None, history)"""
    n = g.size // 9
    s = s0.copy()
    t = np.full(36 * n, np.nan) if tangent else None
    h = {k: v.copy() for k, v in h0.items()}
    m.evaluate(0.0, 1.0, g, s, t, h)
    return s, t, h


def run_tensor(m, g, s0, h0, tangent=True, out_of_place=False):
    """the same call on device tensors (in place, or evaluate_from with the committed arrays checked untouched)"""
    n = g.size // 9
    gd = dev(g)
    td = torch.full((36 * n,), float("nan"), dtype=torch.float64, device=DEV) if tangent else None
    if out_of_place:
        sp, hp = dev(s0), {k: dev(v) for k, v in h0.items()}
        sd, hd = torch.full_like(sp, float("nan")), {k: torch.full_like(v, float("nan")) for k, v in hp.items()}
        m.evaluate_from(0.0, 1.0, gd, sp, sd, td, hp, hd)
        assert same(to_host(sp), s0) and all(same(to_host(hp[k]), h0[k]) for k in h0)
    else:
        sd, hd = dev(s0), {k: dev(v) for k, v in h0.items()}
        m.evaluate(0.0, 1.0, gd, sd, td, hd)
    return to_host(sd), None if td is None else to_host(td), {k: to_host(v) for k, v in hd.items()}


def swift_port(g, s0, h0, max_iter=50):
    n = g.size // 9
    return swift_evaluate(SWIFT_P, mandel(g), s0.reshape(n, 6), h0["eps_n"].reshape(n, 6), h0["alpha"], max_iter=max_iter)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. VonMises3D in implicit form against the golden fixtures
# ---------------------------------------------------------------------------------------------------------------------------
GOLDEN = [(f, c) for f in ("von_mises_3d.npz", "random_parameters_von_mises_3d.npz", "von_mises_perfect_plasticity.npz")
          for c in load_calls(f)]


@pytest.mark.parametrize("path", ["ndarray", "tensor"])
@pytest.mark.parametrize("fname,c", GOLDEN, ids=[f"{f[:-4]}-{c.name}" for f, c in GOLDEN])
def test_von_mises_golden(fname, c, path):
    m = law("von_mises_3d_implicit", {k: c.params[k] for k in VM_P})
    s, t, h = c.fresh()
    if path == "ndarray":
        m.evaluate(0.0, c.del_t, c.grad.copy(), s, t, h)
    else:
        sd, td, hd = dev(s), dev(t), {k: dev(v) for k, v in h.items()}
        m.evaluate(0.0, c.del_t, dev(c.grad), sd, td, hd, check=True)
        s, t, h = to_host(sd), to_host(td), {k: to_host(v) for k, v in hd.items()}
    assert m.device_stats(0) == 0
    errs = {"stress": rel_err(s, c.stress_out), "tangent": rel_err(t, c.tangent_out), **{k: rel_err(h[k], c.hist_out[k]) for k in c.hist_out}}
    print(fname, c.name, path, errs)
    assert not np.isnan(t).any()
    assert all(e <= TOL["pl"] for e in errs.values()), errs


# ---------------------------------------------------------------------------------------------------------------------------
# 2. both Swift forms against the NumPy port
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", SWIFT_FORMS)
def test_swift_matches_numpy_port(form, n):
    g, s0, h0 = swift_inputs(n, 31 + n)
    m = law(form, SWIFT_P)
    s, _, h = run(m, g, s0, h0, tangent=False)
    assert m.device_stats(0) == 0
    s_np, e_np, a_np, status = swift_port(g, s0, h0)
    assert not status.any()
    plastic = a_np != h0["alpha"]
    if n >= 63:
        assert plastic.any() and (~plastic).any(), (plastic.sum(), n)
    errs = (rel_err(s, s_np.reshape(-1)), rel_err(h["eps_n"], e_np.reshape(-1)), rel_err(h["alpha"], a_np))
    print(form, n, "elastic / plastic", int((~plastic).sum()), int(plastic.sum()), "rel_err stress, eps_n, alpha", errs)
    assert max(errs) <= TOL["tight"], errs


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the linear probe: a zero diagonal at every elimination step, every N
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1000])
@pytest.mark.parametrize("unknowns", sorted({2, 3, 5, N_MAX}))
def test_linear_probe_pivots(unknowns, n):
    m, (A, B, c, M) = probe(unknowns)
    assert np.all(np.diag(A) == 0.0) and np.linalg.cond(A) < 10
    rng = np.random.default_rng(unknowns + n)
    g, s0 = rng.normal(scale=3e-3, size=9 * n), rng.normal(scale=30.0, size=6 * n)
    h0 = {"xs": np.full(unknowns * n, np.nan), "count": np.zeros(n)}
    s, t, h = run(m, g, s0, h0)
    assert m.device_stats(0) == 0
    x_ref, s_ref, D_ref = probe_expected(A, B, c, M, g, s0)
    errs = (rel_err(h["xs"], x_ref.reshape(-1)), rel_err(s, s_ref.reshape(-1)), rel_err(t, D_ref.reshape(-1)))
    print("probe", unknowns, n, "rel_err x, stress, tangent", errs)
    assert max(errs) <= TOL["port"], errs
    assert np.array_equal(h["count"], np.ones(n))
    s2, _, h2 = run(m, g, s0, h0, tangent=False)
    assert same(s, s2) and same(h["xs"], h2["xs"])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the consistent tangent
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tangent_case():
    """one call of 257 points, its tangents from both implicit forms and from the autodiff law"""
    n = 257
    g, s0, h0 = swift_inputs(n, 41)
    out = {"n": n, "in": (g, s0, h0)}
    for name in SWIFT_FORMS + ["von_mises_swift_ad"]:
        out[name] = run(law(name, SWIFT_P), g, s0, h0)
    out["plastic"] = out["von_mises_swift_ad"][2]["alpha"] != h0["alpha"]
    assert out["plastic"].any() and (~out["plastic"]).any()
    return out


@pytest.mark.parametrize("form", SWIFT_FORMS)
def test_swift_tangent_matches_finite_differences(tangent_case, form):
    """central differences of the law's own tangent=None launches: grad entries that change one Mandel strain at a time"""
    n = tangent_case["n"]
    g, s0, h0 = tangent_case["in"]
    m = law(form, SWIFT_P)
    D = tangent_case[form][1].reshape(n, 6, 6)
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
    print(form, "tangent against central differences", rel_err(D, fd))
    assert rel_err(D, fd) <= 1e-5, rel_err(D, fd)


@pytest.mark.parametrize("form", SWIFT_FORMS)
def test_swift_tangent_matches_the_autodiff_law(tangent_case, form):
    t, t_ad = tangent_case[form][1], tangent_case["von_mises_swift_ad"][1]
    print(form, "tangent against von_mises_swift_ad", rel_err(t, t_ad))
    assert rel_err(t, t_ad) <= 1e-6, rel_err(t, t_ad)


def test_elastic_tangents_are_symmetric_and_the_same_bits(tangent_case):
    n, elastic = tangent_case["n"], ~tangent_case["plastic"]
    D1 = tangent_case["von_mises_swift_implicit"][1].reshape(n, 6, 6)[elastic]
    D8 = tangent_case["von_mises_swift_general"][1].reshape(n, 6, 6)[elastic]
    assert same(D1, D1.transpose(0, 2, 1)) and same(D8, D8.transpose(0, 2, 1))
    assert same(D8, D1)
    assert same(D1, np.broadcast_to(D1[0], D1.shape))  # and one elastic matrix for all of them


# ---------------------------------------------------------------------------------------------------------------------------
# 5. bit identities
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", SWIFT_FORMS + ["von_mises_3d_implicit"])
def test_bit_identities(form):
    n = 1000
    g, s0, h0 = swift_inputs(n, 61)
    m = law(form, VM_P if form == "von_mises_3d_implicit" else SWIFT_P)
    s1, t1, h1 = run(m, g, s0, h0)
    assert m.device_stats(0) == 0
    # a tangent launch and a tangent=None launch
    s2, _, h2 = run(m, g, s0, h0, tangent=False)
    assert same(s1, s2) and all(same(h1[k], h2[k]) for k in h1)
    # ndarrays and tensors, in place and out of place (run_tensor checks the committed arrays)
    for out_of_place in (False, True):
        for tangent in (True, False):
            s3, t3, h3 = run_tensor(m, g, s0, h0, tangent=tangent, out_of_place=out_of_place)
            assert same(s1, s3) and all(same(h1[k], h3[k]) for k in h1) and (not tangent or same(t1, t3))
    # a point alone has the bits it has in the batch: a plastic one and an elastic one
    plastic = h1["alpha"] != h0["alpha"]
    assert plastic.any() and (~plastic).any()
    for k in (int(np.flatnonzero(plastic)[int(plastic.sum()) // 2]), int(np.flatnonzero(~plastic)[int((~plastic).sum()) // 2])):
        sk, tk, hk = run(m, g[9 * k:9 * k + 9], s0[6 * k:6 * k + 6], {"eps_n": h0["eps_n"][6 * k:6 * k + 6], "alpha": h0["alpha"][k:k + 1]})
        assert same(sk, s1[6 * k:6 * k + 6]) and same(tk, t1[36 * k:36 * k + 36])
        assert same(hk["eps_n"], h1["eps_n"][6 * k:6 * k + 6]) and same(hk["alpha"], h1["alpha"][k:k + 1])


# ---------------------------------------------------------------------------------------------------------------------------
# 6. non-convergence
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1000])
@pytest.mark.parametrize("form", SWIFT_FORMS)
def test_swift_non_convergence_count_is_exact(form, n):
    m = law(form, SWIFT_P, max_iter=1)
    g, s0, h0 = swift_inputs(n, 31 + n)
    expected = int(swift_port(g, s0, h0, max_iter=1)[3].sum())
    plastic = int((swift_port(g, s0, h0)[2] != h0["alpha"]).sum())
    print(form, n, "not converged after one step (NumPy port)", expected, "plastic", plastic)
    assert expected > 0
    for tangent in (None, torch.empty(36 * n, dtype=torch.float64, device=DEV)):
        hd = {k: dev(v) for k, v in h0.items()}
        m.evaluate(0.0, 1.0, dev(g), dev(s0), tangent, hd)
        assert m.device_stats(0) == expected
    s, h = s0.copy(), {k: v.copy() for k, v in h0.items()}
    with pytest.raises(RuntimeError, match=_capi.status_string(_capi.ERR_NONCONVERGED)):
        m.evaluate(0.0, 1.0, g, s, None, h)
    assert not same(s, s0) and not same(h["alpha"], h0["alpha"])  # the results are written before the error
    # a clean call resets the count
    clean = law(form, SWIFT_P)
    assert clean._compiled is m._compiled
    run(clean, g, s0, h0)
    assert clean.device_stats(0) == 0
    hd = {k: dev(v) for k, v in h0.items()}
    m.evaluate(0.0, 1.0, dev(0.0 * g), dev(0.0 * s0), None, hd)  # no strain, no stress: every point elastic
    assert m.device_stats(0) == 0


@pytest.mark.parametrize("n", [65, 1000])
def test_zero_jacobian_counts_every_point(n):
    m, _ = probe(3, zero_jacobian=True)
    rng = np.random.default_rng(n)
    g, s0 = rng.normal(scale=3e-3, size=9 * n), rng.normal(size=6 * n)
    for tangent in (None, torch.empty(36 * n, dtype=torch.float64, device=DEV)):
        hd = {"xs": torch.zeros(3 * n, dtype=torch.float64, device=DEV), "count": torch.zeros(n, dtype=torch.float64, device=DEV)}
        m.evaluate(0.0, 1.0, dev(g), dev(s0), tangent, hd)
        assert m.device_stats(0) == n
        assert np.array_equal(to_host(hd["count"]), np.ones(n))


@pytest.mark.parametrize("n", [65, 1000])
def test_start_code_two_counts_its_points_and_update_still_runs(n):
    m, (A, B, c, M) = probe(2, start="return eps[0] > 0.0 ? 2 : 1;")
    rng = np.random.default_rng(7 * n)
    g, s0 = rng.normal(scale=3e-3, size=9 * n), rng.normal(size=6 * n)
    refused = g.reshape(n, 9)[:, 0] > 0.0
    assert refused.any() and (~refused).any()
    h = {"xs": np.full(2 * n, np.nan), "count": np.zeros(n)}
    s = s0.copy()
    with pytest.raises(RuntimeError, match=_capi.status_string(_capi.ERR_NONCONVERGED)):
        m.evaluate(0.0, 1.0, g, s, None, h)
    assert m.device_stats(0) == int(refused.sum())
    assert np.array_equal(h["count"], np.ones(n))  # update ran at every point
    x_ref, s_ref, _ = probe_expected(A, B, c, M, g, s0)
    xs = h["xs"].reshape(n, 2)
    assert np.array_equal(xs[refused], np.zeros_like(xs[refused]))  # on the x that start gave
    assert same(s.reshape(n, 6)[refused], s0.reshape(n, 6)[refused] + 0.0)
    assert rel_err(xs[~refused], x_ref[~refused]) <= TOL["port"] and rel_err(s.reshape(n, 6)[~refused], s_ref[~refused]) <= TOL["port"]
    # a following clean call resets the count
    clean, _ = probe(2)
    run(clean, g, s0, {"xs": np.zeros(2 * n), "count": np.zeros(n)})
    assert clean.device_stats(0) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the wrappers
# ---------------------------------------------------------------------------------------------------------------------------
def jaumann_inputs(n, seed, symmetric):
    rng = np.random.default_rng(seed)
    g = rng.normal(scale=0.02 if not symmetric else 2e-3, size=(n, 3, 3))
    if symmetric:
        g = g + g.transpose(0, 2, 1)
    s0 = rng.normal(scale=1000.0, size=6 * n)
    h0 = {"eps_n": rng.normal(scale=1e-3, size=6 * n), "alpha": np.abs(rng.normal(scale=1e-3, size=n))}
    return g.reshape(-1), s0, h0


def test_jaumann_rate_with_a_symmetric_gradient_is_the_unwrapped_law():
    m = law("von_mises_swift_implicit", SWIFT_P)
    j = fc.JaumannRate(m, {"eps_n": [0]})
    assert j.path == "fused"
    g, s0, h0 = jaumann_inputs(1000, 11, symmetric=True)
    a, b = run(j, g, s0, h0), run(m, g, s0, h0)
    assert (b[2]["alpha"] != h0["alpha"]).any()
    assert same(a[0], b[0]) and same(a[1], b[1]) and all(same(a[2][k], b[2][k]) for k in h0)


def test_jaumann_rate_with_a_spinning_gradient():
    n = 500
    m = law("von_mises_swift_implicit", SWIFT_P)
    j, j_ad = fc.JaumannRate(m, {"eps_n": [0]}), fc.JaumannRate(law("von_mises_swift_ad", SWIFT_P), {"eps_n": [0]})
    assert j.path == "fused" and j_ad.path == "fused"
    g, s0, h0 = jaumann_inputs(n, 3, symmetric=False)
    a, b = run(j, g, s0, h0), run(j_ad, g, s0, h0)
    assert j.device_stats(0) == 0
    assert not same(a[0], run(m, g, s0, h0)[0])  # the rotation did something
    errs = (rel_err(a[0], b[0]), rel_err(a[1], b[1]), *(rel_err(a[2][k], b[2][k]) for k in h0))
    print("JaumannRate(implicit) against JaumannRate(autodiff)", errs)
    assert max(errs) <= 1e-6, errs
    # the NumPy rotation followed by the unwrapped law
    sr, hr = rotate_state(g, s0, h0, {"eps_n": [0]})
    ref = run(m, g, sr, hr)
    errs = (rel_err(a[0], ref[0]), rel_err(a[1], ref[1]), *(rel_err(a[2][k], ref[2][k]) for k in h0))
    print("JaumannRate(implicit) against rotate, then evaluate", errs)
    assert max(errs) <= 1e-12, errs


SEQS = [(k, name, calls) for k, name, calls in load_sequences() if name == "vm" and k == "plane_strain"]


@pytest.mark.parametrize("path", ["ndarray", "tensor"])
@pytest.mark.parametrize("kind,lname,calls", SEQS, ids=[k for k, _, _ in SEQS])
def test_plane_strain_wrapper_reproduces_golden(kind, lname, calls, path):
    w = fc.PlaneStrainFrom3D(law("von_mises_3d_implicit", VM_P))
    for c in calls:
        s, t = c["stress_in"].copy(), np.full_like(c["tangent_out"], np.nan)
        h = {k: v.copy() for k, v in c["hist_in"].items()}
        if path == "ndarray":
            w.evaluate(0.0, 2.0, c["grad"], s, t, h)
        else:
            sd, td, hd = dev(s), dev(t), {k: dev(v) for k, v in h.items()}
            w.evaluate(0.0, 2.0, dev(c["grad"]), sd, td, hd)
            s, t, h = to_host(sd), to_host(td), {k: to_host(v) for k, v in hd.items()}
        errs = (rel_err(s, c["stress_out"]), rel_err(t, c["tangent_out"]), *(rel_err(h[k], c["hist_out"][k]) for k in h))
        assert max(errs) <= TOL["pl"], errs


def test_the_wrapper_cases_exist():
    assert len(SEQS) >= 1
