"""GPU checks of the fused wrapper kernel of user laws (csrc/jit/user_law_wrapped.hip): the four ``*From3D`` wrappers around a
``UserLaw`` with an explicit or autodiff tangent as one launch -- the strain wrappers bit for bit against map -> evaluate -> map,
the stress wrappers against the NumPy model of the rule with the zero start (tests/stress_wrapper_util.py, ``elastic=None``) and
against the generic path, the independence of a point from the rest of its wave, failure reporting, the reference's
uniaxial-stress curves and the example."""

import os
import subprocess
import sys

import numpy as np
import pytest
from golden_util import GOLDEN, rel_err
from material_point import HostState, MaterialPoints
from stress_wrapper_util import LE_P, VM_P, StressFrom3DOracle
from user_law_wrapped_util import NS, ORACLE, history_dims, strain_calls, stress_calls, user_law
from wrappers_util import PARAMS, load_sequences

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import jit  # noqa: E402
from fenics_constitutive_amd import userlaw_sources as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("FCAMD_SMALL_CALL_WARNING", "0")
STRAIN = {"plane_strain": fc.PlaneStrainFrom3D, "uniaxial_strain": fc.UniaxialStrainFrom3D}
STRESS = {"PLANE_STRESS": fc.PlaneStressFrom3D, "UNIAXIAL_STRESS": fc.UniaxialStressFrom3D}
ALL = {**STRAIN, **STRESS}
STRAIN_LAWS = ("le", "maxwell", "vm", "le_ad", "maxwell_ad", "vm_ad", "swift_ad")
STRESS_LAWS = ("le", "maxwell", "vm", "le_ad", "maxwell_ad", "vm_ad")
N_SECOND_TRIP = 131072 + 64 + 5  # one CU's worth of blocks: every wave makes a second trip and the ragged tile falls on it


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def host(x):
    return x.cpu().numpy()


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class Run:
    """one wrapper over a sequence of calls on buffers of its own, tensors or ndarrays; ``out()`` is the host copy of everything a
    call leaves: mapped stress, tangent, history and the cached 3-D stress"""

    def __init__(self, w, s0, h0, tensors=True):
        self.w, self.tensors = w, tensors
        self.sd = w.stress_strain_dim
        self.n = s0.size // self.sd
        up = dev if tensors else (lambda x: x.copy())
        self.s, self.h = up(s0), None if h0 is None else {k: up(v) for k, v in h0.items()}
        self.t = up(np.full(self.sd * self.sd * self.n, np.nan))

    def call(self, del_t, g):
        self.w.evaluate(0.0, del_t, dev(g) if self.tensors else g, self.s, self.t, self.h)
        return self.out()

    def out(self):
        get = host if self.tensors else (lambda x: x.copy())
        o = {"stress": get(self.s), "tangent": get(self.t), "stress_3d": host(self.w.stress_3d).reshape(self.n, 6)}
        o.update({k: get(v) for k, v in (self.h or {}).items()})
        return o


def assert_fused(w):
    assert w.grad_del_u_3d is None and w.tangent_3d is None and w.stress_3d is not None


# --- 1. strain wrappers: the bits of map -> evaluate -> map -------------------------------------------------------------------

def _strain_pair(kind, lname, n, tensors):
    s0, h0, grads = strain_calls(kind, lname, n)
    a, b = STRAIN[kind](user_law(lname)), STRAIN[kind](user_law(lname))
    b.fused = False
    ra, rb = Run(a, s0, h0, tensors), Run(b, s0, h0, tensors)
    for call, g in enumerate(grads):
        oa, ob = ra.call(1.0, g), rb.call(1.0, g)
        for k in oa:
            assert same(oa[k], ob[k]), (kind, lname, n, call, k, rel(oa[k], ob[k]))
        assert a.model.device_stats(0) == 0
    assert_fused(a)
    assert b.tangent_3d is not None
    return ra


@pytest.mark.parametrize("tensors", [True, False], ids=["tensor", "ndarray"])
@pytest.mark.parametrize("lname", STRAIN_LAWS)
@pytest.mark.parametrize("kind", sorted(STRAIN))
def test_strain_wrappers_are_map_evaluate_map_bit_for_bit(kind, lname, tensors):
    for n in NS:
        ra = _strain_pair(kind, lname, n, tensors)
    if history_dims(lname) and "alpha" in history_dims(lname):
        assert np.any(ra.out()["alpha"] > strain_calls(kind, lname, NS[-1])[1]["alpha"])  # the plastic range is reached


@pytest.mark.parametrize("lname", ["vm", "vm_ad"])
@pytest.mark.parametrize("kind", sorted(STRAIN))
def test_strain_wrappers_on_a_second_grid_trip(kind, lname, monkeypatch):
    monkeypatch.setattr(jit, "num_cu", lambda device: 1)
    _strain_pair(kind, lname, N_SECOND_TRIP, True)


SEQS = load_sequences()
GOLDEN_TOL = {"le": 1e-10, "maxwell": 1e-10, "vm": 1e-6}  # test_gpu_wrappers.py: TOL
GOLDEN_LAWS = {"le": S.linear_elasticity, "maxwell": S.spring_maxwell, "vm": S.von_mises_3d,
               "le_ad": S.linear_elasticity_ad, "maxwell_ad": S.spring_maxwell_ad, "vm_ad": S.von_mises_3d_ad}


@pytest.mark.parametrize("mode", ["", "_ad"], ids=["explicit", "autodiff"])
@pytest.mark.parametrize("kind,lname,calls", SEQS, ids=[f"{k}-{name}" for k, name, _ in SEQS])
def test_strain_wrappers_reproduce_the_reference_sequences(kind, lname, calls, mode):
    w = STRAIN[kind](GOLDEN_LAWS[lname + mode](PARAMS[lname]))
    tol = GOLDEN_TOL[lname]
    for c in calls:
        s, t = dev(c["stress_in"]), dev(np.full_like(c["tangent_out"], np.nan))
        h = None if c["hist_in"] is None else {k: dev(v) for k, v in c["hist_in"].items()}
        w.evaluate(0.0, 2.0, dev(c["grad"]), s, t, h)
        assert rel_err(host(s), c["stress_out"]) <= tol and rel_err(host(t), c["tangent_out"]) <= tol
        for k in (h or {}):
            assert rel_err(host(h[k]), c["hist_out"][k]) <= tol, k
    assert_fused(w)


# --- 2. stress wrappers against the NumPy rule with the zero start ------------------------------------------------------------

def _residual_ok(constraint, s3):
    b = [2] if constraint == "PLANE_STRESS" else [1, 2]
    r = np.max(np.abs(s3[:, b]), axis=1)
    return np.all((r == 0) | (r <= 1e-12 * np.linalg.norm(s3, axis=1) * (1 + 1e-9)))


def _assert_plane_stress_zeros(o, n):
    assert np.all(o["stress"].reshape(n, 4)[:, 2] == 0.0)
    tt = o["tangent"].reshape(n, 4, 4)
    assert np.all(tt[:, 2, :] == 0.0) and np.all(tt[:, :, 2] == 0.0)


_oracle_cache = {}


def oracle_outputs(constraint, lname, n):
    """the NumPy rule over the call sequence, computed once per case: [outputs after each call]"""
    key = (constraint, lname, n)
    if key not in _oracle_cache:
        fn, params, hdims, _, _ = ORACLE[lname]
        o = StressFrom3DOracle(constraint, "", fn, params, hdims, None)
        s0, h0, calls = stress_calls(constraint, lname, n)
        sd = 4 if constraint == "PLANE_STRESS" else 1
        s, t = s0.copy(), np.zeros(sd * sd * n)
        h = None if h0 is None else {k: v.copy() for k, v in h0.items()}
        outs = []
        for del_t, g in calls:
            o.evaluate(0.0, del_t, g, s, t, h)
            assert not o.failed.any() and o.evaluations.max() <= 5
            out = {"stress": s.copy(), "tangent": t.copy(), "stress_3d": o.stress_3d.copy()}
            out.update({k: v.copy() for k, v in (h or {}).items()})
            outs.append(out)
        _oracle_cache[key] = outs
    return _oracle_cache[key]


@pytest.mark.parametrize("tensors", [True, False], ids=["tensor", "ndarray"])
@pytest.mark.parametrize("lname", STRESS_LAWS)
@pytest.mark.parametrize("constraint", sorted(STRESS))
def test_stress_wrappers_follow_the_rule_and_the_generic_path(constraint, lname, tensors):
    """against the NumPy model of the rule at the project's tolerance of the law, against ``fused = False`` at 1e-10 ("two runs of
    the same rule": the torch norm and the kernel's may decide a borderline iteration differently)"""
    base = lname.replace("_ad", "")
    tol = ORACLE[base][4]
    for n in NS:
        s0, h0, calls = stress_calls(constraint, base, n)
        a, b = STRESS[constraint](user_law(lname)), STRESS[constraint](user_law(lname))
        b.fused = False
        ra, rb = Run(a, s0, h0, tensors), Run(b, s0, h0, tensors)
        for call, ((del_t, g), oo) in enumerate(zip(calls, oracle_outputs(constraint, base, n))):
            oa, ob = ra.call(del_t, g), rb.call(del_t, g)
            assert a.model.device_stats(0) == 0
            worst = {k: (rel(oa[k], oo[k]), rel(oa[k], ob[k])) for k in oa}
            print(constraint, lname, n, call, worst)
            for k in oa:
                assert worst[k][0] <= tol, (n, call, k, worst[k])
                assert worst[k][1] <= 1e-10, (n, call, k, worst[k])
            assert _residual_ok(constraint, oa["stress_3d"])
            if constraint == "PLANE_STRESS":
                _assert_plane_stress_zeros(oa, n)
        assert_fused(a)
        assert b.tangent_3d is not None


@pytest.mark.parametrize("base", ["le", "maxwell", "vm"])
@pytest.mark.parametrize("constraint", sorted(STRESS))
def test_stress_wrappers_explicit_and_autodiff_agree(constraint, base):
    """the bound of test_gpu_user_law_autodiff.py::test_plane_stress_of_von_mises_autodiff"""
    n = NS[-1]
    s0, h0, calls = stress_calls(constraint, base, n)
    ra, rb = Run(STRESS[constraint](user_law(base)), s0, h0), Run(STRESS[constraint](user_law(base + "_ad")), s0, h0)
    for del_t, g in calls:
        oa, ob = ra.call(del_t, g), rb.call(del_t, g)
        for k in oa:
            assert rel(oa[k], ob[k]) <= 1e-8, (k, rel(oa[k], ob[k]))


@pytest.mark.parametrize("lname", ["vm", "vm_ad"])
@pytest.mark.parametrize("constraint", sorted(STRESS))
def test_stress_wrappers_on_a_second_grid_trip(constraint, lname, monkeypatch):
    """The points are those of the n = 257 case, repeated: point i has the inputs of point i % 257.  The test is about the
    grid-stride loop and the ragged tile, and the 257 points are the ones the rule is known to converge on (oracle_outputs: no
    failure, at most 5 evaluations).  A fresh random draw of 131141 points is no such set: the criterion is relative to |sigma|_2,
    so under uniaxial stress a point whose axial stress happens to cancel to ~1e-3 of the stress scale has a bound below the
    round-off of its lateral stresses, and the rule itself -- the NumPy model and the generic path as much as the kernel -- runs
    such a point to 50 evaluations.  With repeated points every row of the large launch must also be, bit for bit, the row the
    n = 257 launch gives that point."""
    monkeypatch.setattr(jit, "num_cu", lambda device: 1)
    n, m = N_SECOND_TRIP, NS[-1]
    assert (n + 63) // 64 > 4 * 512  # more tiles than the capped grid has waves
    sd = 4 if constraint == "PLANE_STRESS" else 1
    dims = {"stress": sd, "tangent": sd * sd, "stress_3d": 6, "eps_n": 6, "alpha": 1}
    src = np.arange(n) % m

    def tiled(x, width):
        return np.ascontiguousarray(x.reshape(m, width)[src]).reshape(-1)

    s0, h0, calls = stress_calls(constraint, "vm", m)
    big_s0, big_h0 = tiled(s0, sd), {k: tiled(v, dims[k]) for k, v in h0.items()}
    a, b, c = (STRESS[constraint](user_law(lname)) for _ in range(3))
    b.fused = False
    ra, rb, rc = Run(a, big_s0, big_h0), Run(b, big_s0, big_h0), Run(c, s0, h0)
    for (del_t, g), oo in list(zip(calls, oracle_outputs(constraint, "vm", m)))[:2]:
        big_g = tiled(g, sd)
        oa, ob, oc = ra.call(del_t, big_g), rb.call(del_t, big_g), rc.call(del_t, g)
        assert a.model.device_stats(0) == 0
        for k in oa:
            assert same(oa[k].reshape(-1), tiled(oc[k], dims[k])), k
            assert rel(oa[k], ob[k]) <= 1e-10, (k, rel(oa[k], ob[k]))
            assert rel(oa[k].reshape(-1), tiled(oo[k], dims[k])) <= ORACLE["vm"][4], k
        assert _residual_ok(constraint, oa["stress_3d"])
        if constraint == "PLANE_STRESS":
            _assert_plane_stress_zeros(oa, n)
    assert_fused(a)


# --- 3. a point does not depend on the rest of its wave -----------------------------------------------------------------------

@pytest.mark.parametrize("lname", ["vm", "vm_ad"])
@pytest.mark.parametrize("kind", sorted(ALL))
def test_a_point_alone_has_the_bits_it_has_among_others(kind, lname):
    n = 65
    stress = kind in STRESS
    s0, h0, calls = stress_calls(kind, "vm", n) if stress else strain_calls(kind, "vm", n)
    calls = calls if stress else [(1.0, g) for g in calls]
    sd = ALL[kind](user_law(lname)).stress_strain_dim
    gd2 = 1 if sd == 1 else 4
    crowd = Run(ALL[kind](user_law(lname)), s0, h0)
    crowd_out = [crowd.call(del_t, g) for del_t, g in calls]
    alpha0, alpha1 = h0["alpha"], crowd_out[-1]["alpha"]
    plastic = alpha1 > alpha0
    assert plastic.any() and not plastic.all()  # elastic and plastic points mixed
    picks = {int(np.flatnonzero(plastic)[0]), int(np.flatnonzero(~plastic)[0]), 64}  # 64: alone in the ragged tile of the crowd
    dims = {"stress": sd, "tangent": sd * sd, "stress_3d": 6, "eps_n": 6, "alpha": 1}
    for i in sorted(picks):
        alone = Run(ALL[kind](user_law(lname)), s0.reshape(n, sd)[i].copy(), {k: v.reshape(n, -1)[i].copy() for k, v in h0.items()})
        for (del_t, g), oc in zip(calls, crowd_out):
            oa = alone.call(del_t, g.reshape(n, gd2)[i].copy())
            for k in oa:
                assert same(oa[k].reshape(-1), oc[k].reshape(n, dims[k])[i]), (kind, lname, i, k)


# --- 4. failure reporting -----------------------------------------------------------------------------------------------------

# LINEAR_ELASTICITY with two switches: a point whose eps_xx exceeds `fail_above` returns 1, one whose eps_xx exceeds
# `singular_above` hands out a tangent of zeros (a singular C_bb for the stress wrappers)
PROBE = S.LINEAR_ELASTICITY.replace("    return 0;", """    if (eps[0] > p.singular_above)
        for (int i = 0; i < 36; ++i) D[i] = 0.0;
    return eps[0] > p.fail_above ? 1 : 0;""")
BIG = 1e300


def probe_law(fail_above=BIG, singular_above=BIG):
    return fc.UserLaw(PROBE, dict(LE_P, fail_above=fail_above, singular_above=singular_above), None, name="wrapped_probe")


def _probe_inputs(kind, n, seed=5):
    rng = np.random.default_rng(seed)
    sd = ALL[kind](probe_law()).stress_strain_dim
    gd2 = 1 if sd == 1 else 4
    g = rng.normal(scale=1e-2, size=gd2 * n)
    s0 = rng.normal(size=sd * n)
    return sd, gd2, g, s0


@pytest.mark.parametrize("kind", sorted(ALL))
def test_a_failing_point_function_is_counted_and_reported(kind):
    assert "p.fail_above" in PROBE
    n = 257
    sd, gd2, g, s0 = _probe_inputs(kind, n)
    expected = int(np.sum(g.reshape(n, gd2)[:, 0] > 0.0))
    assert 0 < expected < n
    good = Run(ALL[kind](probe_law()), s0, None).call(1.0, g)
    # tensors: no raise, the count in device_stats
    r = Run(ALL[kind](probe_law(fail_above=0.0)), s0, None)
    out = r.call(1.0, g)
    assert r.w.model.device_stats(0) == expected
    for k in out:
        assert same(out[k], good[k]), k  # the return code changes nothing else
    # ndarrays: the results are written, then the reference's RuntimeError
    r = Run(ALL[kind](probe_law(fail_above=0.0)), s0, None, tensors=False)
    with pytest.raises(RuntimeError, match=jit.NONCONVERGED_MESSAGE):
        r.call(1.0, g)
    out = r.out()
    for k in out:
        assert same(out[k], good[k]), k
    # and a law that reports nothing raises nothing
    Run(ALL[kind](probe_law()), s0, None, tensors=False).call(1.0, g)


@pytest.mark.parametrize("kind", sorted(STRESS))
def test_a_singular_tangent_block_fails_the_point_and_no_other(kind):
    n = 257
    sd, gd2, g, s0 = _probe_inputs(kind, n, seed=6)
    singular = g.reshape(n, gd2)[:, 0] > 0.0
    good = Run(ALL[kind](probe_law()), s0, None).call(1.0, g)
    r = Run(ALL[kind](probe_law(singular_above=0.0)), s0, None)
    out = r.call(1.0, g)
    assert r.w.model.device_stats(0) == int(singular.sum())
    assert np.all(np.isfinite(out["stress"])) and np.all(np.isfinite(out["stress_3d"]))
    for k in out:
        width = out[k].size // n
        assert same(out[k].reshape(n, width)[~singular], good[k].reshape(n, width)[~singular]), k
    # the failed points keep the zero increment: their row is the one evaluation from the committed state
    assert not _residual_ok(kind, out["stress_3d"][singular])
    # a tangent of zeros everywhere: every point counts
    r = Run(ALL[kind](probe_law(singular_above=-BIG)), s0, None)
    out = r.call(1.0, g)
    assert r.w.model.device_stats(0) == n
    assert np.all(np.isfinite(out["stress"])) and np.all(np.isfinite(out["stress_3d"]))
    with pytest.raises(RuntimeError, match=jit.NONCONVERGED_MESSAGE):
        Run(ALL[kind](probe_law(singular_above=-BIG)), s0, None, tensors=False).call(1.0, g)


# --- 5. the reference's uniaxial-stress curves --------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["host", "torch"])
@pytest.mark.parametrize("lname", ["vm", "vm_ad"])
@pytest.mark.parametrize("case", ["uniaxial_stress_3d", "uniaxial_cyclic_strain_3d"])
def test_von_mises_uniaxial_stress_curves(case, lname, path):
    """test_gpu_stress_wrappers.py::test_von_mises_uniaxial_stress_curves through the user law, at its bound"""
    z = np.load(os.path.join(GOLDEN, "material_point.npz"))
    disp, load = z[case + ".disp"], z[case + ".load"]
    n = disp.shape[1]
    w = fc.UniaxialStressFrom3D(user_law(lname))
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
            w.evaluate(0.0, 1.0, dev(disp[k] - disp[k - 1]), s_t, t, h_t)
            assert w.model.device_stats(0) == 0
            s_c.copy_(s_t)
            h_c = h_t
            out.append(host(s_t))
    assert_fused(w)
    assert np.max(np.abs(np.array(out) - load)) <= 1e-9 * VM_P["p_y0"]


# --- 6. the example -----------------------------------------------------------------------------------------------------------

def test_the_plane_stress_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "user_law_plane_stress.py"), "2000"], capture_output=True,
                         text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plane stress" in out.stdout and "uniaxial stress" in out.stdout and "OK" in out.stdout, out.stdout
