"""Per-point parameter fields on the GPU (FCAMD_EVAL_PARAM_FIELDS, evaluate_fields_kernel): a constant field gives the
bits of the scalar law, scattered parameter groups give the bits of one scalar law per group, continuous fields match the
NumPy oracle point by point and their tangent matches finite differences, non-convergence is reported, and every form
without field support refuses before anything is launched."""

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import _capi  # noqa: E402
from fenics_constitutive_amd.interfaces import StressStrainConstraint as S  # noqa: E402
from fenics_constitutive_amd.multidevice import MultiDeviceResidentState  # noqa: E402
from fenics_constitutive_amd.problem import ResidentProblemState  # noqa: E402
from fenics_constitutive_amd.resident import ResidentState  # noqa: E402
from golden_util import rel_err  # noqa: E402
from oracle import numpy_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
# law name -> (constructor, scalar parameters, the parameters in the model's order, oracle kind)
LAWS = {
    "LinearElasticityModel": (lambda p: fc.LinearElasticityModel(p, S.FULL), {"E": 210000.0, "nu": 0.3}, ("E", "nu"), "linear_elasticity"),
    "LinearElasticity3D": (fc.LinearElasticity3D, {"mu": 80769.0, "kappa": 175000.0}, ("mu", "kappa"), "comfe_linear_elasticity"),
    "VonMises3D": (fc.VonMises3D, {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 250.0, "p_y00": 2500.0, "p_w": 200.0},
                   ("p_ka", "p_mu", "p_y0", "p_y00", "p_w"), "von_mises_3d"),
    "MisesPlasticityLinearHardening3D": (fc.MisesPlasticityLinearHardening3D, {"mu": 80769.0, "kappa": 175000.0, "y_0": 250.0, "h": 1000.0},
                                         ("mu", "kappa", "y_0", "h"), "comfe_mises_plasticity"),
}
COMFE = ("LinearElasticity3D", "MisesPlasticityLinearHardening3D")


def make(name, params):
    """the law with these parameters (scalars: as the reference passes them -- one-element arrays for the comfe-rs laws)"""
    ctor = LAWS[name][0]
    if name in COMFE:
        params = {k: (v if isinstance(v, np.ndarray) else np.array([float(v)])) for k, v in params.items()}
    return ctor(params)


def grads(n, seed, steps=3):
    """gradient mix: log-uniform magnitudes, about a fifth of the points plastic for the Mises laws"""
    rng = np.random.default_rng(seed)
    scale = 10 ** rng.uniform(-4.5, -2.8, size=n)
    return [rng.normal(size=9 * n) * np.repeat(scale, 9) for _ in range(steps)]


def hist_zeros(law, n, like):
    hd = law.history_dim
    if hd is None:
        return None
    if isinstance(like, np.ndarray):
        return {k: np.zeros(d * n) for k, d in hd.items()}
    return {k: torch.zeros(d * n, dtype=torch.float64, device=DEV) for k, d in hd.items()}


def bits(x):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return a.view(np.int64)


def assert_same_bits(a, b, what=""):
    ba, bb = bits(a), bits(b)
    bad = np.flatnonzero(ba != bb)
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first at {bad[:5]}"


def run_in_place(law, gs, n, numpy_arrays):
    """three load steps with commits (the reference's in-place protocol)"""
    if numpy_arrays:
        s, t = np.zeros(6 * n), np.zeros(36 * n)
        h = hist_zeros(law, n, s)
        for g in gs:
            law.evaluate(0.0, 1.0, g.copy(), s, t, h)
    else:
        s, t = torch.zeros(6 * n, dtype=torch.float64, device=DEV), torch.zeros(36 * n, dtype=torch.float64, device=DEV)
        h = hist_zeros(law, n, s)
        for g in gs:
            law.evaluate(0.0, 1.0, torch.from_numpy(g).to(DEV), s, t, h, check=True)
        torch.cuda.synchronize()
    return s, t, h


def run_resident(law, gs, n, **kw):
    """increments of two Newton evaluates each, committed -- what a device assembler does"""
    st = ResidentState(law, n, **kw)
    for k, g in enumerate(gs):
        st.evaluate(0.0, 1.0, torch.from_numpy(0.5 * g).to(DEV))
        st.evaluate(0.0, 1.0, torch.from_numpy(g).to(DEV))
        if k < len(gs) - 1:
            st.update()
    torch.cuda.synchronize()
    h = st.history
    return st.stress.clone(), st.tangent.clone(), None if h is None else {k: v.clone() for k, v in h.items()}


def run_resident_into(law, gs, n, after_call=lambda stats: None):
    """the host assembler's form: NumPy gradient in, the trial stress / tangent into NumPy arrays (fcamd_evaluate_resident)"""
    st = ResidentState(law, n)
    s, t = np.zeros(6 * n), np.zeros(36 * n)
    for k, g in enumerate(gs):
        after_call(st.evaluate_into(0.0, 1.0, 0.5 * g, s, t))
        after_call(st.evaluate_into(0.0, 1.0, g, s, t))
        if k < len(gs) - 1:
            st.update()
    h = st.history
    return s, t, None if h is None else {k: v.clone() for k, v in h.items()}


def compare_runs(a, b, what, rows=None):
    sa, ta, ha = a
    sb, tb, hb = b
    pick = (lambda x, d: x) if rows is None else (lambda x, d: x.reshape(-1, d)[rows].reshape(-1))
    assert_same_bits(pick(sa, 6), sb, what + " stress")
    assert_same_bits(pick(ta, 36), tb, what + " tangent")
    if ha is not None:
        for k in ha:
            size = lambda x: x.numel() if torch.is_tensor(x) else x.size  # noqa: E731
            d = size(ha[k]) // (size(sa) // 6)
            assert_same_bits(pick(ha[k], d), hb[k], what + f" history[{k}]")


def plastic_fraction(law, gs, n):
    if type(law).__name__ not in ("VonMises3D", "MisesPlasticityLinearHardening3D"):
        return None
    run_in_place(law, gs[:1], n, False)
    return law.device_stats().n_plastic / n


# --- 1. a constant field is the scalar law, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 4099])
@pytest.mark.parametrize("name", list(LAWS))
def test_constant_field_equals_scalar(name, n):
    scal = LAWS[name][1]
    gs = grads(n, 11 + n)
    ref = make(name, scal)
    fld = make(name, {k: np.full(n, float(v)) for k, v in scal.items()})  # every parameter a field
    assert fld.field_points == n
    frac = plastic_fraction(ref, gs, n)
    if frac is not None:
        assert 0.05 < frac < 0.5, frac
    for numpy_arrays in (False, True):
        compare_runs(run_in_place(fld, gs, n, numpy_arrays), run_in_place(ref, gs, n, numpy_arrays), f"{name} numpy={numpy_arrays}")
    compare_runs(run_resident(fld, gs, n), run_resident(ref, gs, n), f"{name} ResidentState")
    compare_runs(run_resident_into(fld, gs, n), run_resident_into(ref, gs, n), f"{name} ResidentState.evaluate_into")
    # one field among scalars
    one = make(name, dict(scal, **{LAWS[name][2][-1]: np.full(n, float(scal[LAWS[name][2][-1]]))}))
    compare_runs(run_in_place(one, gs, n, False), run_in_place(ref, gs, n, False), f"{name} one field")


# --- 1b. the chunked pass of fcamd_evaluate_resident takes every chunk's fields at the chunk's first point -----------
@pytest.mark.parametrize("name", ["LinearElasticityModel", "VonMises3D"])
def test_fields_through_the_chunked_resident_pass(name):
    """n = 357 (five tiles and a ragged tail of 37) in chunks of 128 points -- the fields of the three launches start at points 0, 128
    and 256 -- gives the bits of the default path's single launch.  The fields differ at every point: a chunk that read them from a
    wrong offset would change every value of the chunk."""
    n = 357
    p = random_fields(name, n, np.random.default_rng(13))
    assert all(np.unique(v).size == n for v in p.values() if isinstance(v, np.ndarray))
    law = make(name, p)
    gs = [3.0 * g for g in grads(n, 17)]
    ref = run_resident_into(law, gs, n)
    ctx = law._handle(_capi.default_device()).ctx
    modes, plastic = [], []

    def after_call(stats):
        modes.append(ctx.last_host_mode())
        plastic.append(stats.n_plastic)

    ctx.set_option("bounce_max", 0), ctx.set_option("zero_copy", 0), ctx.set_option("host_chunk", 128)
    try:
        got = run_resident_into(law, gs, n, after_call)
    finally:
        ctx.set_option("bounce_max", 256 << 10), ctx.set_option("zero_copy", 1), ctx.set_option("host_chunk", 0)
    assert modes == [_capi.HOST_TEMP_LOCK] * (2 * len(gs)), modes
    assert name != "VonMises3D" or max(plastic) > 0
    compare_runs(got, ref, f"{name} chunked evaluate_into")


# --- 2. scattered parameter groups are one scalar law per group, bit for bit -------------------------------------
GROUPS = {
    "LinearElasticityModel": [{"E": 210000.0, "nu": 0.3}, {"E": 70000.0, "nu": 0.33}, {"E": 30000.0, "nu": 0.2}, {"E": 1000.0, "nu": 0.45}],
    "LinearElasticity3D": [{"mu": 80769.0, "kappa": 175000.0}, {"mu": 26000.0, "kappa": 68000.0}, {"mu": 12500.0, "kappa": 16700.0},
                           {"mu": 300.0, "kappa": 3300.0}],
    "VonMises3D": [{"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 250.0, "p_y00": 2500.0, "p_w": 200.0},
                   {"p_ka": 68000.0, "p_mu": 26000.0, "p_y0": 120.0, "p_y00": 400.0, "p_w": 50.0},
                   {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 600.0, "p_y00": 900.0, "p_w": 10.0},
                   {"p_ka": 16700.0, "p_mu": 12500.0, "p_y0": 30.0, "p_y00": 60.0, "p_w": 500.0}],
    "MisesPlasticityLinearHardening3D": [{"mu": 80769.0, "kappa": 175000.0, "y_0": 250.0, "h": 1000.0},
                                         {"mu": 26000.0, "kappa": 68000.0, "y_0": 120.0, "h": 0.0},
                                         {"mu": 80769.0, "kappa": 175000.0, "y_0": 600.0, "h": 20000.0},
                                         {"mu": 12500.0, "kappa": 16700.0, "y_0": 30.0, "h": 300.0}],
}


@pytest.mark.parametrize("defaults", [True, False], ids=["sparse_packed_split", "dense"])
@pytest.mark.parametrize("name", list(LAWS))
def test_scattered_groups_equal_per_group_scalar_laws(name, defaults):
    n = 4099
    rng = np.random.default_rng(5)
    group = rng.integers(0, 4, size=n)
    sets = GROUPS[name]
    fields = {k: np.array([sets[gi][k] for gi in range(4)])[group] for k in sets[0]}
    law = make(name, fields)
    assert law.field_points == n
    gs = grads(n, 21)
    kw = {} if defaults else dict(sparse_history=False, sparse_tangent=False, packed_history=False, split_history=False,
                                  reuse_constant_tangent=False)
    got = run_resident(law, gs, n, **kw)
    for gi in range(4):
        rows = np.flatnonzero(group == gi)
        sub = [g.reshape(n, 9)[rows].reshape(-1) for g in gs]
        ref = run_resident(make(name, sets[gi]), sub, rows.size, **kw)
        compare_runs(got, ref, f"{name} group {gi}", rows=torch.from_numpy(rows).to(DEV))


# --- 3. continuous random fields against the NumPy oracle; the tangent against central differences ---------------
def lognormal(rng, center, n):
    return center * 10 ** rng.uniform(-1.0, 1.0, size=n)  # two decades


def random_fields(name, n, rng):
    p = dict(LAWS[name][1])
    if name == "LinearElasticityModel":
        p["E"] = lognormal(rng, 210000.0, n)
    elif name == "LinearElasticity3D":
        p["mu"] = lognormal(rng, 80769.0, n)
    elif name == "VonMises3D":
        p["p_mu"], p["p_y0"] = lognormal(rng, 80769.0, n), lognormal(rng, 250.0, n)
    else:
        p["mu"], p["y_0"] = lognormal(rng, 80769.0, n), lognormal(rng, 250.0, n)
    return p


def oracle_per_point(name, p, g, s, h, n):
    kind = LAWS[name][3]
    s, t = s.copy(), np.zeros(36 * n)
    h = None if h is None else {k: v.copy() for k, v in h.items()}
    for i in range(n):
        pi = {k: (float(v[i]) if isinstance(v, np.ndarray) else float(v)) for k, v in p.items()}
        if name in COMFE:
            pi = {k: np.array([v]) for k, v in pi.items()}
        hi = None if h is None else {k: v.reshape(n, -1)[i].copy() for k, v in h.items()}
        si, ti = s.reshape(n, 6)[i].copy(), t.reshape(n, 36)[i].copy()
        O.MODELS[kind](pi, 0.0, 1.0, g.reshape(n, 9)[i].copy(), si, ti, hi)
        s.reshape(n, 6)[i], t.reshape(n, 36)[i] = si, ti
        if h is not None:
            for k in h:
                h[k].reshape(n, -1)[i] = hi[k]
    return s, t, h


@pytest.mark.parametrize("name", list(LAWS))
def test_random_fields_match_the_oracle(name):
    n = 300
    rng = np.random.default_rng(7)
    p = random_fields(name, n, rng)
    law = make(name, p)
    g = grads(n, 3, steps=1)[0] * 3.0
    s0 = np.zeros(6 * n)
    h0 = hist_zeros(law, n, s0)
    s, t, h = run_in_place(law, [g], n, True)
    rs, rt, rh = oracle_per_point(name, p, g, s0, h0, n)
    tol = 1e-10 if "Elastic" in name else 1e-6  # the existing parity tests' (tests/test_gpu_parity.py: TOL)
    assert rel_err(s, rs) <= tol and rel_err(t, rt) <= tol, (rel_err(s, rs), rel_err(t, rt))
    if h is not None:
        for k in h:
            assert rel_err(h[k], rh[k]) <= tol, (k, rel_err(h[k], rh[k]))


# (not MisesPlasticityLinearHardening3D: the reference's own tangent for it, 2 mu theta_bar n n^T with the non-unit n, is not the
# derivative of its stress update -- the NumPy oracle of the scalar law differs from central differences by ~17 % at plastic points;
# test_random_fields_match_the_oracle holds the field kernel to that tangent)
@pytest.mark.parametrize("name", ["VonMises3D", "LinearElasticityModel", "LinearElasticity3D"])
def test_field_tangent_matches_central_differences(name):
    n = 64
    rng = np.random.default_rng(9)
    law = make(name, random_fields(name, n, rng))
    f = 1.0 / 2**0.5
    e = rng.normal(size=(n, 6)) * 10 ** rng.uniform(-4, -2.5, size=(n, 1))

    def grad_of(eps):
        g = np.zeros((n, 9))
        g[:, 0], g[:, 4], g[:, 8] = eps[:, 0], eps[:, 1], eps[:, 2]
        g[:, 1] = g[:, 3] = eps[:, 3] / (2 * f)
        g[:, 2] = g[:, 6] = eps[:, 4] / (2 * f)
        g[:, 5] = g[:, 7] = eps[:, 5] / (2 * f)
        return g.reshape(-1)

    def stress(eps):
        s, t, _ = run_in_place(law, [grad_of(eps)], n, True)
        return s.reshape(n, 6), t.reshape(n, 6, 6)

    _, T = stress(e)
    fd = np.zeros((n, 6, 6))
    for c in range(6):
        hstep = 1e-7 * np.maximum(np.abs(e).max(axis=1), 1e-6)
        d = np.zeros((n, 6))
        d[:, c] = hstep
        fd[:, :, c] = (stress(e + d)[0] - stress(e - d)[0]) / (2 * hstep[:, None])
    err = np.linalg.norm(fd - T, axis=(1, 2)) / np.linalg.norm(T, axis=(1, 2))
    assert np.quantile(err, 0.9) < 1e-5, np.sort(err)[-10:]


# --- 4. one point whose parameters make its Newton iteration fail -------------------------------------------------
def test_nonconvergence_of_one_point_is_reported():
    from test_oracle_c import NONCONVERGING

    n = 200
    p = {k: np.full(n, v) for k, v in LAWS["VonMises3D"][1].items()}
    for k, v in NONCONVERGING.items():
        p[k][77] = v
    law = fc.VonMises3D(p)
    g = np.zeros(9 * n)
    g[77 * 9 + 1] = 1.0
    s, t = torch.zeros(6 * n, dtype=torch.float64, device=DEV), torch.zeros(36 * n, dtype=torch.float64, device=DEV)
    h = hist_zeros(law, n, s)
    with pytest.raises(RuntimeError, match="did not converge"):
        law.evaluate(0.0, 1.0, torch.from_numpy(g).to(DEV), s, t, h, check=True)
    assert law.last_stats.n_nonconverged == 1
    st = ResidentState(law, n)
    st.evaluate(0.0, 1.0, torch.from_numpy(g).to(DEV))
    with pytest.raises(RuntimeError, match="did not converge"):
        st.update()
    with pytest.raises(RuntimeError, match="did not converge"):
        law.evaluate(0.0, 1.0, g, np.zeros(6 * n), np.zeros(36 * n), {k: np.zeros(d * n) for k, d in law.history_dim.items()})


# --- 5. every form without field support refuses; nothing is written -----------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    n = 256
    p = dict(LAWS["VonMises3D"][1], p_y0=np.linspace(200.0, 300.0, n))
    law = fc.VonMises3D(p)
    g = torch.from_numpy(grads(n, 1, steps=1)[0]).to(DEV)
    s = torch.full((6 * n,), 7.0, dtype=torch.float64, device=DEV)
    t = torch.full((36 * n,), 7.0, dtype=torch.float64, device=DEV)
    h = {"eps_n": torch.zeros(6 * n, dtype=torch.float64, device=DEV), "alpha": torch.zeros(n, dtype=torch.float64, device=DEV)}
    rows = torch.arange(n, dtype=torch.int32, device=DEV)
    with pytest.raises(NotImplementedError):
        law.evaluate_indexed(0.0, 1.0, g, s, s, t, rows, h, h)
    with pytest.raises(NotImplementedError):
        with _capi.batched_launches():
            law.evaluate_from(0.0, 1.0, g, s, s, t, h, h)
    with pytest.raises(NotImplementedError):
        ResidentProblemState(law, n)
    with pytest.raises(NotImplementedError):
        law.use_devices([0])
    with pytest.raises(NotImplementedError):
        MultiDeviceResidentState(law, n, devices=[0])
    for w in (fc.UniaxialStrainFrom3D, fc.PlaneStressFrom3D):
        with pytest.raises(NotImplementedError):
            w(law)
    # point count of the call differs from the fields'
    with pytest.raises(AssertionError):
        law.evaluate(0.0, 1.0, g[: 9 * (n - 64)], s[: 6 * (n - 64)], t[: 36 * (n - 64)],
                     {"eps_n": h["eps_n"][: 6 * (n - 64)], "alpha": h["alpha"][: n - 64]})
    with pytest.raises(AssertionError):
        ResidentState(law, n + 1)
    torch.cuda.synchronize()
    assert bool((s == 7.0).all()) and bool((t == 7.0).all()) and bool((h["alpha"] == 0.0).all())


def test_c_abi_refusals():
    """fcamd_evaluate_batch with a field entry, the fused wrapper form and a misaligned field: refused, nothing launched"""
    n = 128
    law = fc.VonMises3D(dict(LAWS["VonMises3D"][1], p_y0=np.linspace(200.0, 300.0, n)))
    m = law._handle(0)
    lib = m._lib
    z = lambda k: torch.zeros(k, dtype=torch.float64, device=DEV)  # noqa: E731
    g, s, t, eps, alpha = z(9 * n), torch.full((6 * n,), 7.0, dtype=torch.float64, device=DEV), z(36 * n), z(6 * n), z(n)
    fields = law._field_ptrs(0, n)
    y0 = law._field_dev[0][2]
    hist = (C.c_void_p * 2)(eps.data_ptr(), alpha.data_ptr())
    farr = (C.c_void_p * 5)(*[C.c_void_p(f) for f in fields])
    x = _capi.EvalArgs(g.data_ptr(), s.data_ptr(), s.data_ptr(), t.data_ptr(), hist, hist, 2)
    _capi.set_param_fields(x, farr)
    models = (C.c_void_p * 1)(m.handle)
    ns = (C.c_int64 * 1)(n)
    assert lib.fcamd_evaluate_batch(1, models, ns, C.byref(x), 0.0, 1.0) == _capi.ERR_UNSUPPORTED
    bad = (C.c_void_p * 5)(0, 0, y0.data_ptr() + 8, 0, 0)
    x.stress_3d = C.addressof(bad)
    assert lib.fcamd_evaluate_device_ex(m.handle, 0.0, 1.0, n, C.byref(x)) == _capi.ERR_ALIGN
    x.stress_3d = C.addressof(farr)
    x.wrapper_constraint = 1  # FCAMD_UNIAXIAL_STRAIN
    assert lib.fcamd_evaluate_device_ex(m.handle, 0.0, 1.0, n, C.byref(x)) == _capi.ERR_UNSUPPORTED
    # another law: fields are refused by the C entry as well
    sls = fc.SpringMaxwellModel({"E0": 1.0, "E1": 1.0, "tau": 1.0, "nu": 0.3}, S.FULL)._handle(0)
    y = (C.c_void_p * 4)(y0.data_ptr(), 0, 0, 0)
    x2 = _capi.EvalArgs(g.data_ptr(), s.data_ptr(), s.data_ptr(), t.data_ptr(), hist, hist, 2)
    _capi.set_param_fields(x2, y)
    vis = z(6 * n)
    h2 = (C.c_void_p * 2)(vis.data_ptr(), eps.data_ptr())
    x2.history_prev = x2.history = h2
    assert lib.fcamd_evaluate_device_ex(sls.handle, 0.0, 1.0, n, C.byref(x2)) == _capi.ERR_UNSUPPORTED
    # and a zero-filled member is the plain call
    x3 = _capi.EvalArgs(g.data_ptr(), s.data_ptr(), s.data_ptr(), t.data_ptr(), hist, hist, 2)
    assert lib.fcamd_evaluate_device_ex(m.handle, 0.0, 1.0, n, C.byref(x3)) == _capi.OK
    torch.cuda.synchronize()
