"""The gradient producer on the GPU (fenics_constitutive_amd.DisplacementGradient, csrc/jit/displacement_gradient.hip) and the
host path that takes its output (FCAMD_EVAL_GRAD_ON_DEVICE: ResidentState.evaluate_into / ResidentProblemState.evaluate_law_into
with a device tensor, integration.use_resident_state(..., gradient_operators=...)).

The kernel is compared ON THE BITS with the ordered NumPy oracle of gradient_util.py; the host path with a device gradient is
compared on the bits with the same call on an ndarray of the same values."""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_gradient import DeviceGradientState, IncrementMesh  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import _capi, gradient, jit  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402
from fenics_constitutive_amd.integration import use_resident_problem_state, use_resident_state  # noqa: E402
from fenics_constitutive_amd.problem import ResidentProblemState  # noqa: E402
from fenics_constitutive_amd.resident import ResidentState  # noqa: E402
from fe_gpu_util import CANARY, MARGIN, bits, guarded, assert_margins_intact  # noqa: E402
from fe_gpu_util import one_cu  # noqa: E402, F401 (the fixture: pytest finds it in this namespace)
from gradient_util import LAYOUTS, SHAPES, cell_counts, cube_operator_tables, oracle, random_tables, rounding_bound  # noqa: E402
from test_gpu_integration import Fn, Problem  # noqa: E402
from test_gpu_parity import make_law, random_case  # noqa: E402

FULL = fc.StressStrainConstraint.FULL


def run_and_compare(shape, n_cells, layout, affine, integer, seed):
    du, dofmap, ref, jinv, n_nodes = random_tables(shape, n_cells, seed, integer, affine)
    assert dofmap.min() == 0 and dofmap.max() == n_nodes - 1
    op = fc.DisplacementGradient(dofmap, ref, jinv, n_nodes, layout=layout)
    nout = op.gdim**2 * op.n_points
    buf, out = guarded(nout)
    got = op(du, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    want = oracle(du, dofmap, ref, jinv, layout)
    have = to_host(out)
    diff = bits(have) != bits(want)
    assert not diff.any(), f"{shape} cells={n_cells} {layout} affine={affine} integer={integer}: {int(diff.sum())} of {nout} entries differ, first at {int(np.argmax(diff))}"
    assert_margins_intact(buf, nout)
    return op


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. every shape, both layouts, per-cell and per-point inverse Jacobians, the sizes around a tile
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["per_cell", "per_point"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bits_of_the_ordered_oracle(shape, layout, affine):
    q = SHAPES[shape][2]
    for n_cells in cell_counts(q):
        for integer in (True, False):
            run_and_compare(shape, n_cells, layout, affine, integer, seed=n_cells + 7 * integer)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the grid-stride loop
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,affine", [("hex8", False), ("q5", True), ("q5", False), ("tri_p2", True), ("tet_p1", True)])
def test_grid_stride_loop(shape, affine, one_cu):
    q = SHAPES[shape][2]
    per_trip = gradient.BLOCKS_PER_CU * 4 * 64  # points all waves of the capped grid cover in one trip
    # two whole trips, five more full tiles and a ragged one: every wave makes two trips, six make a third, the ragged tile is
    # the sixth wave's third
    n_cells = -(-(2 * per_trip + 5 * 64 + 23) // q)
    assert (n_cells * q) % 64 != 0 and (n_cells * q) // 64 == 2 * gradient.BLOCKS_PER_CU * 4 + 5
    for integer in (True, False):
        run_and_compare(shape, n_cells, "nabla_grad", affine, integer, seed=3)
    assert one_cu and all(nb == gradient.BLOCKS_PER_CU for _, nb in one_cu), one_cu  # the launches really were capped


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. call forms
# ---------------------------------------------------------------------------------------------------------------------------------
def test_call_forms():
    du, dofmap, ref, jinv, n_nodes = random_tables("hex8", 21, 11, False, False)
    op = fc.DisplacementGradient(dofmap, ref, jinv, n_nodes)
    nout = 9 * op.n_points
    want = oracle(du, dofmap, ref, jinv)
    a = op(du)
    assert a.dtype == torch.float64 and a.is_cuda and a.numel() == nout
    b = op(to_device(du, "cuda"))
    assert a.data_ptr() != b.data_ptr()
    assert np.array_equal(bits(to_host(a)), bits(want)) and np.array_equal(bits(to_host(b)), bits(want))
    # a strided ndarray is gathered on the host first
    wide = np.zeros((du.size, 2))
    wide[:, 0] = du
    assert np.array_equal(bits(to_host(op(wide[:, 0]))), bits(want))
    buf, out = guarded(nout)
    assert op(du, out=out) is out
    assert np.array_equal(bits(to_host(out)), bits(want))
    assert_margins_intact(buf, nout)
    # refusals come before the launch: the canaries (and the output region) stay as they are
    buf, out = guarded(nout)
    launches = []
    real = jit.launch
    jit.launch = lambda *args: launches.append(args) or real(*args)
    try:
        with pytest.raises(ValueError, match="aligned"):
            op(du, out=buf[MARGIN + 1: MARGIN + 1 + nout])
        with pytest.raises(ValueError):
            op(du, out=buf[MARGIN: MARGIN + nout - 9])
        with pytest.raises(ValueError):
            op(du, out=buf[MARGIN: MARGIN + 2 * nout: 2])
        with pytest.raises(ValueError):
            op(du, out=torch.empty(nout, dtype=torch.float64))  # on the host
        with pytest.raises(ValueError):
            op(du, out=out.float())
        with pytest.raises(ValueError):
            op(du[:-1])
        with pytest.raises(TypeError):
            op(du.astype(np.float32))
        with pytest.raises(TypeError):
            op(to_device(du, "cuda").float())
    finally:
        jit.launch = real
    torch.cuda.synchronize()
    assert not launches
    assert (bits(to_host(buf)) == CANARY).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. ResidentState.evaluate_into(tensor) against evaluate_into(ndarray of the same values)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def ctx():
    c = _capi.get_context(_capi.default_device())
    saved = {k: c.get_option(k) for k in ("host_tangent_min_points", "host_chunk", "bounce_max")}
    yield c
    for k, v in saved.items():
        c.set_option(k, v)
    c.set_option("host_tangent_threads", -1)


KINDS = ["linear_elasticity", "spring_maxwell", "von_mises_3d", "comfe_mises_plasticity"]
CONST_TANGENT = ("linear_elasticity", "spring_maxwell")
MODE_NAMES = {"in": _capi.HOST_ZERO_COPY_IN, "out": _capi.HOST_ZERO_COPY_OUT, "temp": _capi.HOST_TEMP_LOCK, "bounce": _capi.HOST_BOUNCE,
              "cpu": _capi.HOST_TANGENT_CPU}


def three_calls(ctx, kind, n, device_gradient, arrays, pin=False, split_lock=False, stage_gradient=False):
    """a state of its own; evaluate, evaluate, update, evaluate into the same caller arrays (the third call: sparse tangent where
    the law has one); per call the caller's arrays, the trial state, the stats and last_host_mode"""
    p, g1, s0, h0 = random_case(kind, n, seed=n % 89 + 3)
    g2 = random_case(kind, n, seed=n % 89 + 4)[1]
    law = make_law(kind, p)
    st = ResidentState(law, n, stress0=s0, history0=h0, placement="torch")
    so, to = arrays(6 * n), arrays(36 * n)
    so[:], to[:] = np.nan, np.nan
    if pin:
        assert so.ctypes.data % 16 == 0 and to.ctypes.data % 16 == 0  # the one-launch pass needs the outputs on the 16-byte grid
        law.pin_host_arrays(so, to)
    if split_lock:  # the front half of the stress array registered: the whole array can no longer be locked for a call
        ctx.register_host_buffer(so[: 6 * (n // 2)])
    out = []
    try:
        for step, g in enumerate((g1, g2, g1)):
            if pin and not device_gradient:
                g = g.copy()
                law.pin_host_arrays(g)
            if stage_gradient and not device_gradient:  # off the 16-byte grid: uploaded chunk by chunk, never read in place
                g = offset_by_8(g.size)
                g[:] = (g1, g2, g1)[step]
            stats = st.evaluate_into(float(step), 2.0, to_device(g, st.device) if device_gradient else g, so, to)
            mode = ctx.last_host_mode()
            hist = None if st.history is None else {k: to_host(v) for k, v in st.history.items()}
            out.append((so.copy(), to.copy(), to_host(st.stress), hist, (stats.n_nonconverged, stats.n_plastic, stats.n_newton_iters, stats.n_domain), mode))
            if step == 1:
                st.update()
    finally:
        if pin:
            law.unpin_arrays()
        if split_lock:
            ctx.unregister_host_buffer(so[: 6 * (n // 2)])
    return out


def assert_same_calls(nd, dev, what):
    for k, (a, b) in enumerate(zip(nd, dev)):
        for name, x, y in (("stress", a[0], b[0]), ("tangent", a[1], b[1]), ("trial stress", a[2], b[2])):
            assert np.array_equal(bits(x), bits(y)), f"{what} call {k}: {name} differs in {int((bits(x) != bits(y)).sum())} entries"
        assert not np.isnan(b[0]).any() and not np.isnan(b[1]).any(), f"{what} call {k}: unwritten entries"
        for name in (a[3] or {}):
            assert np.array_equal(bits(a[3][name]), bits(b[3][name])), f"{what} call {k}: history[{name}]"
        assert a[4] == b[4], f"{what} call {k}: stats {a[4]} / {b[4]}"
        assert not (b[5] & MODE_NAMES["in"]), f"{what} call {k}: FCAMD_HOST_ZERO_COPY_IN set with a device gradient (mode {b[5]})"


@pytest.mark.parametrize("n", [1, 63, 65, 1000])
@pytest.mark.parametrize("kind", KINDS)
def test_evaluate_into_small_pageable_arrays(ctx, kind, n):
    """the scratch path wherever the host OUTPUTS of the call fit "bounce_max" (the gradient no longer counts), else page locks
    for the call"""
    nd = three_calls(ctx, kind, n, False, np.empty)
    dev = three_calls(ctx, kind, n, True, np.empty)
    assert_same_calls(nd, dev, f"{kind}/{n}")
    bounce_max = ctx.get_option("bounce_max")
    for k, call in enumerate(dev):
        tangent_sent = not (kind in CONST_TANGENT and k > 0)  # a constant tangent is downloaded once per array and del_t
        expected = n * 8 * (6 + 36 * tangent_sent) <= bounce_max
        assert bool(call[5] & MODE_NAMES["bounce"]) == expected, (k, call[5], expected)
        assert expected or (call[5] & MODE_NAMES["temp"]), (k, call[5])
    if kind in ("von_mises_3d", "comfe_mises_plasticity") and n >= 63:
        assert 0 < dev[0][4][1] < n, "the case must mix elastic and plastic points"


@pytest.mark.parametrize("threads", [3, 0], ids=["pool", "kernel_tangent"])
@pytest.mark.parametrize("kind", KINDS)
def test_evaluate_into_pinned_arrays_one_launch(ctx, kind, threads):
    n = 70_003
    ctx.set_option("host_tangent_threads", threads)
    nd = three_calls(ctx, kind, n, False, np.empty, pin=True)
    dev = three_calls(ctx, kind, n, True, np.empty, pin=True)
    assert_same_calls(nd, dev, f"{kind}/pinned/{threads}")
    for k, call in enumerate(dev):
        mode = call[5]
        assert not (mode & (MODE_NAMES["bounce"] | MODE_NAMES["temp"])), (k, mode)
        if not (kind in CONST_TANGENT and k > 0):  # (a constant tangent is sent once; the stress store alone sets no bit)
            assert mode & MODE_NAMES["out"], (k, mode)  # the kernel's own stores into the caller's arrays: the one-launch pass
    # the first call is a full-tangent one: rebuilt by the pool where there is one
    assert bool(dev[0][5] & MODE_NAMES["cpu"]) == (threads > 0), dev[0][5]
    assert bool(nd[0][5] & MODE_NAMES["cpu"]) == (threads > 0) and (nd[0][5] & MODE_NAMES["in"])


@pytest.mark.parametrize("kind", ["linear_elasticity", "von_mises_3d"])
def test_evaluate_into_several_scratch_chunks(ctx, kind):
    """host arrays that cannot be page-locked for the call (a part of the stress array belongs to a registered range) go through
    the scratch in chunks of 64 MiB: 250 003 points with a tangent are two, the second reads the device gradient at its offset"""
    n = 250_003
    assert n * 8 * (6 + 36) > 64 << 20
    nd = three_calls(ctx, kind, n, False, np.empty, split_lock=True)
    dev = three_calls(ctx, kind, n, True, np.empty, split_lock=True)
    assert_same_calls(nd, dev, f"{kind}/scratch chunks")
    for k, call in enumerate(dev):
        assert call[5] == MODE_NAMES["bounce"], (k, call[5])


def offset_by_8(size):
    a = np.empty(size + 1)[1:]
    assert a.ctypes.data % 16 == 8
    return a


@pytest.mark.parametrize("kind", KINDS)
def test_evaluate_into_chunk_ring(ctx, kind):
    """host outputs off the 16-byte grid: chunks of 8192 points, the tangent staged, the gradient read in place slice by slice"""
    n = 70_003
    ctx.set_option("host_chunk", 8192)
    # (the ndarray reference's gradient is staged through the chunk slots: its launches do not share the in-place slicing of the
    # device gradient, so a wrong offset there cannot cancel in the comparison)
    nd = three_calls(ctx, kind, n, False, offset_by_8, stage_gradient=True)
    dev = three_calls(ctx, kind, n, True, offset_by_8)
    assert_same_calls(nd, dev, f"{kind}/ring")
    assert all(not (call[5] & MODE_NAMES["in"]) for call in nd), [call[5] for call in nd]
    for k, call in enumerate(dev):
        mode = call[5]
        assert (mode & MODE_NAMES["temp"]) and not (mode & (MODE_NAMES["bounce"] | MODE_NAMES["out"] | MODE_NAMES["cpu"])), (k, mode)


def test_raw_device_entry_refuses_the_flag():
    n = 100
    law = make_law("linear_elasticity", random_case("linear_elasticity", n, seed=1)[0])
    m = law._handle(_capi.default_device())
    g = torch.zeros(9 * n, dtype=torch.float64, device="cuda")
    s = to_device(np.full(6 * n, CANARY, dtype=np.uint64).view(np.float64), "cuda")
    t = to_device(np.full(36 * n, CANARY, dtype=np.uint64).view(np.float64), "cuda")
    with pytest.raises(NotImplementedError):
        m.evaluate_device_ex(0.0, 1.0, n, g.data_ptr(), s.data_ptr(), s.data_ptr(), t.data_ptr(), [], [], flags=_capi.EVAL_GRAD_ON_DEVICE)
    torch.cuda.synchronize()
    assert (bits(to_host(s)) == CANARY).all() and (bits(to_host(t)) == CANARY).all()
    # a misaligned device gradient never reaches the library's launches either
    st = ResidentState(law, n, placement="torch")
    with pytest.raises(ValueError, match="aligned"):
        st.evaluate_into(0.0, 1.0, torch.zeros(9 * n + 1, dtype=torch.float64, device="cuda")[1:], np.zeros(6 * n), np.zeros(36 * n))
    with pytest.raises(ValueError):  # the C entry's own check
        m.evaluate_resident(0.0, 1.0, n, g.data_ptr() + 8, st.stress_committed.data_ptr(), st.stress.data_ptr(), [], [], None, None, None,
                            _capi.EVAL_GRAD_ON_DEVICE)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the problem state, and the operator's output in the other entries
# ---------------------------------------------------------------------------------------------------------------------------------
def test_problem_state_takes_a_tensor_gradient():
    n_cells, q = 300, 4
    n = n_cells * q
    owner = np.arange(n_cells) % 2  # interleaved submeshes
    rows = [(np.flatnonzero(owner == k)[:, None] * q + np.arange(q)[None, :]).reshape(-1) for k in range(2)]
    vm_p, g_vm, _, _ = random_case("von_mises_3d", rows[0].size, seed=5)
    mx_p, g_mx, _, _ = random_case("spring_maxwell", rows[1].size, seed=6)
    s0 = np.random.default_rng(2).normal(scale=30.0, size=6 * n)
    results = []
    for device_gradient in (False, True):
        laws = [make_law("von_mises_3d", vm_p), make_law("spring_maxwell", mx_p)]
        state = ResidentProblemState([(laws[0], rows[0]), (laws[1], rows[1])], n, del_t=0.5)
        state.set_state(s0)
        so, to = np.full(6 * n, np.nan), np.full(36 * n, np.nan)
        laws[0].pin_host_arrays(so, to)
        try:
            for it in range(2):
                for k, g in enumerate((g_vm, g_mx)):
                    g = (1.0 + it) * g
                    state.evaluate_law_into(k, to_device(g, "cuda") if device_gradient else g, so, to, sync=(k == 1))
                results.append((so.copy(), to.copy()))
        finally:
            laws[0].unpin_arrays()
    for (s_a, t_a), (s_b, t_b) in zip(results[:2], results[2:]):
        assert not np.isnan(s_b).any() and not np.isnan(t_b).any()
        assert np.array_equal(bits(s_a), bits(s_b)) and np.array_equal(bits(t_a), bits(t_b))


def test_operator_output_feeds_the_device_entries():
    mesh = FE.Cube(3, 2, 2)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    op = fc.DisplacementGradient(dofmap, ref, jinv, mesh.n_nodes)
    du = np.random.default_rng(0).normal(scale=1e-4, size=mesh.n_dofs)
    n = mesh.n_points
    law = fc.LinearElasticityModel({"E": 42.0, "nu": 0.3}, FULL)
    st = ResidentState(law, n, placement="torch")
    st.evaluate(0.0, 1.0, op(du))
    s_ref, t_ref = np.zeros(6 * n), np.zeros(36 * n)
    law.evaluate(0.0, 1.0, to_host(op(du)), s_ref, t_ref, None)
    assert np.array_equal(bits(to_host(st.stress)), bits(s_ref))
    # a user-defined law reads the same array
    from fenics_constitutive_amd import userlaw_sources

    user = userlaw_sources.linear_elasticity({"E": 42.0, "nu": 0.3})
    s = torch.zeros(6 * n, dtype=torch.float64, device="cuda")
    t = torch.zeros(36 * n, dtype=torch.float64, device="cuda")
    user.evaluate(0.0, 1.0, op(du), s, t, None)
    torch.cuda.synchronize()
    assert np.array_equal(bits(to_host(s)), bits(s_ref)) and np.array_equal(bits(to_host(t)), bits(t_ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the FE loop
# ---------------------------------------------------------------------------------------------------------------------------------
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}


def test_cube_under_tension_with_the_operator():
    mesh = FE.Cube(5, 4, 5)
    n = mesh.n_points
    ref_state = FE.ResidentProtocolState(ResidentState(fc.VonMises3D(VM_P), n), n)
    r_ref, n_ref, u_ref = FE.tension_test(mesh, ref_state, steps=6)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    op = fc.DisplacementGradient(dofmap, ref, jinv, mesh.n_nodes, layout="grad")
    state = DeviceGradientState(ResidentState(fc.VonMises3D(VM_P), n), n, op)
    r, norms, u = FE.tension_test(IncrementMesh(mesh), state, steps=6)
    assert [len(h) for h in norms] == [len(h) for h in n_ref]
    assert max(len(h) for h in norms) >= 4  # the cube yields
    assert np.max(np.abs(r - r_ref)) <= 1e-8 * np.max(np.abs(r_ref)), (r, r_ref)
    assert np.max(np.abs(u - u_ref)) <= 1e-7 * np.max(np.abs(u_ref))
    got = to_host(op(u))
    assert (np.abs(got - mesh.gradient(u)) <= rounding_bound(u, dofmap, ref, jinv, "grad")).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. integration
# ---------------------------------------------------------------------------------------------------------------------------------
class CubeIncrDisp:
    """IncrementalDisplacement stand-in (solver/_incrementalunknowns.py): current / previous nodal arrays over a Cube"""

    def __init__(self, mesh):
        self.mesh, self.current, self.previous, self.calls = mesh, Fn(mesh.n_dofs), Fn(mesh.n_dofs), 0

    def evaluate_local_incremental_gradient(self, cells, fn):
        self.calls += 1
        g = self.mesh.gradient(self.current.x.array - self.previous.x.array).reshape(self.mesh.n_cells, 8 * 9)
        fn.x.array[:] = g[cells].reshape(-1)


def cube_problem(mesh, seed):
    rng = np.random.default_rng(seed)
    owner = np.arange(mesh.n_cells) % 2
    le = fc.LinearElasticityModel({"E": 42.0, "nu": 0.3}, FULL)
    mx = fc.SpringMaxwellModel({"E0": 42.0, "E1": 10.0, "tau": 10.0, "nu": 0.2}, FULL)
    laws = []
    for k, law in enumerate((le, mx)):
        cells = np.flatnonzero(owner == k).astype(np.int32)
        laws.append((law, cells, (cells[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)))
    p = Problem(laws, mesh.n_points)
    p.incr_disp = CubeIncrDisp(mesh)
    p.stress.previous.x.array[:] = rng.normal(scale=5.0, size=6 * mesh.n_points)
    return p


@pytest.mark.parametrize("patch", ["state", "problem_state"])
def test_integration_with_gradient_operators(patch):
    mesh = FE.Cube(4, 3, 5)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    a, b = cube_problem(mesh, 4), cube_problem(mesh, 4)
    ops = [fc.DisplacementGradient(dofmap[los.cells], ref, jinv[los.cells], mesh.n_nodes, layout="grad") for los in b._law_on_submeshs]
    if patch == "state":
        use_resident_state(a)
        use_resident_state(b, gradient_operators=ops)
    else:
        use_resident_problem_state(a)
        use_resident_problem_state(b, gradient_operators=ops)
    rng = np.random.default_rng(9)
    try:
        for inc in range(2):
            for it in range(2):
                du = rng.normal(scale=1e-3, size=mesh.n_dofs)
                for p in (a, b):
                    p.incr_disp.current.x.array[:] = p.incr_disp.previous.x.array + du
                    p.form()
                for name, x, y, tol in (("stress", a.stress.current.x.array, b.stress.current.x.array, 1e-10),
                                        ("tangent", a.tangent.x.array, b.tangent.x.array, 1e-10)):
                    assert np.abs(x).max() > 0
                    assert np.max(np.abs(x - y)) <= tol * np.max(np.abs(x)), (name, inc, it)
            for p in (a, b):
                p.update()
                p.incr_disp.previous.x.array[:] = p.incr_disp.current.x.array
    finally:
        for p in (a, b):
            for los in p._law_on_submeshs:
                los.law.unpin_arrays()
    assert a.incr_disp.calls == 8 and b.incr_disp.calls == 0  # with operators the host gradient is never formed
    assert not b._law_on_submeshs[0].displacement_gradient_fn.x.array.any()
