"""The force operator on the GPU (fenics_constitutive_amd.InternalForce, csrc/jit/internal_force.hip): nodal internal forces from
the stress of the quadrature points and the tangent action from tangent and gradient, compared ON THE BITS with the ordered NumPy
oracle of force_util.py; behind a resident state; and in the matrix-free Newton loop of examples/cube_tension_matrix_free.py."""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_matrix_free import DeviceLoop, cube_operators, tension_test_matrix_free  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import force as force_module  # noqa: E402
from fenics_constitutive_amd import gradient, jit  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402
from fenics_constitutive_amd.resident import ResidentState  # noqa: E402
from fe_gpu_util import CANARY, MARGIN, bits, guarded, assert_margins_intact  # noqa: E402
from fe_gpu_util import one_cu  # noqa: E402, F401 (the fixture: pytest finds it in this namespace)
from force_util import MANDEL_DIM, OracleLoop, cell_counts, force_oracle, random_inputs, tangent_action_oracle  # noqa: E402
from gradient_util import SHAPES, cube_operator_tables, oracle  # noqa: E402

#: gradient_util's shapes, one whose cells per tile the odd rule lowers (64 // 3 = 21 cells would be 567 doubles of jinv: 20), and
#: two with ONE cell per tile and Q and D odd: no tile base stays on the 16-byte grid and the kernel takes its guarded 8-byte loads
ALL_SHAPES = dict(SHAPES, q3=(3, 4, 3, True), odd33_1d=(1, 2, 33, False), odd33_3d=(3, 4, 33, False))
SOURCES = ("stress", "tangent")
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}


# stays here: fe_gpu_util's flattens both sides first, this one compares them in their shapes and so refuses (4,) against (2, 2)
def assert_same_bits(have, want, what):
    diff = bits(have) != bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} entries differ, first at {int(np.argmax(diff))}"


def build(shape, t, layout="nabla_grad"):
    op = fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"], layout=layout)
    return op, fc.InternalForce(op, t["weights"])


def run(f, t, source, layout, out=None, accumulate=False):
    if source == "stress":
        return f(to_device(t["stress"], "cuda"), out=out, accumulate=accumulate)
    return f.tangent_action(to_device(t["tangent"], "cuda"), to_device(t["grad_v"], "cuda"), out=out, accumulate=accumulate)


def expected(t, source, layout, start=None):
    tables = (t["dofmap"], t["ref"], t["jinv"], t["weights"], t["n_nodes"])
    if source == "stress":
        return force_oracle(t["stress"], *tables, start=start)
    return tangent_action_oracle(t["tangent"], t["grad_v"], *tables, layout, start=start)


def run_and_compare(shape, n_cells, source, layout, affine, integer, seed):
    t = random_inputs(ALL_SHAPES[shape], n_cells, seed, integer, affine)
    assert t["dofmap"].min() == 0 and t["dofmap"].max() == t["n_nodes"] - 1 and not (t["dofmap"] == t["lonely"]).any()
    op, f = build(shape, t, layout)
    d_ = op.gdim
    nout = d_ * t["n_nodes"]
    buf, out = guarded(nout)  # accumulate=False overwrites the canaries of the view
    got = run(f, t, source, layout, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    have = to_host(out)
    what = f"{shape} cells={n_cells} {source} {layout} affine={affine} integer={integer}"
    assert_same_bits(have, expected(t, source, layout), what)
    assert (bits(have.reshape(-1, d_)[t["lonely"]]) == 0).all(), f"{what}: the node no cell touches is not +0.0"
    assert_margins_intact(buf, nout)
    # and on top of an earlier vector: the untouched node keeps its old value
    start = np.random.default_rng(seed).integers(-5, 6, size=nout).astype(np.float64)
    buf, out = guarded(nout, fill=start)
    run(f, t, source, layout, out=out, accumulate=True)
    torch.cuda.synchronize()
    have = to_host(out)
    assert_same_bits(have, expected(t, source, layout, start=start), what + " accumulate")
    assert_same_bits(have.reshape(-1, d_)[t["lonely"]], start.reshape(-1, d_)[t["lonely"]], what + " accumulate, untouched node")
    assert_margins_intact(buf, nout)
    return f


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. every shape, both sources, per-cell and per-point inverse Jacobians, the sizes around a tile
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["per_cell", "per_point"])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("shape", list(ALL_SHAPES))
def test_bits_of_the_ordered_oracle(shape, source, affine):
    d_, _, q = ALL_SHAPES[shape][:3]
    w = force_module.cells_per_tile(d_, q)
    assert (shape != "q3" or w == 20) and ((w * q * d_ * d_) % 2 == 0) == (not shape.startswith("odd33")) and (w == 1 or not shape.startswith("odd33"))
    for k, n_cells in enumerate(cell_counts(w, q)):
        for integer in (True, False):
            layout = gradient.LAYOUTS[(k + integer) % 2]  # both layouts of the gradient at every shape (the stress form reads none)
            f = run_and_compare(shape, n_cells, source, layout, affine, integer, seed=n_cells + 7 * integer)
    assert f.cells_per_tile == w


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the grid-stride loops of both kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("shape,affine", [("hex8", False), ("q5", True), ("q3", False), ("tri_p2", True)])
def test_grid_stride_loops(shape, affine, source, one_cu):
    d_, _, q = ALL_SHAPES[shape][:3]
    w = force_module.cells_per_tile(d_, q)
    waves = gradient.BLOCKS_PER_CU * 4  # tiles all waves of the capped grid cover in one trip
    # two whole trips, five more whole tiles and a short one: every wave makes two trips, six make a third, the short tile is the
    # sixth wave's third
    n_cells = (2 * waves + 5) * w + w // 2
    assert w // 2 >= 1 and n_cells // w == 2 * waves + 5 and n_cells % w
    for integer in (True, False):
        f = run_and_compare(shape, n_cells, source, "nabla_grad", affine, integer, seed=3)
    assert d_ * f.n_nodes > gradient.BLOCKS_PER_CU * 256  # the node kernel: more dofs than one trip of the capped grid covers
    kernels = {k for k, _ in one_cu}
    assert kernels == {force_module.ELEMENT_KERNEL, force_module.NODE_KERNEL}
    assert all(b == gradient.BLOCKS_PER_CU for _, b in one_cu), one_cu  # the launches really were capped


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. two operators on complementary cells of one mesh, the second accumulating onto the first
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("shape,affine", [("hex8", False), ("tet_p2", True)])
def test_accumulate_over_submeshes(shape, affine, source):
    t = random_inputs(shape, 75, 21, False, affine)
    d_, _, q = SHAPES[shape][:3]
    s_ = MANDEL_DIM[d_]
    owner = np.arange(75) % 3 == 1  # interleaved submeshes of 25 and 50 cells
    parts = []
    for cells in (np.flatnonzero(owner), np.flatnonzero(~owner)):
        sub = dict(t, dofmap=np.ascontiguousarray(t["dofmap"][cells]), jinv=np.ascontiguousarray(t["jinv"][cells]),
                   weights=np.ascontiguousarray(t["weights"][cells]))
        for name, width in (("stress", s_), ("tangent", s_ * s_), ("grad_v", d_ * d_)):
            sub[name] = np.ascontiguousarray(t[name].reshape(75, q * width)[cells]).reshape(-1)
        parts.append(sub)
    nout = d_ * t["n_nodes"]
    buf, out = guarded(nout)
    want = None
    for k, sub in enumerate(parts):
        _, f = build(shape, sub)
        run(f, sub, source, "nabla_grad", out=out, accumulate=k > 0)
        want = expected(sub, source, "nabla_grad", start=want)
    torch.cuda.synchronize()
    assert_same_bits(to_host(out), want, f"{shape} {source}: two submeshes")
    assert_margins_intact(buf, nout)
    # the order of the two is part of the result: the other order is another sum (and the whole mesh at once a third)
    other = expected(parts[0], source, "nabla_grad", start=expected(parts[1], source, "nabla_grad"))
    assert not np.array_equal(other, want) and np.allclose(other, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the transpose of the producer, exactly
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,affine", [("hex8", False), ("tet_p2", True), ("tri_p2", True), ("interval", True)])
def test_adjoint_of_the_gradient_operator_exactly(shape, affine):
    """<force(s), v> = sum_p w_p T_p : grad v_p with no rounding at all: small integers in the tables, the stress and v, inverse
    Jacobians and weights that are small multiples of 1/4, zero shear components (so H never enters).  That these inputs are exact
    is checked first, on the CPU: the float oracle equals the same sums in 64-bit integers."""
    t = random_inputs(shape, 37, 5, True, affine)
    d_, a_, q = SHAPES[shape][:3]
    s_ = MANDEL_DIM[d_]
    stress = t["stress"].reshape(-1, s_).copy()
    stress[:, d_ if d_ > 1 else 1:] = 0.0  # D = 2: zz as well, which does no work in the plane
    t["stress"] = stress.reshape(-1)
    v = np.random.default_rng(9).integers(-8, 9, size=d_ * t["n_nodes"]).astype(np.float64)
    dofmap, ref, jinv, weights = t["dofmap"], t["ref"], t["jinv"], t["weights"]
    # CPU: the oracle in integers (jinv and weights times 4)
    j4 = np.rint(4 * (jinv if jinv.ndim == 4 else np.repeat(jinv[:, None], q, axis=1))).astype(np.int64)
    w4 = np.rint(4 * weights).astype(np.int64)
    assert np.array_equal(j4 / 4.0, jinv if jinv.ndim == 4 else np.repeat(jinv[:, None], q, axis=1)) and np.array_equal(w4 / 4.0, weights)
    si = stress[:, :d_].astype(np.int64).reshape(-1, q, d_)  # the diagonal of T
    g16 = np.einsum("qak,cqkx->cqax", ref.astype(np.int64), j4)  # 4 * d N_a / d x_x
    fe16 = np.einsum("cqr,cqar,cq->car", si, g16, w4)  # 16 * fe: T diagonal, t[r] = T[r][r] g[r]
    f16 = np.zeros((t["n_nodes"], d_), dtype=np.int64)
    np.add.at(f16, dofmap.reshape(-1), fe16.reshape(-1, d_))
    f_cpu = force_oracle(t["stress"], dofmap, ref, jinv, weights, t["n_nodes"])
    assert np.array_equal(f_cpu * 16.0, f16.reshape(-1).astype(np.float64)), "the chosen inputs are not exact"
    grad_cpu = oracle(v, dofmap, ref, jinv, "grad").reshape(-1, q, d_, d_)
    g4 = np.einsum("car,qak,cqkx->cqrx", v.astype(np.int64).reshape(-1, d_)[dofmap], ref.astype(np.int64), j4)
    assert np.array_equal(grad_cpu * 4.0, g4.astype(np.float64))
    rhs16 = int(np.einsum("cqr,cqrr,cq->", si, g4, w4))
    assert int(f16.reshape(-1) @ v.astype(np.int64)) == rhs16 and rhs16 != 0
    # GPU
    op, f = build(shape, t, "grad")
    have_f = to_host(f(to_device(t["stress"], "cuda")))
    have_g = to_host(op(v)).reshape(-1, q, d_, d_)
    assert_same_bits(have_f, f_cpu, f"{shape}: force")
    lhs = float(have_f @ v)
    rhs = float(np.einsum("cqr,cqrr,cq->", stress[:, :d_].reshape(-1, q, d_), have_g, weights))
    assert lhs == rhs == rhs16 / 16.0, (lhs, rhs, rhs16 / 16.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. behind a resident state
# ---------------------------------------------------------------------------------------------------------------------------------
def tilted_stretch(mesh, scale):
    u = np.zeros((mesh.n_nodes, 3))
    u[:, 2] = scale * 0.0065 * (1.0 + 0.6 * (mesh.nodes[:, 0] - 0.5)) * mesh.nodes[:, 2]
    u[:, 0] = -0.3 * scale * 0.0065 * mesh.nodes[:, 0] * mesh.nodes[:, 1]
    return u.reshape(-1)


@pytest.mark.parametrize("kind", ["linear_elasticity", "von_mises_3d"])
def test_in_the_loop_behind_a_resident_state(kind):
    mesh = FE.Cube(4, 3, 5)
    n = mesh.n_points
    op, f = cube_operators(mesh)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    tables = (dofmap, ref, jinv, f._weights, mesh.n_nodes)
    law = fc.LinearElasticityModel({"E": 42.0, "nu": 0.3}, fc.StressStrainConstraint.FULL) if kind == "linear_elasticity" else fc.VonMises3D(VM_P)
    rs = ResidentState(law, n, placement="torch")
    v = np.random.default_rng(4).normal(scale=1e-3, size=mesh.n_dofs)
    tangents = []
    for call, scale in enumerate((0.9, 1.0)):  # the second evaluate writes the sparse tangent where the law has one
        rs.evaluate(0.0, 1.0, op(tilted_stretch(mesh, scale)))
        have = to_host(f(rs.stress))
        stress = to_host(rs.stress)
        assert np.abs(stress).max() > 0
        assert_same_bits(have, force_oracle(stress, *tables), f"{kind} call {call}: force(rs.stress)")
        grad_v = op(v)
        have = to_host(f.tangent_action(rs.tangent, grad_v))
        tangent = to_host(rs.tangent)
        assert_same_bits(have, tangent_action_oracle(tangent, to_host(grad_v), *tables, "nabla_grad"), f"{kind} call {call}: tangent_action")
        assert np.abs(have).max() > 0
        tangents.append(tangent.reshape(n, 36))
    if kind == "von_mises_3d":
        stats = rs.check()
        assert 0 < stats.n_plastic < n, "the cube must yield in part"
        assert 0 < (tangents[0] != tangents[1]).any(axis=1).sum() < n  # the second call rewrote the rows of the plastic points only


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the matrix-free tension test
# ---------------------------------------------------------------------------------------------------------------------------------
def test_matrix_free_tension_test():
    """The example's loop converges in every load step under fe_mini's own criterion.  The reaction tolerance: the direct solve and
    the matrix-free loop differ on the CPU (same law -- the NumPy oracle --, the ordered oracles as operators) by ``delta`` relative
    to the largest reaction, from the conjugate gradients stopping at 1e-12 and the other summation order; the GPU run is allowed ten
    times that against the direct solve: the factor covers the device law's rounding, not another algorithm.
    Measured on the CPU: delta = 4.9e-14."""
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    n = mesh.n_points

    def cpu_state():
        return FE.CopyProtocolState(FE.OracleLaw(O.von_mises_3d, VM_P, {"eps_n": 6, "alpha": 1}), n)

    r_direct, norms_direct, _ = FE.tension_test(mesh, cpu_state(), steps=8)
    op, f = cube_operators(mesh)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    r_cpu, norms_cpu, _, _ = tension_test_matrix_free(mesh, OracleLoop(cpu_state(), dofmap, ref, jinv, f._weights, mesh.n_nodes), steps=8)
    scale = np.max(np.abs(r_direct))
    delta = np.max(np.abs(r_cpu - r_direct)) / scale
    loop = DeviceLoop(ResidentState(fc.VonMises3D(VM_P), n, placement="torch"), op, f)
    r_gpu, norms_gpu, u, solves = tension_test_matrix_free(mesh, loop, steps=8)  # (raises where a load step does not converge)
    difference = np.max(np.abs(r_gpu - r_direct)) / scale
    print(f"matrix-free tension test: delta (CPU, matrix-free against direct) {delta:.3e}, GPU against direct {difference:.3e}, "
          f"Newton iterations {[len(h) for h in norms_gpu]}, conjugate-gradient iterations {min(solves)} .. {max(solves)}")
    assert len(norms_gpu) == 8 and max(len(h) for h in norms_gpu) >= 4  # the cube yields
    for h in norms_gpu:
        assert h[-1] <= 1e-10 * max(scale, 1.0)
    assert 0 < delta < 1e-10
    assert difference <= 10 * delta, (difference, delta)
    # only nodal vectors crossed the link
    assert loop.evaluations == sum(len(h) for h in norms_gpu) and loop.actions >= sum(solves)
    assert loop.bytes_up == loop.bytes_down == 8 * mesh.n_dofs * (loop.evaluations + loop.actions)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. refusals come before any launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    t = random_inputs("hex8", 21, 11, False, False)
    op, f = build("hex8", t)
    n, nd = f.n_points, 3 * f.n_nodes
    stress, tangent, grad_v = (to_device(t[k], "cuda") for k in ("stress", "tangent", "grad_v"))
    f(stress), f.tangent_action(tangent, grad_v)  # tables uploaded, kernels loaded: what follows can only add launches
    buf, out = guarded(nd)
    spare = torch.zeros(2 * 36 * n + 2, dtype=torch.float64, device="cuda")
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        for call in (lambda **kw: f(stress, **kw), lambda **kw: f.tangent_action(tangent, grad_v, **kw)):
            with pytest.raises(ValueError, match="aligned"):
                call(out=buf[MARGIN + 1: MARGIN + 1 + nd])
            with pytest.raises(ValueError, match="entries"):
                call(out=buf[MARGIN: MARGIN + nd - 3])
            with pytest.raises(ValueError, match="contiguous"):
                call(out=spare[: 2 * nd: 2])
            with pytest.raises(ValueError, match="cuda"):
                call(out=torch.empty(nd, dtype=torch.float64))  # on the host
            with pytest.raises(TypeError):
                call(out=out.float())
            with pytest.raises(ValueError, match="accumulate"):
                call(accumulate=True)
        with pytest.raises(ValueError, match="entries"):
            f(stress[:-6], out=out)
        with pytest.raises(ValueError, match="aligned"):
            f(spare[1: 1 + 6 * n], out=out)
        with pytest.raises(ValueError, match="contiguous"):
            f(spare[: 12 * n: 2], out=out)
        with pytest.raises(ValueError, match="cuda"):
            f(stress.cpu(), out=out)
        with pytest.raises(TypeError):
            f(t["stress"], out=out)
        with pytest.raises(ValueError, match="entries"):
            f.tangent_action(tangent[:-36], grad_v, out=out)
        with pytest.raises(ValueError, match="entries"):
            f.tangent_action(tangent, grad_v[:-9], out=out)
        with pytest.raises(ValueError, match="aligned"):
            f.tangent_action(spare[1: 1 + 36 * n], grad_v, out=out)
        with pytest.raises(ValueError, match="aligned"):
            f.tangent_action(tangent, spare[1: 1 + 9 * n], out=out)
        with pytest.raises(ValueError, match="contiguous"):
            f.tangent_action(tangent, spare[: 18 * n: 2], out=out)
        with pytest.raises(ValueError, match="cuda"):
            f.tangent_action(tangent, grad_v.cpu(), out=out)
        with pytest.raises(TypeError):
            f.tangent_action(tangent.float(), grad_v, out=out)
        if torch.cuda.device_count() > 1:
            with pytest.raises(ValueError, match="cuda"):
                f(stress.to("cuda:1"), out=out)
    finally:
        jit.launch = real
    torch.cuda.synchronize()
    assert not launches
    assert (bits(to_host(buf)) == CANARY).all()
    # an empty mesh: zeros, or out as it is under accumulate
    t0 = random_inputs("hex8", 1, 2, False, False)
    empty = fc.InternalForce(fc.DisplacementGradient(t0["dofmap"][:0], t0["ref"], t0["jinv"][:0], 5), t0["weights"][:0])
    none = torch.zeros(0, dtype=torch.float64, device="cuda")
    assert (to_host(empty(none)) == 0.0).all() and empty(none).numel() == 15
    keep = to_device(np.arange(15.0), "cuda")
    assert empty.tangent_action(none, none, out=keep, accumulate=True) is keep and np.array_equal(to_host(keep), np.arange(15.0))
    assert (to_host(empty(none, out=keep)) == 0.0).all()
