"""BiCGStab on the matrix-free tangent operator on the GPU (fenics_constitutive_amd.MatrixFreeBiCGStab, csrc/jit/bicgstab_free.hip):
the node-dots kernel alone and whole runs compared ON THE BITS with the NumPy oracle of bicgstab_free_util.py -- unsymmetric tangents,
without a preconditioner, with block-Jacobi and with both multilevel cycles, with and without a start vector, under a grid capped at
one compute unit, for every ``check_every`` --, every output between canaries; the statuses, the refusals, the other routes untouched
behind it, the system the conjugate gradients do not solve, and the Newton loop of examples/cube_tension_matrix_free_nonsymmetric.py."""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_constraints, tension_test_device_solve  # noqa: E402
from cube_tension_matrix_free import cube_operators  # noqa: E402
from cube_tension_matrix_free_nonsymmetric import MatrixFreeNonsymmetricLoop  # noqa: E402
from cube_tension_nonsymmetric import DP_P, TOP_DISPLACEMENT, drucker_prager  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import bicgstab, bicgstab_free, gradient, jit, solver  # noqa: E402
from fenics_constitutive_amd import tangent_operator as to  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402
from bicgstab_free_util import K_CYCLES, K_ITERATIONS, K_SHAPES, k_iterations_system, operator_solve  # noqa: E402
from bicgstab_util import nonassociated_tangent  # noqa: E402
from fe_gpu_util import CANARY, MARGIN, bits, guarded, assert_margins_intact, assert_same_bits, solve_guarded, assert_same_result, tables_of  # noqa: E402
from fe_gpu_util import one_cu  # noqa: E402, F401 (the fixture: pytest finds it in this namespace)
from force_util import MANDEL_DIM, random_inputs  # noqa: E402
from gradient_util import cube_operator_tables  # noqa: E402
from multilevel_free_util import FreeOracle  # noqa: E402
from solver_util import SEG, ordered_dot, spd_tangent  # noqa: E402
from tangent_operator_util import TILING_SHAPES, distinct_inputs, product_oracle  # noqa: E402
from tangent_operator_util import operator_solve as cg_operator_solve  # noqa: E402

TO_SHAPES = ("hex8", "tet_p2", "tri_p2", "interval")
CYCLES = K_CYCLES
KINDS = (None, "block_jacobi") + CYCLES
BREAKDOWN = bicgstab.STATUSES.index("breakdown")
ITERATING = (to.ELEMENT_KERNEL, bicgstab_free.NODE_DOTS_KERNEL, bicgstab.HALF_KERNEL, to.ELEMENT_KERNEL, bicgstab_free.NODE_DOTS_KERNEL, bicgstab.FULL_KERNEL,
             bicgstab.DIRECTION_KERNEL)


def same_number(have, want):
    return bits(np.float64(have)) == bits(np.float64(want))


def operator_of(t):
    return fc.TangentOperator(fc.InternalForce(fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"]), t["weights"]))


def preconditioners(a, tables, kind, mask, **options):
    """(the device solver's ``preconditioner``, the oracle's) of one kind"""
    if kind in CYCLES:
        return fc.MultilevelPreconditioner(a, cycle=kind, **options), FreeOracle(*tables, mask=mask, cycle=kind, **options)
    return kind, kind


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel alone
# ---------------------------------------------------------------------------------------------------------------------------------
def mesh_of(shape, n_nodes, seed):
    """random tables of ``shape`` over exactly ``n_nodes`` nodes: every node but ``lonely`` (in the middle of the numbering) in a cell,
    the cells' nodes distinct; the tangent random and unsymmetric (force_util.random_inputs)"""
    d_, a_, q_, affine = TILING_SHAPES[shape]
    n_used = n_nodes - 1
    assert n_used >= a_
    cover = -(-n_used // a_)
    n_cells = cover + max(2, cover // 2)
    t = random_inputs(TILING_SHAPES[shape], n_cells, seed, False, affine)
    rng = np.random.default_rng(seed + 3000)
    dofmap = np.stack([(c * a_ + np.arange(a_)) % n_used if c < cover else rng.permutation(n_used)[:a_] for c in range(n_cells)])
    lonely = n_nodes // 2
    t["dofmap"] = np.where(dofmap >= lonely, dofmap + 1, dofmap).astype(np.int32)
    t["n_nodes"], t["lonely"] = n_nodes, lonely
    assert (np.diff(np.sort(t["dofmap"], axis=1), axis=1) > 0).all()
    assert np.array_equal(np.flatnonzero(np.bincount(t["dofmap"].reshape(-1), minlength=n_nodes) == 0), [lonely])
    return t


def check_product(a, tangent_dev, va, vb, what, launches=None):
    """bicgstab_free.product in both dot modes between canaries against A(tangent, va) and solver_util.ordered_dot; returns q"""
    n = a.shape[0]
    va_dev, vb_dev = to_device(va, "cuda"), to_device(vb, "cuda")
    control = bicgstab_free._product(a).control(a.device)
    results = []
    for both in (False, True):
        buf, out = guarded(n)
        if launches is not None:
            del launches[:]
        got = bicgstab_free.product(a, tangent_dev, va_dev, vb_dev, both=both, out=out)
        if launches is not None:
            assert launches == [(to.ELEMENT_KERNEL, gradient.BLOCKS_PER_CU), (bicgstab_free.NODE_DOTS_KERNEL, gradient.BLOCKS_PER_CU)], launches
        assert got[0].data_ptr() == out.data_ptr() and len(got) == (3 if both else 2)
        torch.cuda.synchronize()
        assert_margins_intact(buf, n)
        q = to_host(out)
        results.append(q)
        assert all(np.isfinite(d) and d != 0.0 for d in got[1:]) and int(control.ints[solver._STATUS]) == 0, (what, both, got[1:])  # still "running"
        assert int(control.ints[solver._COUNTER]) == 0 and int(control.ints[solver._ITERATIONS]) == 0, what
        assert same_number(got[1], ordered_dot(q, vb)), (what, both, got[1], ordered_dot(q, vb))
        if both:
            assert same_number(got[2], ordered_dot(q, q)), (what, got[2], ordered_dot(q, q))
            assert same_number(control.host[bicgstab_free._OMEGA], np.float64(got[1]) / np.float64(got[2])), what
    assert_same_bits(results[0], results[1], f"{what}: the two dot modes' q")
    assert_same_bits(results[0], to_host(a(tangent_dev, va_dev)), f"{what}: q against A(tangent, va)")
    assert_same_bits(to_host(va_dev), va, f"{what}: va was written")
    assert_same_bits(to_host(vb_dev), vb, f"{what}: vb was written")
    return results[0]


@pytest.mark.parametrize("shape", ["interval", "tri_p2", "hex8"])
def test_the_kernel_alone(shape):
    d_ = TILING_SHAPES[shape][0]
    for target in (200, SEG, SEG + 1, 2 * SEG + 5):  # dofs: below a block, a segment, one past, two and a ragged third
        n_nodes = -(-target // d_)  # (D = 2: 3074 and 6150 dofs, D = 3: 201, 3075 and 6150: the nearest above a node count allows)
        t = mesh_of(shape, n_nodes, 40 + target)
        a = operator_of(t)
        n = a.shape[0]
        assert target <= n < target + d_ and (target != SEG or n == SEG)
        rng = np.random.default_rng(target)
        va, vb = rng.normal(size=n), rng.normal(size=n)
        tangent_dev = to_device(t["tangent"], "cuda")
        mask = rng.random(n) < 0.2
        mask.reshape(-1, d_)[t["lonely"]] = False  # (a constrained dof needs a cell)
        for m in (None, mask):
            a.set_constrained(m)
            what = f"{shape} {n} dofs mask={'yes' if m is not None else 'no'}"
            q = check_product(a, tangent_dev, va, vb, what)
            assert (bits(q.reshape(-1, d_)[t["lonely"]]) == 0).all(), what  # the node of no cell: +0.0
            if m is not None:
                assert m.any() and np.array_equal(bits(q[m]), bits(va[m])), what
            if target == 200:
                assert_same_bits(q, product_oracle(t["tangent"], va, *tables_of(t), mask=m), f"{what}: the oracle")
            # a zero vb: breakdown in the control block, q written all the same
            buf, out = guarded(n)
            for both in (False, True):
                got = bicgstab_free.product(a, tangent_dev, to_device(va, "cuda"), torch.zeros(n, dtype=torch.float64, device="cuda"), both=both, out=out)
                control = bicgstab_free._product(a).control(a.device)
                assert int(control.ints[solver._STATUS]) == BREAKDOWN and bits(np.float64(got[1])) == 0, (what, both)
                assert_margins_intact(buf, n)
                assert_same_bits(to_host(out), q, f"{what}: q behind a zero vb")
        q, dot = bicgstab_free.product(a, tangent_dev, to_device(va, "cuda"), to_device(vb, "cuda"))  # without out: a new tensor
        assert q.shape == (n,) and same_number(dot, ordered_dot(to_host(q), vb))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. on one compute unit
# ---------------------------------------------------------------------------------------------------------------------------------
def interval_mesh(n_nodes):
    """a chain of two-node cells over n_nodes nodes (D = 1: the dofs are the nodes), lengths and tangent random"""
    rng = np.random.default_rng(n_nodes)
    dofmap = np.stack([np.arange(n_nodes - 1), np.arange(1, n_nodes)], axis=1).astype(np.int32)
    h = rng.uniform(0.5, 1.5, size=n_nodes - 1)
    return dict(dofmap=dofmap, ref=np.array([[[-1.0], [1.0]]]), jinv=np.ascontiguousarray((1.0 / h)[:, None, None]), weights=h[:, None].copy(),
                n_nodes=n_nodes, tangent=rng.uniform(1.0, 2.0, size=n_nodes - 1))


def test_the_kernel_on_one_compute_unit(one_cu):
    n_nodes = 17 * SEG + 5  # 18 segments: more than the 16 blocks one compute unit is capped at
    t = interval_mesh(n_nodes)
    a = operator_of(t)
    mask = np.zeros(n_nodes, dtype=bool)
    mask[[0, n_nodes // 3]] = True
    a.set_constrained(mask)
    rng = np.random.default_rng(1)
    va, vb = rng.normal(size=n_nodes), rng.normal(size=n_nodes)
    q = check_product(a, to_device(t["tangent"], "cuda"), va, vb, f"interval {n_nodes} on one compute unit", launches=one_cu)
    assert_same_bits(q, product_oracle(t["tangent"], va, *tables_of(t), mask=mask), "one compute unit: the oracle")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. exactly k iterations
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K_SHAPES)
def test_exactly_k_iterations(shape):
    assert K_SHAPES == TO_SHAPES + ("q3", "odd33_3d", "wide70") and K_ITERATIONS == (1, 2, 5)
    t, mask, tangent, b, start = k_iterations_system(shape)
    tables = tables_of(t)
    a = operator_of(t)
    a.set_constrained(mask)
    tangent_dev = to_device(tangent, "cuda")
    for kind in KINDS:
        if kind in CYCLES and shape == "wide70":  # no element matrix of 210 x 210: the preconditioner itself refuses the shape
            with pytest.raises(ValueError, match="does not compile without scratch"):
                fc.MultilevelPreconditioner(a, cycle=kind, coarsest_nodes=4)
            continue
        pc, oracle_pc = preconditioners(a, tables, kind, mask, **({"coarsest_nodes": 4} if kind in CYCLES else {}))
        for its in K_ITERATIONS:
            s = fc.MatrixFreeBiCGStab(a, preconditioner=pc, rtol=0.0, maxiter=its)
            for x0 in (None, start):
                what = f"{shape} {kind} k={its} x0={'yes' if x0 is not None else 'no'}"
                want = operator_solve(tangent, b, *tables, mask=mask, x0=x0, preconditioner=oracle_pc, rtol=0.0, maxiter=its)
                res, x = solve_guarded(s, tangent_dev, b, x0)
                assert want.status == "maxiter" and want.iterations == its, what
                assert_same_result(res, x, want, what)
        if kind in CYCLES:
            assert len(pc.levels) >= 2
    x0_dev = to_device(start, "cuda")
    res = s(tangent_dev, to_device(b, "cuda"), x0=x0_dev)  # without out: a new tensor, x0 untouched
    assert res.x.data_ptr() != x0_dev.data_ptr() and np.array_equal(to_host(x0_dev), start)
    assert_same_bits(to_host(res.x), want.x, f"{shape}: without out")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. a cube with two segments: check_every, the statuses, what stays untouched behind a solve
# ---------------------------------------------------------------------------------------------------------------------------------
RUNS = ((("rtol", 0.0), ("maxiter", 11)), (("rtol", 1e-6),))


@pytest.fixture(scope="module")
def cube_system():
    """the tension-test operator of a 10 x 10 x 9 cube of hexahedra (3630 dofs: two segments; levels 1210, 48, 4 at coarsest_nodes=32)
    with the non-associated tangent of bicgstab_util (b = 0.6, b_flow = 0 at 30 % of the points) and its right-hand side; ``oracle(kind,
    kw)``: the oracle's solve, made once"""
    mesh = FE.Cube(10, 10, 9)
    op, f = cube_operators(mesh)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    tables = (dofmap, ref, jinv, f._weights, mesh.n_nodes)
    mask, _ = tension_constraints(mesh)
    assert SEG < mesh.n_dofs <= 2 * SEG
    tangent = nonassociated_tangent(mesh.n_points)
    b = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mesh.n_dofs))
    a = fc.TangentOperator(f)
    a.set_constrained(mask)
    made = {}

    def oracle(kind, kw):
        if (kind, kw) not in made:
            pc = FreeOracle(*tables, mask=mask, cycle=kind, coarsest_nodes=32) if kind in CYCLES else kind
            made[(kind, kw)] = operator_solve(tangent, b, *tables, mask=mask, preconditioner=pc, **dict(kw))
        return made[(kind, kw)]

    return mesh, f, tables, mask, tangent, b, a, oracle


@pytest.mark.parametrize("kind", KINDS, ids=[str(kind) for kind in KINDS])
def test_check_every_changes_nothing(kind, cube_system):
    mesh, f, tables, mask, tangent, b, a, oracle = cube_system
    pc = fc.MultilevelPreconditioner(a, cycle=kind, coarsest_nodes=32) if kind in CYCLES else kind
    tangent_dev = to_device(tangent, "cuda")
    for kw in RUNS:
        want = oracle(kind, kw)
        assert want.status == ("maxiter" if "maxiter" in dict(kw) else "converged") and want.iterations >= (11 if kind in (None, "block_jacobi") else 4), want.iterations
        for every in (1, 3, 16):  # (11 iterations end in the middle of a batch of 3 and of 16; so does the converged solve's last)
            res, x = solve_guarded(fc.MatrixFreeBiCGStab(a, preconditioner=pc, check_every=every, **dict(kw)), tangent_dev, b)
            assert_same_result(res, x, want, f"{kind} {dict(kw)} check_every={every}")
            assert res.looks == 1 + -(-want.iterations // every)


def test_statuses(cube_system):
    mesh, f, tables, mask, tangent, b, a, oracle = cube_system
    n = b.size
    start = np.random.default_rng(2).normal(size=n)
    tangent_dev = to_device(tangent, "cuda")
    bad_b = b.copy()
    bad_b[17] = np.nan
    bad_tangent = tangent.copy()
    bad_tangent[36 * (mesh.n_points // 2) + 7] = np.inf
    for kind in KINDS:
        pc, oracle_pc = preconditioners(a, tables, kind, mask, **({"coarsest_nodes": 32} if kind in CYCLES else {}))
        s = fc.MatrixFreeBiCGStab(a, preconditioner=pc, rtol=1e-6)
        # b = 0: converged at the start, no 0/0
        for x0 in (None, np.zeros(n)):
            res, x = solve_guarded(s, tangent_dev, np.zeros(n), x0)
            assert (res.status, res.iterations, res.converged, res.residual_norm, res.rhs_norm, res.looks) == ("converged", 0, True, 0.0, 0.0, 1)
            assert (bits(x) == 0).all()
        # maxiter 0: x is x0
        res, x = solve_guarded(fc.MatrixFreeBiCGStab(a, preconditioner=pc, maxiter=0), tangent_dev, b, start)
        assert (res.status, res.iterations, res.looks) == ("maxiter", 0, 1)
        assert_same_bits(x, start, f"{kind}: maxiter 0")
        # a NaN in b
        res, x = solve_guarded(s, tangent_dev, bad_b)
        assert (res.status, res.iterations, res.looks) == ("nonfinite", 0, 1)
        # an all-zero tangent: every free node's own block is zero -- no iteration, x is x0
        if kind is not None:
            res, x = solve_guarded(s, np.zeros_like(tangent), b, start)
            assert (res.status, res.iterations, res.converged, res.looks) == ("singular_block", 0, False, 1)
            assert_same_bits(x, start, f"{kind}: singular block")
        # and the object solves again afterwards
        res, x = solve_guarded(s, tangent_dev, b)
        assert_same_result(res, x, oracle(kind, RUNS[1]), f"{kind}: after the statuses")
    # a non-finite tangent entry: the residual of the start b - A x0 is not finite
    s = fc.MatrixFreeBiCGStab(a, preconditioner=None, rtol=1e-6)
    res, x = solve_guarded(s, bad_tangent, b, start)
    want = operator_solve(bad_tangent, b, *tables, mask=mask, x0=start, preconditioner=None, rtol=1e-6)
    assert (res.status, res.iterations, res.converged, res.looks) == (want.status, want.iterations, False, 1) == ("nonfinite", 0, False, 1)
    assert_same_bits(x, start, "a non-finite tangent entry")


def test_breakdown_and_the_half_step_exit():
    """the small integer systems of test_gpu_bicgstab.py carried over to an operator: a tangent that couples the normal strains alone by
    a skew-symmetric matrix of small integers over integer tables (no factor sqrt(0.5) takes part: every sum is exact), so that
    ``w^T A w`` is exactly zero for every integer ``w`` in every summation order; and the identity"""
    t = distinct_inputs("hex8", 40, 9, True, True, every_node=True)
    tables = tables_of(t)
    a = operator_of(t)
    n = a.shape[0]
    rng = np.random.default_rng(3)
    m = rng.integers(-3, 4, size=(40 * 8, 3, 3)).astype(np.float64)
    skew = np.zeros((40 * 8, 6, 6))
    skew[:, :3, :3] = m - m.transpose(0, 2, 1)
    skew = skew.reshape(-1)
    ints = np.random.default_rng(4).integers(-4, 5, size=n).astype(np.float64)
    start = np.random.default_rng(5).integers(-4, 5, size=n).astype(np.float64)
    a.set_constrained(None)
    v = product_oracle(skew, ints, *tables)
    assert np.abs(v).max() > 0 and ordered_dot(v, ints) == 0.0 and float(v @ ints) == 0.0
    s = fc.MatrixFreeBiCGStab(a, preconditioner=None)
    res, x = solve_guarded(s, skew, ints)
    assert (res.status, res.iterations, res.converged, res.looks) == ("breakdown", 0, False, 2)
    assert (bits(x) == 0).all()
    assert_same_result(res, x, operator_solve(skew, ints, *tables, preconditioner=None), "breakdown")
    want = operator_solve(skew, ints, *tables, x0=start, preconditioner=None, maxiter=3)
    res, x = solve_guarded(fc.MatrixFreeBiCGStab(a, preconditioner=None, maxiter=3), skew, ints, start)
    assert_same_result(res, x, want, "the skew-symmetric operator with a start vector")
    # the identity (every dof constrained): s = r - (rho / rv) v is zero, the solve ends at the half step of its first iteration
    every = np.ones(n, dtype=bool)
    a.set_constrained(every)
    tangent = spd_tangent(40 * 8, 6, 1, False)
    rhs = np.random.default_rng(6).normal(size=n)
    for kind in (None, "block_jacobi"):
        want = operator_solve(tangent, rhs, *tables, mask=every, x0=start, preconditioner=kind)
        res, x = solve_guarded(fc.MatrixFreeBiCGStab(a, preconditioner=kind), tangent, rhs, start)
        assert (want.status, want.iterations, want.residual_norm) == ("converged", 1, 0.0)
        assert_same_result(res, x, want, f"{kind}: the half-step exit")
        assert res.looks == 2 and np.allclose(x, rhs, rtol=1e-14, atol=1e-14)  # x = x0 + 1.0 * (rhs - x0), rounded twice


def test_on_one_compute_unit(one_cu):
    """a whole solve under the cap: 18 segments on the 16 blocks of one compute unit, every launch of the iteration in its order"""
    n_nodes = 17 * SEG + 5
    t = interval_mesh(n_nodes)
    a = operator_of(t)
    mask = np.zeros(n_nodes, dtype=bool)
    mask[[0, n_nodes // 3]] = True
    a.set_constrained(mask)
    rng = np.random.default_rng(3)
    b, start = np.where(mask, 0.0, rng.normal(size=n_nodes)), rng.normal(size=n_nodes)
    for kind, x0 in (("block_jacobi", start), (None, None)):
        del one_cu[:]
        res, x = solve_guarded(fc.MatrixFreeBiCGStab(a, preconditioner=kind, rtol=0.0, maxiter=2, check_every=2), t["tangent"], b, x0)
        assert_same_result(res, x, operator_solve(t["tangent"], b, *tables_of(t), mask=mask, x0=x0, preconditioner=kind, rtol=0.0, maxiter=2),
                           f"interval {n_nodes} {kind}, one compute unit")
        assert {nb for name, nb in one_cu} == {gradient.BLOCKS_PER_CU}  # every launch really was capped
        names = [name for name, _ in one_cu]
        assert names[-14:] == 2 * list(ITERATING) and names[-15] == bicgstab.START_KERNEL
        assert bicgstab.PRODUCT_KERNEL not in names and solver.MATVEC_KERNEL not in names  # no kernel that reads a matrix
        assert (to.NODE_KERNEL in names) == (x0 is not None) and (solver.INVERSE_KERNEL in names) == (kind is not None)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the reason for the feature, on the device
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_unsymmetric_system_conjugate_gradients_do_not_solve():
    """test_gpu_bicgstab.py's system -- Cube(3, 2, 4), b = 0.6, b_flow = 0 at 30 % of the points -- without a matrix: the conjugate
    gradients on the operator do not end converged, MatrixFreeBiCGStab converges on the oracle's bits"""
    mesh = FE.Cube(3, 2, 4)
    op, f = cube_operators(mesh)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    tables = (dofmap, ref, jinv, f._weights, mesh.n_nodes)
    mask, _ = tension_constraints(mesh)
    a = fc.TangentOperator(f)
    a.set_constrained(mask)
    tangent = nonassociated_tangent(mesh.n_points, b=0.6, b_flow=0.0, H=2000.0, frac=0.3, seed=5)
    rhs = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mesh.n_dofs))
    res, x = solve_guarded(fc.ConjugateGradient(a, maxiter=10 * mesh.n_dofs, check_every=256), tangent, rhs)
    assert not res.converged and res.status in ("indefinite", "maxiter")
    for kind in (None, "block_jacobi"):
        want = operator_solve(tangent, rhs, *tables, mask=mask, preconditioner=kind)
        res, x = solve_guarded(fc.MatrixFreeBiCGStab(a, preconditioner=kind), tangent, rhs)
        assert_same_result(res, x, want, f"{kind}: the unsymmetric system")
        assert res.converged and res.iterations <= 200
        assert np.linalg.norm(rhs - product_oracle(tangent, x, *tables, mask=mask)) <= 1e-7 * np.linalg.norm(rhs)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the other routes keep their bits
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_other_routes_keep_their_bits(cube_system):
    """ConjugateGradient(A) with block-Jacobi and with the shared multilevel instance, BiCGStab(K) and pc.apply give identical results
    before and after MatrixFreeBiCGStab solves that share A and pc (the launch plans of the source / destination pairs live side by
    side; the control blocks and work vectors are each solver's own)"""
    mesh, f, tables, mask, tangent, b, a, oracle = cube_system
    spd_dev, tangent_dev, b_dev = to_device(spd_tangent(mesh.n_points, 6, 1, False), "cuda"), to_device(tangent, "cuda"), to_device(b, "cuda")
    pc = fc.MultilevelPreconditioner(a, cycle="additive", coarsest_nodes=32)
    k = fc.TangentMatrix(f)
    k.set_constrained(mask)
    values = k(tangent_dev)
    routes = {"ConjugateGradient(A)": lambda: fc.ConjugateGradient(a, rtol=0.0, maxiter=7)(spd_dev, b_dev),
              "ConjugateGradient(A, pc)": lambda: fc.ConjugateGradient(a, preconditioner=pc, rtol=0.0, maxiter=7)(spd_dev, b_dev),
              "BiCGStab(K)": lambda: fc.BiCGStab(k, rtol=0.0, maxiter=7)(values, b_dev)}

    def run():
        out = {}
        for name, route in routes.items():
            res = route()
            out[name] = (to_host(res.x), res.iterations, res.status, res.residual_norm, res.rhs_norm)
        out["pc.apply"] = (to_host(pc.apply(spd_dev, b_dev)), 0, "", 0.0, 0.0)
        return out

    before = run()
    assert all(before[name][2] == "maxiter" and before[name][1] == 7 for name in routes)
    for kind, oracle_kind in ((pc, "additive"), ("block_jacobi", "block_jacobi")):
        res, x = solve_guarded(fc.MatrixFreeBiCGStab(a, preconditioner=kind, rtol=1e-6), tangent_dev, b)
        assert_same_result(res, x, oracle(oracle_kind, RUNS[1]), f"{oracle_kind}: the solve in between")
    after = run()
    for name in before:
        assert_same_bits(after[name][0], before[name][0], f"{name} behind MatrixFreeBiCGStab")
        assert after[name][1:3] == before[name][1:3] and same_number(after[name][3], before[name][3]) and same_number(after[name][4], before[name][4]), name
    # and the operator route agrees with the matrix route to rounding: the two products round differently
    free, _ = solve_guarded(fc.MatrixFreeBiCGStab(a, rtol=0.0, maxiter=7), tangent_dev, b)
    assert np.allclose(to_host(free.x), after["BiCGStab(K)"][0], rtol=1e-7, atol=1e-10 * np.abs(after["BiCGStab(K)"][0]).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. refusals come before any launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(cube_system):
    mesh, f, tables, mask, tangent, b, a, oracle = cube_system
    n, nt = a.shape[0], tangent.size
    solvers = [fc.MatrixFreeBiCGStab(a, rtol=1e-6), fc.MatrixFreeBiCGStab(a, preconditioner=fc.MultilevelPreconditioner(a, coarsest_nodes=32), rtol=1e-6)]
    tangent_dev, b_dev = to_device(tangent, "cuda"), to_device(b, "cuda")
    for s in solvers:
        assert s(tangent_dev, b_dev).converged  # tables uploaded, kernels loaded: what follows can only add launches
    bicgstab_free.product(a, tangent_dev, b_dev, b_dev)
    buf, out = guarded(n)
    spare = torch.zeros(2 * max(n, nt) + 2, dtype=torch.float64, device="cuda")
    # tensors on the host made there: ``tensor.cpu()`` of 2 MB would hand pageable memory to the HIP runtime, whose cache of page
    # locks then outlives the array (hostio.py) and spoils the host path of whatever runs later in the process
    host_tangent, host_b = torch.zeros(nt, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        calls = [lambda s=s, **kw: s(kw["tangent"], kw["v"], out=kw["out"]) for s in solvers]
        calls.append(lambda **kw: bicgstab_free.product(a, kw["tangent"], kw["v"], b_dev, out=kw["out"]))
        for call in calls:
            ok = dict(tangent=tangent_dev, v=b_dev, out=out)
            with pytest.raises(ValueError, match="aligned"):
                call(**{**ok, "out": buf[MARGIN + 1: MARGIN + 1 + n]})
            with pytest.raises(ValueError, match="entries"):
                call(**{**ok, "out": buf[MARGIN: MARGIN + n - 3]})
            with pytest.raises(ValueError, match="contiguous"):
                call(**{**ok, "out": spare[: 2 * n: 2]})
            with pytest.raises(ValueError, match="cuda"):
                call(**{**ok, "out": torch.empty(n, dtype=torch.float64)})
            with pytest.raises(TypeError):
                call(**{**ok, "out": out.float()})
            with pytest.raises(ValueError, match="alias"):
                call(**{**ok, "out": b_dev})
            with pytest.raises(ValueError, match="entries"):
                call(**{**ok, "tangent": tangent_dev[:-36]})
            with pytest.raises(ValueError, match="aligned"):
                call(**{**ok, "tangent": spare[1: 1 + nt]})
            with pytest.raises(TypeError):
                call(**{**ok, "tangent": tangent})  # an ndarray
            with pytest.raises(TypeError):
                call(**{**ok, "tangent": tangent_dev.float()})
            with pytest.raises(ValueError, match="cuda"):
                call(**{**ok, "tangent": host_tangent})
            with pytest.raises(ValueError, match="entries"):
                call(**{**ok, "v": b_dev[:-3]})
            with pytest.raises(ValueError, match="contiguous"):
                call(**{**ok, "v": spare[: 2 * n: 2]})
            with pytest.raises(TypeError):
                call(**{**ok, "v": b})  # an ndarray
            with pytest.raises(TypeError):
                call(**{**ok, "v": b_dev.float()})
            with pytest.raises(ValueError, match="cuda"):
                call(**{**ok, "v": host_b})
        for s in solvers:
            with pytest.raises(ValueError, match="x0 itself"):
                s(tangent_dev, b_dev, x0=spare[2: 2 + n], out=spare[:n])
            with pytest.raises(ValueError, match="contiguous"):
                s(tangent_dev, b_dev, x0=spare[: 2 * n: 2], out=out)
        with pytest.raises(ValueError, match="alias"):
            bicgstab_free.product(a, tangent_dev, b_dev, spare[:n], out=spare[:n])
        with pytest.raises(ValueError, match="multilevel"):
            fc.MatrixFreeBiCGStab(a, preconditioner="multilevel")
        with pytest.raises(ValueError, match="another object"):
            fc.MatrixFreeBiCGStab(a, preconditioner=fc.MultilevelPreconditioner(fc.TangentMatrix(f)))
        with pytest.raises(TypeError):
            fc.MatrixFreeBiCGStab(fc.TangentMatrix(f))
        with pytest.raises(TypeError):
            fc.BiCGStab(a)
    finally:
        jit.launch = real
    torch.cuda.synchronize()
    assert launches == []
    assert (bits(to_host(buf)) == CANARY).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the Newton loop of the example
# ---------------------------------------------------------------------------------------------------------------------------------
def test_in_the_loop_of_the_example():
    """examples/cube_tension_matrix_free_nonsymmetric.py on Cube(3, 2, 4): DruckerPrager3D with b = 0.15, b_flow = 0, eight load steps,
    MatrixFreeBiCGStab(rtol=1e-12) with block-Jacobi and with the additive cycle: the Newton counts per step of the direct (SciPy) solve
    on the host, the largest relative reaction difference at most 1e-8, the bound the examples assert; no matrix anywhere in the loop"""
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    state = FE.CopyProtocolState(FE.OracleLaw(O.comfe_drucker_prager, DP_P, {"history": 7}), mesh.n_points)
    with np.errstate(all="ignore"):
        r_direct, norms_direct, _ = FE.tension_test(mesh, state, steps=8, top_displacement=TOP_DISPLACEMENT)
    scale = np.max(np.abs(r_direct))
    for pc, options in (("block_jacobi", {}), ("additive", {"coarsest_nodes": 8})):
        loop = MatrixFreeNonsymmetricLoop(mesh, drucker_prager(), pc, rtol=1e-12, **options)
        r_gpu, norms_gpu, u, solves = tension_test_device_solve(mesh, loop, steps=8, top_displacement=TOP_DISPLACEMENT)  # (raises where a solve does not converge)
        difference = np.max(np.abs(r_gpu - r_direct)) / scale
        counts = [len(h) for h in norms_gpu]
        print(f"matrix-free nonsymmetric tension test, {pc}: GPU against direct {difference:.3e}, Newton iterations {counts}, BiCGStab iterations {solves}")
        assert counts == [len(h) for h in norms_direct] == [2, 3, 3, 4, 6, 6, 6, 6]
        assert loop.solves == len(solves) == sum(counts) - 8
        assert isinstance(loop.cg, fc.MatrixFreeBiCGStab) and not any(isinstance(x, fc.TangentMatrix) for x in vars(loop).values())
        c = to_host(loop.rs.tangent).reshape(-1, 6, 6)
        assert np.abs(c - c.transpose(0, 2, 1)).max() >= 1e-3 * np.abs(c).max()  # the last tangent is not symmetric
        assert difference <= 1e-8, difference
