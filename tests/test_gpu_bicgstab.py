"""The device BiCGStab on the GPU (fenics_constitutive_amd.BiCGStab, csrc/jit/bicgstab.hip): whole runs compared ON THE BITS with
the NumPy oracle of bicgstab_util.py -- unsymmetric matrices in both formats, without a preconditioner, with block-Jacobi and with
both multilevel cycles, with and without a start vector, under a grid capped at one compute unit, for every ``check_every`` --, the
statuses, the refusals, the conjugate gradients and the standalone preconditioner untouched behind it, the system the conjugate
gradients do not solve, and the Newton loop of examples/cube_tension_nonsymmetric.py."""

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
from cube_tension_nonsymmetric import DP_P, TOP_DISPLACEMENT, drucker_prager, nonsymmetric_loop  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import bicgstab, gradient, jit, multilevel, solver  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402
from bicgstab_util import asymmetry, nonassociated_tangent, skew_blocks  # noqa: E402
from bicgstab_util import bicgstab as oracle_bicgstab  # noqa: E402
from fe_gpu_util import CANARY, MARGIN, bits, guarded, assert_margins_intact, assert_same_bits, solve_guarded, assert_same_result  # noqa: E402
from fe_gpu_util import one_cu  # noqa: E402, F401 (the fixture: pytest finds it in this namespace)
from force_util import random_inputs  # noqa: E402
from gradient_util import SHAPES  # noqa: E402
from matrix_util import csr_values  # noqa: E402
import multilevel_util as MU  # noqa: E402
from solver_util import SEG, conjugate_gradient, from_format, full_pattern, spd_tangent  # noqa: E402

FORMATS = ("bsr", "csr")
BCG_SHAPES = ("hex8", "tet_p2", "tri_p2", "interval")
CYCLES = ("multiplicative", "additive")
KINDS = (None, "block_jacobi") + CYCLES
ITERATING = (bicgstab.PRODUCT_KERNEL, bicgstab.HALF_KERNEL, bicgstab.FULL_KERNEL, bicgstab.DIRECTION_KERNEL)


def preconditioners(k, kind, mask, **options):
    """(the device solver's ``preconditioner``, the oracle's) of one kind"""
    if kind in CYCLES:
        return fc.MultilevelPreconditioner(k, cycle=kind, **options), MU.Oracle(k.indptr, k.indices, cycle=kind, mask=mask, **options)
    return kind, kind


def to_format(fmt, indptr, indices, blocks):
    return blocks.reshape(-1) if fmt == "bsr" else csr_values(indptr, indices, blocks)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. exactly k iterations on unsymmetric random matrices
# ---------------------------------------------------------------------------------------------------------------------------------
def assembled(shape, n_cells, seed, fmt, fraction=0.2):
    """(K, values on the device, blocks on the host, mask): the matrix of force_util's UNSYMMETRIC random tangent over random tables,
    every node with a block of its own (the nodes no cell touches: constrained), random constrained dofs and, in the meshes of more
    than five cells (the smaller ones are one aggregate), all dofs of the members of aggregate 0 constrained"""
    d_, a_, q_, affine = SHAPES[shape]
    t = random_inputs(shape, n_cells, seed, False, affine)
    f = fc.InternalForce(fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"]), t["weights"])
    pat, unused = full_pattern(t["dofmap"], t["n_nodes"])
    k = fc.TangentMatrix(f, format=fmt, pattern_dofmap=pat)
    used = np.ones(t["n_nodes"], dtype=bool)
    used[unused] = False
    mask = ((np.random.default_rng(seed + 5).random(d_ * t["n_nodes"]) < fraction) & np.repeat(used, d_)) | np.repeat(~used, d_)
    agg, _ = multilevel.aggregate(k.indptr, k.indices)
    if n_cells > 5:
        mask |= np.repeat(agg == 0, d_)
    k.set_constrained(mask)
    values = k(to_device(t["tangent"], "cuda"))
    torch.cuda.synchronize()
    return k, values, from_format(fmt, k.indptr, k.indices, to_host(values), d_), mask


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", BCG_SHAPES)
def test_exactly_k_iterations(shape, fmt):
    d_, a_, q_, _ = SHAPES[shape]
    for n_cells in (1, 5, -(-257 // q_)):
        k, values, blocks, mask = assembled(shape, n_cells, 21 + n_cells, fmt)
        a = k.to_scipy(values)
        rng = np.random.default_rng(4)
        b = np.where(mask, 0.0, rng.normal(size=k.shape[0]))
        start = rng.normal(size=k.shape[0])
        for kind in KINDS:
            pc, oracle_pc = preconditioners(k, kind, mask, **({"coarsest_nodes": 4} if kind in CYCLES else {}))
            for its in (1, 2, 7):
                s = fc.BiCGStab(k, preconditioner=pc, rtol=0.0, maxiter=its)
                for x0 in (None, start):
                    what = f"{shape} {fmt} cells={n_cells} {kind} k={its} x0={'yes' if x0 is not None else 'no'}"
                    want = oracle_bicgstab(k.indptr, k.indices, blocks, b, x0=x0, preconditioner=oracle_pc, rtol=0.0, maxiter=its)
                    res, x = solve_guarded(s, values, b, x0)
                    assert_same_result(res, x, want, what)
                    if n_cells > 5:
                        assert want.status == "maxiter" and want.iterations == its, what
            if kind in CYCLES and n_cells > 5:
                assert len(pc.levels) >= 3
        if n_cells > 5 and d_ > 1:  # (with one dof per node the tangent is a scalar and the matrix symmetric)
            assert asymmetry(a) >= 0.1
    # without out: a new tensor, x0 untouched
    x0_dev = to_device(start, "cuda")
    res = s(values, to_device(b, "cuda"), x0=x0_dev)
    assert res.x.data_ptr() != x0_dev.data_ptr() and np.array_equal(to_host(x0_dev), start)
    assert_same_bits(to_host(res.x), want.x, f"{shape} {fmt}: without out")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. a cube with two segments: check_every, the statuses, what stays untouched behind a solve
# ---------------------------------------------------------------------------------------------------------------------------------
RUNS = ((("rtol", 0.0), ("maxiter", 11)), (("rtol", 1e-6),))


@pytest.fixture(scope="module")
def cube_system():
    """the tension-test matrix of a cube of 10^3 hexahedra (3993 dofs: two segments; levels 1331, 64, 8) with the non-associated
    tangent of bicgstab_util (b = 0.6, b_flow = 0 at 30 % of the points), its right-hand side and the oracle's solves"""
    mesh = FE.Cube(10, 10, 10)
    op, f = cube_operators(mesh)
    mask, top = tension_constraints(mesh)
    assert SEG < mesh.n_dofs <= 2 * SEG
    tangent = nonassociated_tangent(mesh.n_points)
    b = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mesh.n_dofs))
    out = {}
    for fmt in FORMATS:
        k = fc.TangentMatrix(f, format=fmt)
        k.set_constrained(mask)
        values = k(to_device(tangent, "cuda"))
        torch.cuda.synchronize()
        out[fmt] = (k, values, from_format(fmt, k.indptr, k.indices, to_host(values), 3))
    assert_same_bits(out["bsr"][2], out["csr"][2], "the two formats hold one matrix")
    k, values, blocks = out["bsr"]
    assert asymmetry(k.to_scipy(values)) >= 0.1
    oracle = {(kind, kw): oracle_bicgstab(k.indptr, k.indices, blocks, b, preconditioner=preconditioners(k, kind, mask, coarsest_nodes=32)[1] if kind in CYCLES else kind,
                                          **dict(kw)) for kind in KINDS for kw in RUNS}
    return mesh, mask, b, out, oracle


@pytest.mark.parametrize("kind", KINDS, ids=[str(kind) for kind in KINDS])
@pytest.mark.parametrize("fmt", FORMATS)
def test_check_every_changes_nothing(fmt, kind, cube_system):
    mesh, mask, b, systems, oracle = cube_system
    k, values, blocks = systems[fmt]
    pc = fc.MultilevelPreconditioner(k, cycle=kind, coarsest_nodes=32) if kind in CYCLES else kind
    for kw in RUNS:
        want = oracle[(kind, kw)]
        assert want.status == ("maxiter" if "maxiter" in dict(kw) else "converged") and want.iterations >= 11
        for every in (1, 3, 16):  # (11 iterations end in the middle of a batch of 3 and of 16; so does the converged solve's last)
            res, x = solve_guarded(fc.BiCGStab(k, preconditioner=pc, check_every=every, **dict(kw)), values, b)
            assert_same_result(res, x, want, f"{fmt} {kind} {dict(kw)} check_every={every}")
            assert res.looks == 1 + -(-want.iterations // every)


def test_statuses(cube_system):
    mesh, mask, b, systems, oracle = cube_system
    k, values, blocks = systems["bsr"]
    n = b.size
    start = np.random.default_rng(2).normal(size=n)
    for kind in KINDS:
        pc, oracle_pc = preconditioners(k, kind, mask, **({"coarsest_nodes": 32} if kind in CYCLES else {}))
        s = fc.BiCGStab(k, preconditioner=pc, rtol=1e-6)
        # b = 0: converged at once, no 0/0
        for x0 in (None, np.zeros(n)):
            res, x = solve_guarded(s, values, np.zeros(n), x0)
            assert (res.status, res.iterations, res.converged, res.residual_norm, res.rhs_norm) == ("converged", 0, True, 0.0, 0.0)
            assert res.looks == 1  # ended at the start: no iteration was enqueued
            assert (bits(x) == 0).all()
        # maxiter reached, and maxiter 0: x is x0
        res, x = solve_guarded(fc.BiCGStab(k, preconditioner=pc, rtol=1e-12, maxiter=5), values, b)
        assert (res.status, res.iterations, res.converged) == ("maxiter", 5, False) and np.isfinite(x).all() and res.residual_norm > 0
        assert_same_result(res, x, oracle_bicgstab(k.indptr, k.indices, blocks, b, preconditioner=oracle_pc, rtol=1e-12, maxiter=5), f"{kind}: maxiter")
        res, x = solve_guarded(fc.BiCGStab(k, preconditioner=pc, maxiter=0), values, b, start)
        assert (res.status, res.iterations, res.looks) == ("maxiter", 0, 1)
        assert_same_bits(x, start, f"{kind}: maxiter 0")
        # a NaN in b
        bad = b.copy()
        bad[17] = np.nan
        res, x = solve_guarded(s, values, bad)
        assert (res.status, res.iterations, res.looks) == ("nonfinite", 0, 1)
        # a zeroed diagonal block: no iteration, x is x0
        if kind is not None:
            broken = values.clone()
            broken.reshape(-1, 3, 3)[int(k.diag_block[mesh.n_nodes // 2])] = 0.0
            res, x = solve_guarded(s, broken, b, start)
            assert (res.status, res.iterations, res.converged, res.looks) == ("singular_block", 0, False, 1)
            assert_same_bits(x, start, f"{kind}: singular block")
        # and the object solves again afterwards
        res, x = solve_guarded(s, values, b)
        assert_same_result(res, x, oracle[(kind, RUNS[1])], f"{kind}: after the statuses")


@pytest.mark.parametrize("fmt", FORMATS)
def test_breakdown_and_the_half_step_exit(fmt, cube_system):
    mesh, mask, b, systems, oracle = cube_system
    k = systems[fmt][0]
    n = b.size
    # a skew-symmetric matrix of small integers, an integer b, no preconditioner: rhat . v = b^T K b is exactly zero
    skew = skew_blocks(k.indptr, k.indices, 3, 3)
    ints = np.random.default_rng(4).integers(-4, 5, size=n).astype(np.float64)
    start = np.random.default_rng(5).integers(-4, 5, size=n).astype(np.float64)
    values = to_device(to_format(fmt, k.indptr, k.indices, skew), "cuda")
    assert_same_bits(from_format(fmt, k.indptr, k.indices, to_host(values), 3), skew, "the skew-symmetric values")
    s = fc.BiCGStab(k, preconditioner=None)
    res, x = solve_guarded(s, values, ints)
    assert (res.status, res.iterations, res.converged, res.looks) == ("breakdown", 0, False, 2)
    assert (bits(x) == 0).all()
    assert_same_result(res, x, oracle_bicgstab(k.indptr, k.indices, skew, ints, preconditioner=None), f"{fmt}: breakdown")
    want = oracle_bicgstab(k.indptr, k.indices, skew, ints, x0=start, preconditioner=None, maxiter=3)
    res, x = solve_guarded(fc.BiCGStab(k, preconditioner=None, maxiter=3), values, ints, start)
    assert_same_result(res, x, want, f"{fmt}: the skew-symmetric matrix with a start vector")
    # the identity (every dof constrained): s = r - (rho / rv) v is zero, the solve ends at the half step of its first iteration
    every = fc.TangentMatrix(k.force, format=fmt)
    every.set_constrained(np.ones(n, dtype=bool))
    values = every(to_device(spd_tangent(mesh.n_points, 6, 1, False), "cuda"))
    blocks = from_format(fmt, every.indptr, every.indices, to_host(values), 3)
    rhs = np.random.default_rng(6).normal(size=n)
    for kind in (None, "block_jacobi"):
        want = oracle_bicgstab(every.indptr, every.indices, blocks, rhs, x0=start, preconditioner=kind)
        res, x = solve_guarded(fc.BiCGStab(every, preconditioner=kind), values, rhs, start)
        assert (want.status, want.iterations, want.residual_norm) == ("converged", 1, 0.0)
        assert_same_result(res, x, want, f"{fmt} {kind}: the half-step exit")
        assert res.looks == 2 and np.allclose(x, rhs, rtol=1e-14, atol=1e-14)  # x = x0 + 1.0 * (rhs - x0), rounded twice


def test_conjugate_gradients_and_apply_behind_a_solve(cube_system):
    """one preconditioner instance in BiCGStab, then in the conjugate gradients and standalone: their oracles' bits (the launch
    plans of the three source / destination pairs live side by side), on the symmetric matrix of the same pattern"""
    mesh, mask, b, systems, oracle = cube_system
    k = systems["bsr"][0]
    values = k(to_device(spd_tangent(mesh.n_points, 6, 1, False), "cuda"))
    blocks = from_format("bsr", k.indptr, k.indices, to_host(values), 3)
    for cycle in CYCLES:
        pc, oracle_pc = preconditioners(k, cycle, mask, coarsest_nodes=32)
        want = oracle_bicgstab(k.indptr, k.indices, blocks, b, preconditioner=oracle_pc, rtol=1e-6)
        s = fc.BiCGStab(k, preconditioner=pc, rtol=1e-6)
        res, x = solve_guarded(s, values, b)
        assert_same_result(res, x, want, f"{cycle}: BiCGStab on the symmetric matrix")
        assert len(pc._on[k.device].plans) == 2
        res, x = solve_guarded(fc.ConjugateGradient(k, preconditioner=pc, rtol=1e-6), values, b)
        assert_same_result(res, x, MU.conjugate_gradient(oracle_pc, blocks, b, rtol=1e-6), f"{cycle}: conjugate gradients behind BiCGStab")
        buf, out = guarded(b.size)
        pc.apply(values, to_device(b, "cuda"), out=out)
        torch.cuda.synchronize()
        assert_margins_intact(buf, b.size)
        assert_same_bits(to_host(out), oracle_pc.setup(blocks).apply(b), f"{cycle}: apply behind BiCGStab")
        assert len(pc._on[k.device].plans) == multilevel.PLANS
        res, x = solve_guarded(s, values, b)
        assert_same_result(res, x, want, f"{cycle}: BiCGStab again")
        assert len(pc._on[k.device].plans) == multilevel.PLANS
    for kind in ("block_jacobi", None):
        res, x = solve_guarded(fc.BiCGStab(k, preconditioner=kind, rtol=1e-6), values, b)
        assert_same_result(res, x, oracle_bicgstab(k.indptr, k.indices, blocks, b, preconditioner=kind, rtol=1e-6), f"{kind}: BiCGStab on the symmetric matrix")
        res, x = solve_guarded(fc.ConjugateGradient(k, preconditioner=kind, rtol=1e-6), values, b)
        assert_same_result(res, x, conjugate_gradient(k.indptr, k.indices, blocks, b, preconditioner=kind, rtol=1e-6), f"{kind}: conjugate gradients behind BiCGStab")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. one compute unit's blocks on 36 segments
# ---------------------------------------------------------------------------------------------------------------------------------
def test_on_one_compute_unit(one_cu):
    mesh = FE.Cube(32, 32, 32)
    op, f = cube_operators(mesh)
    assert -(-mesh.n_dofs // SEG) > 2 * gradient.BLOCKS_PER_CU
    k = fc.TangentMatrix(f, format="csr")
    mask, _ = tension_constraints(mesh)
    k.set_constrained(mask)
    values = k(to_device(nonassociated_tangent(mesh.n_points), "cuda"))
    torch.cuda.synchronize()
    blocks = from_format("csr", k.indptr, k.indices, to_host(values), 3)
    b = np.where(mask, 0.0, np.random.default_rng(3).normal(size=mesh.n_dofs))
    start = np.random.default_rng(4).normal(size=mesh.n_dofs)
    for kind, x0 in (("block_jacobi", start), (None, None)):
        del one_cu[:]
        res, x = solve_guarded(fc.BiCGStab(k, preconditioner=kind, rtol=0.0, maxiter=2, check_every=2), values, b, x0)
        assert_same_result(res, x, oracle_bicgstab(k.indptr, k.indices, blocks, b, x0=x0, preconditioner=kind, rtol=0.0, maxiter=2), f"cube 32 {kind}, one compute unit")
        names = {name for name, nb in one_cu if "fcamd_bcg" in name or "fcamd_cg" in name}
        assert names == set(ITERATING) | {bicgstab.START_KERNEL} | ({solver.INVERSE_KERNEL, solver.MATVEC_KERNEL} if kind else set())
        assert {nb for name, nb in one_cu if name in names} == {gradient.BLOCKS_PER_CU}  # every launch really was capped
        assert [name for name, _ in one_cu if name in ITERATING] == 2 * [bicgstab.PRODUCT_KERNEL, bicgstab.HALF_KERNEL, bicgstab.PRODUCT_KERNEL, bicgstab.FULL_KERNEL,
                                                                         bicgstab.DIRECTION_KERNEL]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. refusals come before any launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    k, values, blocks, mask = assembled("hex8", 21, 11, "bsr")
    n, nnz = k.shape[0], k.nnz
    solvers = [fc.BiCGStab(k), fc.BiCGStab(k, preconditioner="multilevel")]
    other = assembled("hex8", 21, 11, "csr")[0]  # the same pattern, another object
    lonely = fc.TangentMatrix(k.force)  # without the pattern's extra cells: the node no cell touches has no block
    b = to_device(np.where(mask, 0.0, 1.0), "cuda")
    for s in solvers:
        s(values, b)  # tables uploaded, kernels loaded: what follows can only add launches
    buf, out = guarded(n)
    spare = torch.zeros(2 * max(n, nnz) + 2, dtype=torch.float64, device="cuda")
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        for s in solvers:
            with pytest.raises(ValueError, match="aligned"):
                s(values, b, out=buf[MARGIN + 1: MARGIN + 1 + n])
            with pytest.raises(ValueError, match="entries"):
                s(values, b, out=buf[MARGIN: MARGIN + n - 3])
            with pytest.raises(ValueError, match="contiguous"):
                s(values, b, out=spare[: 2 * n: 2])
            with pytest.raises(ValueError, match="cuda"):
                s(values, b, out=torch.empty(n, dtype=torch.float64))
            with pytest.raises(TypeError):
                s(values, b, out=out.float())
            with pytest.raises(ValueError, match="alias"):
                s(values, b, out=b)
            with pytest.raises(ValueError, match="x0 itself"):
                s(values, b, x0=spare[2: 2 + n], out=spare[:n])
            with pytest.raises(ValueError, match="entries"):
                s(values[:-9], b, out=out)
            with pytest.raises(ValueError, match="entries"):
                s(values, b[:-3], out=out)
            with pytest.raises(ValueError, match="aligned"):
                s(values, spare[1: 1 + n], out=out)
            with pytest.raises(ValueError, match="contiguous"):
                s(values, b, x0=spare[: 2 * n: 2], out=out)
            with pytest.raises(TypeError):
                s(values, to_host(b), out=out)
            with pytest.raises(TypeError):
                s(values.float(), b, out=out)
            with pytest.raises(ValueError, match="cuda"):
                s(values, b.cpu(), out=out)
        with pytest.raises(ValueError, match="another matrix"):
            fc.BiCGStab(other, preconditioner=solvers[1].preconditioner)
        with pytest.raises(ValueError, match="preconditioner"):
            fc.BiCGStab(k, preconditioner="amg")
        with pytest.raises(ValueError, match="no diagonal block"):
            fc.BiCGStab(lonely)
    finally:
        jit.launch = real
    torch.cuda.synchronize()
    assert launches == []
    assert (bits(to_host(buf)) == CANARY).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the reason for the feature, on the device
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_unsymmetric_system_conjugate_gradients_do_not_solve(fmt):
    """test_bicgstab.py's system -- Cube(3, 2, 4), b = 0.6, b_flow = 0 at 30 % of the points -- assembled and solved on the device:
    the conjugate gradients do not end converged, BiCGStab converges on the oracle's bits"""
    mesh = FE.Cube(3, 2, 4)
    op, f = cube_operators(mesh)
    mask, _ = tension_constraints(mesh)
    k = fc.TangentMatrix(f, format=fmt)
    k.set_constrained(mask)
    values = k(to_device(nonassociated_tangent(mesh.n_points, b=0.6, b_flow=0.0, H=2000.0, frac=0.3, seed=5), "cuda"))
    torch.cuda.synchronize()
    blocks = from_format(fmt, k.indptr, k.indices, to_host(values), 3)
    a = k.to_scipy(values)
    rhs = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mesh.n_dofs))
    assert asymmetry(a) >= 0.1
    res, x = solve_guarded(fc.ConjugateGradient(k, maxiter=10 * mesh.n_dofs, check_every=256), values, rhs)
    assert not res.converged and res.status != "converged"
    want = oracle_bicgstab(k.indptr, k.indices, blocks, rhs)
    res, x = solve_guarded(fc.BiCGStab(k), values, rhs)
    assert_same_result(res, x, want, f"{fmt}: the unsymmetric system")
    assert res.converged and res.iterations <= 200
    assert np.linalg.norm(rhs - a @ x) <= 1e-7 * np.linalg.norm(rhs)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the Newton loop of the example
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def direct_run():
    """``fe_mini.tension_test`` of Cube(3, 2, 4) on the CPU with the oracle Drucker-Prager law and SciPy's direct solver"""
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    state = FE.CopyProtocolState(FE.OracleLaw(O.comfe_drucker_prager, DP_P, {"history": 7}), mesh.n_points)
    with np.errstate(all="ignore"):
        reactions, norms, _ = FE.tension_test(mesh, state, steps=8, top_displacement=TOP_DISPLACEMENT)
    return mesh, reactions, norms


@pytest.mark.parametrize("fmt", FORMATS)
def test_in_the_loop_of_the_example(fmt, direct_run):
    """examples/cube_tension_nonsymmetric.py on Cube(3, 2, 4): DruckerPrager3D with b = 0.15, b_flow = 0, eight load steps,
    BiCGStab(rtol=1e-12) with block-Jacobi and with the additive cycle: the direct solve's Newton counts, the largest relative
    reaction difference at most 1e-8, the bound the examples assert"""
    mesh, r_direct, norms_direct = direct_run
    scale = np.max(np.abs(r_direct))
    for pc, options in (("block_jacobi", {}), ("additive", {"coarsest_nodes": 8})):
        loop = nonsymmetric_loop(mesh, drucker_prager(), pc, format=fmt, rtol=1e-12, **options)
        r_gpu, norms_gpu, u, solves = tension_test_device_solve(mesh, loop, steps=8, top_displacement=TOP_DISPLACEMENT)  # (raises where a solve does not converge)
        a = loop.K.to_scipy(loop._values)
        difference = np.max(np.abs(r_gpu - r_direct)) / scale
        counts = [len(h) for h in norms_gpu]
        print(f"nonsymmetric tension test, {fmt} {pc}: GPU against direct {difference:.3e}, Newton iterations {counts}, BiCGStab iterations {solves}, "
              f"asymmetry of the last stiffness {asymmetry(a):.3f}")
        assert counts == [len(h) for h in norms_direct] == [2, 3, 3, 4, 6, 6, 6, 6]
        assert loop.assemblies == len(solves) == sum(counts) - 8
        assert asymmetry(a) >= 0.01
        assert difference <= 1e-8, difference
