"""The device BiCGStab without a GPU (fenics_constitutive_amd.bicgstab, csrc/jit/bicgstab.hip): every program compiles for gfx950
without scratch and with the LDS bicgstab.lds_bytes says, the host-side validation, and the ordered oracle (bicgstab_util.py): the
unsymmetric system the conjugate gradients do not solve, the symmetric one under every preconditioner, the statuses, and the
Newton loop of examples/cube_tension_nonsymmetric.py with a non-associated Drucker-Prager law against SciPy's direct solver."""

import os
import sys

import numpy as np
import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import bicgstab, gradient, jit, solver
from fenics_constitutive_amd.force import kernel_resources

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_constraints, tension_test_device_solve  # noqa: E402
from cube_tension_nonsymmetric import DP_P, TOP_DISPLACEMENT  # noqa: E402
from bicgstab_util import asymmetry, elastic_mandel, nonassociated_tangent, oracle_solve_loop, skew_blocks  # noqa: E402
from bicgstab_util import bicgstab as oracle_bicgstab  # noqa: E402
from force_util import random_inputs  # noqa: E402
from gradient_util import cube_operator_tables  # noqa: E402
from matrix_util import matrix_oracle, to_bsr  # noqa: E402
import multilevel_util as MU  # noqa: E402
from solver_util import conjugate_gradient, full_pattern, matvec, ordered_dot  # noqa: E402

KINDS = (None, "block_jacobi", "multilevel")


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. compilation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=["plain", "block_jacobi", "multilevel"])
@pytest.mark.parametrize("gdim", [1, 2, 3])
def test_every_program_compiles_without_scratch(gdim, kind):
    code = bicgstab.compile_kernels(gdim, kind)
    assert f"FCAMD_CG_PRECOND {KINDS.index(kind)}" in bicgstab.program(gdim, kind) and bicgstab.compile_kernels(gdim, KINDS.index(kind)) is code
    for kernel in bicgstab.KERNELS + bicgstab.SHARED_KERNELS:
        r = kernel_resources(code.log, kernel)
        assert r["scratch_bytes"] == 0, (kernel, r)
        assert r["lds_bytes"] == bicgstab.lds_bytes(kernel, kind) <= 64 * 1024, (kernel, r)
    # the product keeps the conjugate-gradient product's LDS: its two trees share one array
    assert bicgstab.lds_bytes(bicgstab.PRODUCT_KERNEL, kind) == solver.lds_bytes(solver.MATVEC_KERNEL)
    assert bicgstab.lds_bytes(bicgstab.HALF_KERNEL, kind) == 8 * (256 + 2) + (8 * solver.SEG if kind == "block_jacobi" else 0)
    before = jit.compile_count()
    assert bicgstab.compile_kernels(gdim, kind) is code and jit.compile_count() == before  # once per program text
    with pytest.raises(ValueError, match="LDS"):
        bicgstab.compile_kernels(gdim, kind, slab=2048)
    with pytest.raises(ValueError, match="multiple"):
        bicgstab.compile_kernels(gdim, kind, slab=1000)
    with pytest.raises(ValueError, match="preconditioner"):
        bicgstab.compile_kernels(gdim, "ilu")
    assert jit.compile_count() == before


def operators(shape="tet_p2", n_cells=5, seed=3, with_lonely=False, **kwargs):
    t = random_inputs(shape, n_cells, seed, False, True)
    f = fc.InternalForce(fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"]), t["weights"])
    if not with_lonely:
        kwargs["pattern_dofmap"] = full_pattern(t["dofmap"], t["n_nodes"])[0]
    return fc.TangentMatrix(f, **kwargs), t


def test_object_reports_what_the_compiler_made():
    k, _ = operators()
    for kind in KINDS:
        s = fc.BiCGStab(k, preconditioner=kind)
        r = s.resources
        assert r["scratch_bytes"] == 0 and r["lds_bytes"] == bicgstab.lds_bytes(bicgstab.PRODUCT_KERNEL) == s.lds_bytes() and r["slab"] == solver.SLAB
        assert all(r[name]["scratch_bytes"] == 0 for name in ("start", "half", "full", "direction", "matvec", "inverse"))
        assert r["half"]["lds_bytes"] == s.lds_bytes(bicgstab.HALF_KERNEL) == bicgstab.lds_bytes(bicgstab.HALF_KERNEL, kind)
        assert all(kernel in s.compile_log for kernel in bicgstab.KERNELS) and s.device == k.device
        assert s.maxiter == 10 * k.shape[0]
    assert "BiCGStab" in fc.__all__ and bicgstab.STATUSES[-1] == "breakdown" and bicgstab.STATUSES[:-1] == solver.STATUSES
    assert isinstance(fc.BiCGStab(k, preconditioner="multilevel").preconditioner, fc.MultilevelPreconditioner)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. validation comes before any upload or launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_validation_errors():
    torch = pytest.importorskip("torch")
    k, t = operators()
    lonely_k, _ = operators(with_lonely=True)
    other, _ = operators(seed=4)
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        S = fc.BiCGStab
        with pytest.raises(TypeError):
            S(k.force)  # not a TangentMatrix
        with pytest.raises(ValueError, match=f"node {int(full_pattern(t['dofmap'], t['n_nodes'])[1][0])} "):
            S(lonely_k)
        with pytest.raises(ValueError, match="preconditioner"):
            S(k, preconditioner="ilu")
        with pytest.raises(ValueError, match="another matrix"):
            S(k, preconditioner=fc.MultilevelPreconditioner(other))
        with pytest.raises(ValueError, match="rtol"):
            S(k, rtol=-1.0)
        with pytest.raises(TypeError):
            S(k, atol="0")
        with pytest.raises(TypeError):
            S(k, maxiter=1e3)
        with pytest.raises(ValueError, match="check_every"):
            S(k, check_every=0)
        s = S(k, preconditioner=None, maxiter=7, check_every=3)
        assert (s.preconditioner, s.maxiter, s.check_every, s.rtol, s.atol) == (None, 7, 3, 1e-8, 0.0)
        n, nnz = k.shape[0], k.nnz
        host = lambda m: torch.zeros(m, dtype=torch.float64)  # noqa: E731
        for solve in (s, S(k), S(k, preconditioner="multilevel")):
            with pytest.raises(TypeError):
                solve(np.zeros(nnz), host(n))  # an ndarray
            with pytest.raises(TypeError):
                solve(host(nnz).float(), host(n))
            with pytest.raises(ValueError, match="cuda"):
                solve(host(nnz), host(n))  # on the host
            assert not solve._work and (solve._ml is None or not solve._ml._on)
    finally:
        jit.launch = real
    assert not launches
    assert not k._on and not s._op._on  # nothing was uploaded


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the reason for the feature
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cube():
    mesh = FE.Cube(3, 2, 4)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    weights = gradient.integration_weights(mesh.nodes[mesh.cells], ref, np.ones(8))
    mask, _ = tension_constraints(mesh)
    rhs = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mesh.n_dofs))

    def system(tangent):
        return matrix_oracle(tangent, dofmap, ref, jinv, weights, mesh.n_nodes, constrained=mask)

    return mesh, (dofmap, ref, jinv, weights), mask, rhs, system


def test_the_unsymmetric_system_conjugate_gradients_do_not_solve(cube):
    """Cube(3, 2, 4), the tension constraints, the non-associated tangent (b = 0.6, b_flow = 0, H = 2000) at a seeded 30 % of the
    points.  Measured with the ordered oracle: asymmetry 0.183; conjugate gradients: ``maxiter`` at 1800, true residual 0.85 |b|;
    BiCGStab with block-Jacobi: 47 iterations, true residual 2.95e-9 |b|, 4.1e-9 from the direct solve (plain: 77 iterations)."""
    import scipy.sparse.linalg as spla

    mesh, _, mask, rhs, system = cube
    indptr, indices, blocks = system(nonassociated_tangent(mesh.n_points, b=0.6, b_flow=0.0, H=2000.0, frac=0.3, seed=5))
    a = to_bsr(indptr, indices, blocks, mesh.n_nodes).tocsr()
    n = rhs.size
    asym = asymmetry(a)
    cg = conjugate_gradient(indptr, indices, blocks, rhs, preconditioner="block_jacobi", maxiter=10 * n)
    res = oracle_bicgstab(indptr, indices, blocks, rhs, preconditioner="block_jacobi")
    want = spla.spsolve(a.tocsc(), rhs)
    true = np.linalg.norm(rhs - a @ res.x) / np.linalg.norm(rhs)
    error = np.linalg.norm(res.x - want) / np.linalg.norm(want)
    print(f"asymmetry {asym:.3f}; conjugate gradients: {cg.status} after {cg.iterations}, true residual {np.linalg.norm(rhs - a @ cg.x) / np.linalg.norm(rhs):.2e} |b|; "
          f"BiCGStab: {res.status} after {res.iterations}, true residual {true:.2e} |b|, {error:.2e} from the direct solve")
    assert asym >= 0.1
    assert not cg.converged and cg.status != "converged"
    assert res.converged and res.status == "converged" and res.iterations <= 200
    assert res.residual_norm <= 1e-8 * res.rhs_norm
    assert true <= 1e-7
    assert error <= 1e-6


def test_the_symmetric_system_under_every_preconditioner(cube):
    import scipy.sparse.linalg as spla

    mesh, _, mask, rhs, system = cube
    indptr, indices, blocks = system(np.tile(elastic_mandel().reshape(-1), mesh.n_points))
    a = to_bsr(indptr, indices, blocks, mesh.n_nodes).tocsr()
    assert asymmetry(a) <= 1e-15
    want = spla.spsolve(a.tocsc(), rhs)
    counts = {}
    for name, pc in (("plain", None), ("block_jacobi", "block_jacobi"),
                     ("multiplicative", MU.Oracle(indptr, indices, cycle="multiplicative", coarsest_nodes=8, mask=mask)),
                     ("additive", MU.Oracle(indptr, indices, cycle="additive", coarsest_nodes=8, mask=mask))):
        res = oracle_bicgstab(indptr, indices, blocks, rhs, preconditioner=pc)
        assert res.converged and res.residual_norm <= 1e-8 * res.rhs_norm, name
        assert np.linalg.norm(res.x - want) <= 1e-6 * np.linalg.norm(want), name
        counts[name] = res.iterations
    print(f"BiCGStab iterations on the elastic Cube(3, 2, 4): {counts}")
    assert counts["block_jacobi"] < counts["plain"] and counts["multiplicative"] < counts["block_jacobi"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the statuses of the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def test_statuses_of_the_oracle(cube):
    mesh, _, mask, rhs, system = cube
    indptr, indices, blocks = system(nonassociated_tangent(mesh.n_points))
    n = rhs.size
    x0 = np.random.default_rng(1).normal(size=n)
    solved = oracle_bicgstab(indptr, indices, blocks, rhs)
    for pc in ("block_jacobi", None, MU.Oracle(indptr, indices, coarsest_nodes=8, mask=mask)):
        zero = oracle_bicgstab(indptr, indices, blocks, np.zeros(n), preconditioner=pc)
        assert zero.status == "converged" and zero.iterations == 0 and (zero.x.view(np.uint64) == 0).all() and zero.residual_norm == 0.0
        short = oracle_bicgstab(indptr, indices, blocks, rhs, preconditioner=pc, rtol=1e-12, maxiter=5)
        assert short.status == "maxiter" and short.iterations == 5 and not short.converged and np.isfinite(short.x).all()
        none = oracle_bicgstab(indptr, indices, blocks, rhs, x0=x0, preconditioner=pc, maxiter=0)
        assert none.status == "maxiter" and none.iterations == 0 and np.array_equal(none.x, x0)
        warm = oracle_bicgstab(indptr, indices, blocks, rhs, x0=solved.x, preconditioner=pc, rtol=1e-7)
        assert warm.status == "converged" and warm.iterations == 0 and np.array_equal(warm.x, solved.x)
        bad = rhs.copy()
        bad[5] = np.nan
        assert oracle_bicgstab(indptr, indices, blocks, bad, preconditioner=pc).status == "nonfinite"
    broken = blocks.copy()
    node = 7
    broken[np.flatnonzero((np.repeat(np.arange(indptr.size - 1), np.diff(indptr)) == node) & (indices == node))[0]] = 0.0
    for pc in ("block_jacobi", MU.Oracle(indptr, indices, coarsest_nodes=8, mask=mask)):
        sing = oracle_bicgstab(indptr, indices, broken, rhs, x0=x0, preconditioner=pc)
        assert sing.status == "singular_block" and sing.iterations == 0 and np.array_equal(sing.x, x0)
    # a skew-symmetric matrix of small integers and an integer right-hand side: rhat . v = b^T K b is exactly zero in every
    # summation order, so the first iteration ends in breakdown with nothing written
    skew = skew_blocks(indptr, indices, 3, 3)
    b = np.random.default_rng(4).integers(-4, 5, size=n).astype(np.float64)
    v = matvec(indptr, indices, skew, b)
    assert np.abs(v).max() > 0 and ordered_dot(v, b) == 0.0 and np.array_equal(to_bsr(indptr, indices, skew, mesh.n_nodes).toarray(), -to_bsr(indptr, indices, skew, mesh.n_nodes).toarray().T)
    res = oracle_bicgstab(indptr, indices, skew, b, preconditioner=None)
    assert (res.status, res.iterations, res.converged) == ("breakdown", 0, False) and (res.x.view(np.uint64) == 0).all()
    assert res.residual_norm == res.rhs_norm == float(np.sqrt(ordered_dot(b, b)))
    # the half-step exit: on the identity s = r - (rho / rv) v is zero
    eye_ptr, eye_idx, eye = np.arange(n // 3 + 1), np.arange(n // 3), np.tile(np.eye(3), (n // 3, 1, 1))
    for pc in ("block_jacobi", None):
        res = oracle_bicgstab(eye_ptr, eye_idx, eye, rhs, preconditioner=pc)
        assert (res.status, res.iterations, res.residual_norm) == ("converged", 1, 0.0) and np.array_equal(res.x, rhs)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the Newton loop with a non-associated Drucker-Prager law
# ---------------------------------------------------------------------------------------------------------------------------------
def test_oracle_newton_loop_with_a_nonassociated_law(cube):
    """examples/cube_tension_nonsymmetric.py on the CPU: Cube(3, 2, 4), Drucker-Prager with a = 600, b = 0.15, b_flow = 0 (chosen on
    the CPU: the oracle law refuses an iterate at the surface's tip I_1 = a / b = 4000, which this load path does not reach, and
    most of the cube yields), the top pulled by 0.005 in eight load steps, the oracle BiCGStab with rtol = 1e-12 against SciPy's direct solver.
    Measured: Newton counts (2, 3, 3, 4, 6, 6, 6, 6), 50 to 72 BiCGStab iterations per solve, 83 % of the points plastic at the end,
    the largest asymmetry of an assembled matrix 0.179, the largest relative reaction difference 6.3e-13."""
    from oracle import numpy_oracle as O

    mesh, (dofmap, ref, jinv, weights), mask, _, _ = cube

    def state():
        return FE.CopyProtocolState(FE.OracleLaw(O.comfe_drucker_prager, DP_P, {"history": 7}), mesh.n_points)

    with np.errstate(all="ignore"):  # (the oracle law evaluates its yield function's derivatives at the stress-free points too)
        direct_state = state()
        r_direct, norms_direct, _ = FE.tension_test(mesh, direct_state, steps=8, top_displacement=TOP_DISPLACEMENT)
        loop = oracle_solve_loop(state(), dofmap, ref, jinv, weights, mesh.n_nodes, rtol=1e-12)
        reactions, norms, u, solves = tension_test_device_solve(mesh, loop, steps=8, top_displacement=TOP_DISPLACEMENT)
    plastic = float((np.abs(direct_state.hist_c["history"].reshape(-1, 7)[:, 1:]).max(axis=1) > 0).mean())
    asym = max(asymmetry(to_bsr(indptr, indices, blocks, mesh.n_nodes).tocsr()) for indptr, indices, blocks, _, _ in loop.systems)
    counts = [len(h) for h in norms]
    difference = np.max(np.abs(reactions - r_direct)) / np.max(np.abs(r_direct))
    print(f"oracle loop, Drucker-Prager {DP_P}: Newton iterations {counts}, BiCGStab iterations {min(solves)} .. {max(solves)}, plastic points {plastic:.2f}, "
          f"largest asymmetry {asym:.3f}, largest relative reaction difference to the direct solve {difference:.2e}")
    assert plastic >= 0.1 and asym >= 0.01
    assert counts == [len(h) for h in norms_direct]
    assert len(loop.systems) == len(solves) == sum(counts) - 8 and all(result.converged for *_, result in loop.systems)
    assert difference <= 1e-8
