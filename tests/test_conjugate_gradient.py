"""The device solver without a GPU (fenics_constitutive_amd.solver, csrc/jit/conjugate_gradient.hip): every program compiles for
gfx950 without scratch and with the LDS solver.lds_bytes says, the ordered dot of the oracle (solver_util.py) against math.fsum, the
oracle conjugate gradients in the Newton loop of examples/cube_tension_device_solve.py against SciPy's direct solver, the statuses
of the oracle, and the host-side validation."""

import math
import os
import sys

import numpy as np
import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import gradient, jit, solver
from fenics_constitutive_amd.force import kernel_resources

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_test_device_solve  # noqa: E402
from force_util import random_inputs  # noqa: E402
from gradient_util import SHAPES, cube_operator_tables  # noqa: E402
from matrix_util import matrix_oracle, to_bsr  # noqa: E402
from solver_util import (SEG, block_inverses, full_pattern, conjugate_gradient, dot_bound, matvec, oracle_solve_loop, ordered_dot)  # noqa: E402

VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}


def operators(shape="tet_p2", n_cells=5, seed=3, with_lonely=False, **kwargs):
    """(TangentMatrix, tables): the pattern of the random tables, the node no cell touches given a block of its own unless asked"""
    t = random_inputs(shape, n_cells, seed, False, True)
    f = fc.InternalForce(fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"]), t["weights"])
    if not with_lonely:
        kwargs["pattern_dofmap"] = full_pattern(t["dofmap"], t["n_nodes"])[0]
    return fc.TangentMatrix(f, **kwargs), t


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. compilation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preconditioned", [True, False], ids=["block_jacobi", "plain"])
@pytest.mark.parametrize("gdim", [1, 2, 3])
def test_every_program_compiles_without_scratch(gdim, preconditioned):
    code = solver.compile_kernels(gdim, preconditioned)
    for kernel in solver.KERNELS:
        r = kernel_resources(code.log, kernel)
        assert r["scratch_bytes"] == 0, (kernel, r)
        assert r["lds_bytes"] == solver.lds_bytes(kernel, preconditioned) <= 64 * 1024, (kernel, r)
    assert solver.lds_bytes(solver.MATVEC_KERNEL) == 8 * (4 * solver.SLAB + 258) and solver.SEG == SEG == 3072
    before = jit.compile_count()
    assert solver.compile_kernels(gdim, preconditioned) is code and jit.compile_count() == before  # once per program text
    with pytest.raises(ValueError, match="LDS"):
        solver.compile_kernels(gdim, preconditioned, slab=2048)
    with pytest.raises(ValueError, match="multiple"):
        solver.compile_kernels(gdim, preconditioned, slab=1000)
    assert jit.compile_count() == before


def test_object_reports_what_the_compiler_made():
    k, _ = operators()
    cg = fc.ConjugateGradient(k)
    r = cg.resources
    assert r["scratch_bytes"] == 0 and r["lds_bytes"] == solver.lds_bytes(solver.MATVEC_KERNEL) and r["slab"] == solver.SLAB
    assert all(r[name]["scratch_bytes"] == 0 for name in ("update", "direction", "inverse", "dot"))
    assert all(kernel in cg.compile_log for kernel in solver.KERNELS) and cg.device == k.device
    assert cg.maxiter == 10 * k.shape[0] and "ConjugateGradient" in fc.__all__


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the ordered dot of the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, SEG - 1, SEG, SEG + 1, 2 * SEG + 5, 256 * SEG + 1])
def test_ordered_dot_against_fsum(n):
    rng = np.random.default_rng(n)
    a, b = rng.normal(size=n), rng.normal(size=n) * np.exp(rng.normal(size=n))
    have, want = ordered_dot(a, b), math.fsum(a * b)
    bound = dot_bound(a, b)
    assert abs(have - want) <= bound, (have, want, bound)
    ints = rng.integers(-8, 9, size=n).astype(np.float64)
    assert ordered_dot(ints, ints) == float((ints.astype(np.int64) ** 2).sum())  # exact on integers


def test_ordered_dot_is_invariant_under_zero_padding():
    rng = np.random.default_rng(5)
    for n in (1, 300, SEG - 1, SEG + 1):
        a, b = rng.normal(size=n), rng.normal(size=n)
        want = ordered_dot(a, b)
        for extra in (1, 255, SEG - n % SEG if n % SEG else 0):  # (within the last segment: the segments stay the same)
            if (n + extra - 1) // SEG == (n - 1) // SEG:
                z = np.zeros(extra)
                assert ordered_dot(np.concatenate([a, z]), np.concatenate([b, z])) == want
        # whole segments of zeros: the partials get +0.0 more
        z = np.zeros(3 * SEG)
        assert ordered_dot(np.concatenate([a, z]), np.concatenate([b, z])) == want


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the oracle's product, inverses and solve
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["hex8", "tet_p2", "tri_p2", "interval"])
def test_oracle_product_and_inverses(shape):
    d_, a_, q_, affine = SHAPES[shape]
    t = random_inputs(shape, 9, 11, False, affine)
    indptr, indices, blocks = matrix_oracle(t["tangent"], t["dofmap"], t["ref"], t["jinv"], t["weights"], t["n_nodes"])
    p = np.random.default_rng(2).normal(size=d_ * t["n_nodes"])
    have, want = matvec(indptr, indices, blocks, p), to_bsr(indptr, indices, blocks, t["n_nodes"]) @ p
    bound = (d_ * int(np.diff(indptr).max()) + 2) * 2.0**-52 * (to_bsr(indptr, indices, np.abs(blocks), t["n_nodes"]) @ np.abs(p))
    assert (np.abs(have - want) <= bound).all() and np.abs(want).max() > 0
    assert (have.reshape(-1, d_)[t["lonely"]].view(np.uint64) == 0).all()  # the empty row: +0.0
    some = np.random.default_rng(3).normal(size=(50, d_, d_)) + 3.0 * np.eye(d_)
    inv, det = block_inverses(some)
    assert np.allclose(inv, np.linalg.inv(some), rtol=1e-11, atol=0) and np.allclose(det, np.linalg.det(some), rtol=1e-12, atol=0)


@pytest.fixture(scope="module")
def oracle_loops():
    """the Newton loop of the example on the CPU with the oracle law, matrix and conjugate gradients, preconditioned and plain"""
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    weights = gradient.integration_weights(mesh.nodes[mesh.cells], ref, np.ones(8))

    def cpu_state():
        return FE.CopyProtocolState(FE.OracleLaw(O.von_mises_3d, VM_P, {"eps_n": 6, "alpha": 1}), mesh.n_points)

    direct = FE.tension_test(mesh, cpu_state(), steps=8)
    loop = oracle_solve_loop(cpu_state(), dofmap, ref, jinv, weights, mesh.n_nodes, rtol=1e-12)
    run = tension_test_device_solve(mesh, loop, steps=8)
    return mesh, direct, loop, run


def test_oracle_solves_of_the_cube_reproduce_the_direct_solver(oracle_loops):
    import scipy.sparse.linalg as spla

    mesh, direct, loop, (reactions, norms, u, solves) = oracle_loops
    counts = [len(h) for h in norms]
    difference = np.max(np.abs(reactions - direct[0])) / np.max(np.abs(direct[0]))
    print(f"oracle loop: Newton iterations {counts}, conjugate-gradient iterations {min(solves)} .. {max(solves)} {solves}, "
          f"largest relative reaction difference to the direct solve {difference:.2e}")
    assert counts == [len(h) for h in direct[1]] == [2, 2, 2, 3, 3, 4, 5, 5]
    assert len(loop.systems) == len(solves) == sum(counts) - 8
    fewer = []
    for indptr, indices, blocks, rhs, result in loop.systems:
        want = spla.spsolve(to_bsr(indptr, indices, blocks, mesh.n_nodes).tocsc(), rhs)
        assert result.converged and result.status == "converged"
        assert np.linalg.norm(result.x - want) <= 1e-6 * np.linalg.norm(want)
        assert result.residual_norm <= 1e-12 * result.rhs_norm and result.rhs_norm == math.sqrt(ordered_dot(rhs, rhs))
        plain = conjugate_gradient(indptr, indices, blocks, rhs, preconditioner=None, rtol=1e-12)
        assert plain.converged and np.linalg.norm(plain.x - want) <= 1e-6 * np.linalg.norm(want)
        fewer.append((result.iterations, plain.iterations))
    assert all(jacobi < plain for jacobi, plain in fewer), fewer
    assert difference <= 1e-8


def test_statuses_of_the_oracle(oracle_loops):
    mesh, _, loop, _ = oracle_loops
    indptr, indices, blocks, rhs, result = loop.systems[0]
    n = rhs.size
    x0 = np.random.default_rng(1).normal(size=n)
    for pc in ("block_jacobi", None):
        neg = conjugate_gradient(indptr, indices, -blocks, rhs, x0=x0, preconditioner=pc)
        assert neg.status == "indefinite" and neg.iterations == 0 and not neg.converged and np.array_equal(neg.x, x0)
        zero = conjugate_gradient(indptr, indices, blocks, np.zeros(n), preconditioner=pc)
        assert zero.status == "converged" and zero.iterations == 0 and (zero.x.view(np.uint64) == 0).all() and zero.residual_norm == 0.0
        short = conjugate_gradient(indptr, indices, blocks, rhs, preconditioner=pc, rtol=1e-12, maxiter=5)
        assert short.status == "maxiter" and short.iterations == 5 and not short.converged and np.isfinite(short.x).all()
        none = conjugate_gradient(indptr, indices, blocks, rhs, preconditioner=pc, rtol=1e-12, maxiter=0)
        assert none.status == "maxiter" and none.iterations == 0
        warm = conjugate_gradient(indptr, indices, blocks, rhs, x0=result.x, preconditioner=pc, rtol=1e-10)
        assert warm.status == "converged" and warm.iterations == 0 and np.array_equal(warm.x, result.x)
    broken = blocks.copy()
    node = 7
    broken[np.flatnonzero((np.repeat(np.arange(indptr.size - 1), np.diff(indptr)) == node) & (indices == node))[0]] = 0.0
    sing = conjugate_gradient(indptr, indices, broken, rhs, x0=x0)
    assert sing.status == "singular_block" and sing.iterations == 0 and np.array_equal(sing.x, x0)
    assert conjugate_gradient(indptr, indices, broken, rhs, preconditioner=None, maxiter=3).status == "maxiter"  # (no inverse: no such status)
    bad = rhs.copy()
    bad[5] = np.nan
    assert conjugate_gradient(indptr, indices, blocks, bad).status == "nonfinite"


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. validation comes before any upload or launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_validation_errors():
    torch = pytest.importorskip("torch")
    k, t = operators()
    lonely_k, _ = operators(with_lonely=True)
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        CG = fc.ConjugateGradient
        with pytest.raises(TypeError):
            CG(k.force)  # not a TangentMatrix
        with pytest.raises(ValueError, match=f"node {int(full_pattern(t['dofmap'], t['n_nodes'])[1][0])} "):
            CG(lonely_k)
        with pytest.raises(ValueError, match="preconditioner"):
            CG(k, preconditioner="ilu")
        with pytest.raises(ValueError, match="rtol"):
            CG(k, rtol=-1.0)
        with pytest.raises(TypeError):
            CG(k, atol="0")
        with pytest.raises(TypeError):
            CG(k, maxiter=1e3)
        with pytest.raises(ValueError, match="check_every"):
            CG(k, check_every=0)
        cg = CG(k, preconditioner=None, maxiter=7, check_every=3)
        assert (cg.preconditioner, cg.maxiter, cg.check_every, cg.rtol, cg.atol) == (None, 7, 3, 1e-8, 0.0)
        n, nnz = k.shape[0], k.nnz
        host = lambda m: torch.zeros(m, dtype=torch.float64)  # noqa: E731
        with pytest.raises(TypeError):
            cg(np.zeros(nnz), host(n))  # an ndarray
        with pytest.raises(TypeError):
            cg(host(nnz).float(), host(n))
        with pytest.raises(ValueError, match="cuda"):
            cg(host(nnz), host(n))  # on the host
        with pytest.raises(TypeError):
            solver.matvec(k.force, host(nnz), host(n))
        with pytest.raises(TypeError):
            solver.matvec(k, np.zeros(nnz), host(n))
        with pytest.raises(ValueError, match="cuda"):
            solver.matvec(k, host(nnz), host(n))
        with pytest.raises(TypeError):
            solver.dot(np.zeros(3), np.zeros(3))
        with pytest.raises(TypeError):
            solver.dot(host(3).float(), host(3))
        with pytest.raises(ValueError, match="GPU"):
            solver.dot(host(3), host(3))
    finally:
        jit.launch = real
    assert not launches
    assert not k._on and not cg._work and not cg._op._on and not solver._dot_control  # nothing was uploaded
