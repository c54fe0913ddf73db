"""The multilevel preconditioner without a GPU (fenics_constitutive_amd.multilevel, csrc/jit/multilevel.hip): the programs compile
for gfx950 without scratch and with the LDS the module states; the aggregation tables against the node-by-node oracle of
multilevel_util.py and against their defining properties; the oracle's Galerkin values against SciPy's triple product; both oracle
cycles symmetric, positive and exactly zero at the constrained dofs; the oracle conjugate gradients against SciPy's direct solver;
the iteration counts on the elastic cube of 12^3 cells; and the host-side validation."""

import math
import os
import sys

import numpy as np
import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import gradient, jit, multilevel, solver
from fenics_constitutive_amd.force import kernel_resources
from fenics_constitutive_amd.matrix import block_pattern

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_constraints  # noqa: E402
from force_util import random_inputs  # noqa: E402
from gradient_util import SHAPES, cube_operator_tables  # noqa: E402
from matrix_util import matrix_oracle, to_bsr  # noqa: E402
import multilevel_util as MU  # noqa: E402
from solver_util import conjugate_gradient, full_pattern  # noqa: E402

CYCLES = ("multiplicative", "additive")


def elastic_tangent(e_modulus=210000.0, nu=0.3):
    lam, mu = e_modulus * nu / ((1 + nu) * (1 - 2 * nu)), e_modulus / (2 * (1 + nu))
    c = 2 * mu * np.eye(6)
    c[:3, :3] += lam
    return c


def cube_matrix(mesh):
    """(TangentMatrix, indptr, indices, blocks, mask): the elastic cube with the tension test's constraints, on the CPU"""
    dofmap, ref, jinv = cube_operator_tables(mesh)
    weights = gradient.integration_weights(mesh.nodes[mesh.cells], ref, np.ones(8))
    mask, _ = tension_constraints(mesh)
    tangent = np.tile(elastic_tangent().reshape(-1), mesh.n_points)
    indptr, indices, blocks = matrix_oracle(tangent, dofmap, ref, jinv, weights, mesh.n_nodes, constrained=mask)
    k = fc.TangentMatrix(fc.InternalForce(fc.DisplacementGradient(dofmap, ref, jinv, mesh.n_nodes), weights))
    k.set_constrained(mask)
    return k, indptr, indices, blocks, mask


@pytest.fixture(scope="module")
def small_cube():
    return cube_matrix(FE.Cube(3, 2, 4))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. compilation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gdim", [1, 2, 3])
def test_every_program_compiles_without_scratch(gdim):
    code = multilevel.compile_kernels(gdim)
    for kernel in solver.KERNELS + multilevel.KERNELS:
        r = kernel_resources(code.log, kernel)
        assert r["scratch_bytes"] == 0, (kernel, r)
        assert r["lds_bytes"] == multilevel.lds_bytes(kernel) <= 64 * 1024, (kernel, r)
    assert multilevel.lds_bytes(multilevel.CLOSE_KERNEL) == 8 * 258 and multilevel.lds_bytes(multilevel.SMOOTH_KERNEL) == 0
    before = jit.compile_count()
    assert multilevel.compile_kernels(gdim) is code and jit.compile_count() == before
    # the solver's own programs are other programs and still compile as they did
    assert solver.compile_kernels(gdim, True) is not code and solver.compile_kernels(gdim, False) is not code
    with pytest.raises(ValueError, match="dofs per node"):
        multilevel.compile_kernels(4)


def test_object_reports_what_the_compiler_made(small_cube):
    k = small_cube[0]
    pc = fc.MultilevelPreconditioner(k, coarsest_nodes=8)
    assert set(pc.resources) == {"galerkin", "restrict", "prolong", "smooth", "close"}
    assert all(r["scratch_bytes"] == 0 for r in pc.resources.values()) and pc.resources["close"]["lds_bytes"] == pc.lds_bytes()
    assert all(kernel in pc.compile_log for kernel in multilevel.KERNELS + solver.KERNELS) and pc.device == k.device
    assert "MultilevelPreconditioner" in fc.__all__
    assert len(pc.levels) == 2 and pc.levels[0] == {"nodes": 60, "blocks": k.nnzb} and pc.levels[1]["nodes"] <= 8
    cg = fc.ConjugateGradient(k, preconditioner="multilevel")
    assert isinstance(cg.preconditioner, fc.MultilevelPreconditioner) and cg.preconditioner.cycle == "multiplicative"
    assert (cg.preconditioner.smoothing, cg.preconditioner.omega, cg.preconditioner.coarsest_nodes, cg.preconditioner.coarsest_sweeps,
            cg.preconditioner.max_levels) == (1, 0.5, 64, 8, 10)
    assert fc.ConjugateGradient(k, preconditioner=pc).preconditioner is pc


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. aggregation
# ---------------------------------------------------------------------------------------------------------------------------------
def check_level(indptr, indices, agg, roots, mem, folds, coarse):
    n = indptr.size - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    nb = [set(indices[indptr[v]: indptr[v + 1]].tolist()) | {v} for v in range(n)]
    n_agg = roots.size
    # every node in exactly one aggregate; aggregates numbered without gaps
    assert agg.shape == (n,) and agg.min() >= 0 and np.array_equal(np.unique(agg), np.arange(n_agg))
    mem_ptr, members = mem
    assert np.array_equal(np.sort(members), np.arange(n)) and mem_ptr[0] == 0 and mem_ptr[-1] == n
    singletons = 0
    for a in range(n_agg):
        mine = members[mem_ptr[a]: mem_ptr[a + 1]]
        assert (np.diff(mine) > 0).all() and (agg[mine] == a).all() and agg[roots[a]] == a
        # the aggregate within its root's neighbourhood: the root's neighbourhood itself (pass 1), and whoever joined in pass 2 is a
        # neighbour of one of those (a free node is never a neighbour of a root: pass 1 would have taken it)
        core = nb[roots[a]]
        inside = [int(i) for i in mine if int(i) in core]
        assert all(any(u in core for u in nb[int(i)]) for i in mine), a
        if nb[roots[a]] == {int(roots[a])}:
            assert mine.tolist() == [int(roots[a])]  # a lone node is a singleton
            singletons += 1
        else:
            assert sorted(inside) == sorted(core), a  # pass 1 took the whole neighbourhood
    # the coarse pattern is the set of aggregate pairs, columns sorted
    c_indptr, c_indices = coarse
    c_rows = np.repeat(np.arange(n_agg), np.diff(c_indptr))
    pairs = set(zip(agg[rows].tolist(), agg[indices].tolist()))
    assert set(zip(c_rows.tolist(), c_indices.tolist())) == pairs and c_indices.size == len(pairs)
    assert all((np.diff(c_indices[c_indptr[i]: c_indptr[i + 1]]) > 0).all() for i in range(n_agg))
    # the fold lists: ascending, every fine block exactly once, each in the block of its pair
    fold_ptr, fold = folds
    assert np.array_equal(np.sort(fold), np.arange(indices.size)) and fold_ptr[0] == 0 and fold_ptr[-1] == indices.size
    for kc in range(c_indices.size):
        mine = fold[fold_ptr[kc]: fold_ptr[kc + 1]]
        assert mine.size and (np.diff(mine) > 0).all()
        assert (agg[rows[mine]] == c_rows[kc]).all() and (agg[indices[mine]] == c_indices[kc]).all()
    return singletons


@pytest.mark.parametrize("shape", ["hex8", "tet_p2", "tri_p2", "interval"])
def test_aggregation_tables(shape):
    d_, a_, q_, affine = SHAPES[shape]
    singletons = 0
    for n_cells in (1, 5, 40):
        t = random_inputs(shape, n_cells, 7 + n_cells, False, affine)
        pat, unused = full_pattern(t["dofmap"], t["n_nodes"])
        assert unused.size  # the node no cell touches: alone in its row
        f = fc.InternalForce(fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"]), t["weights"])
        k = fc.TangentMatrix(f, pattern_dofmap=pat)
        pc = fc.MultilevelPreconditioner(k, coarsest_nodes=1)
        again = fc.MultilevelPreconditioner(k, coarsest_nodes=1)
        want = MU.hierarchy(k.indptr, k.indices, 1)
        assert len(pc.levels) == len(want) >= (2 if k.n_nodes > 1 else 1)
        for l in range(len(want) - 1):
            indptr, indices = pc.pattern(l)
            singletons += check_level(indptr, indices, pc.aggregates(l), pc.roots(l), pc.members(l), pc.folds(l), pc.pattern(l + 1))
            # the node-by-node oracle: the same tables
            assert np.array_equal(pc.aggregates(l), want[l].agg) and np.array_equal(pc.roots(l), want[l].roots)
            assert np.array_equal(pc.pattern(l + 1)[0], want[l + 1].indptr) and np.array_equal(pc.pattern(l + 1)[1], want[l + 1].indices)
            fold_ptr, fold = pc.folds(l)
            assert [fold[fold_ptr[i]: fold_ptr[i + 1]].tolist() for i in range(fold_ptr.size - 1)] == want[l].folds
            # two runs: identical tables
            for have, other in ((pc.aggregates(l), again.aggregates(l)), (pc.roots(l), again.roots(l)), *zip(pc.members(l), again.members(l)),
                                *zip(pc.folds(l), again.folds(l)), *zip(pc.pattern(l + 1), again.pattern(l + 1))):
                assert have.dtype == np.int32 and np.array_equal(have, other)
            assert (pc.diag_block(l + 1) >= 0).all()
        # levels end when one does not shrink or has one node
        assert pc.levels[-1]["nodes"] == 1 or multilevel.aggregate(*pc.pattern(len(want) - 1))[1].size == pc.levels[-1]["nodes"]
    assert singletons >= 3


def test_levels_of_the_cubes():
    for m, coarsest, nodes in ((6, 32, [343, 27]), (12, 32, [2197, 125, 8]), (12, 64, [2197, 125, 8]), (12, 125, [2197, 125]), (12, 3000, [2197])):
        mesh = FE.Cube(m, m, m)
        indptr, indices = block_pattern(mesh.cells, mesh.n_nodes)
        levels = multilevel.hierarchy(indptr, indices, coarsest)
        assert [lv.n_nodes for lv in levels] == nodes, (m, coarsest)
    assert [lv.n_nodes for lv in multilevel.hierarchy(indptr, indices, 1, max_levels=2)] == [2197, 125]


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the oracle: Galerkin values, both cycles, the solve
# ---------------------------------------------------------------------------------------------------------------------------------
def prolongator(agg, n_agg, d_):
    import scipy.sparse as sp

    n = agg.size
    rows = np.arange(d_ * n)
    cols = d_ * np.repeat(agg, d_) + np.tile(np.arange(d_), n)
    return sp.csr_matrix((np.ones(d_ * n), (rows, cols)), shape=(d_ * n, d_ * n_agg))


def test_galerkin_values_against_scipy(small_cube):
    k, indptr, indices, blocks, mask = small_cube
    o = MU.Oracle(indptr, indices, coarsest_nodes=1).setup(blocks)
    assert len(o.levels) == 3
    for l in range(len(o.levels) - 1):
        fine, coarse = o.levels[l], o.levels[l + 1]
        nf, nc = fine.indptr.size - 1, coarse.indptr.size - 1
        p = prolongator(fine.agg, nc, 3)
        want = (p.T @ to_bsr(fine.indptr, fine.indices, o.values[l], nf) @ p).toarray()
        size = (p.T @ to_bsr(fine.indptr, fine.indices, np.abs(o.values[l]), nf) @ p).toarray()
        have = to_bsr(coarse.indptr, coarse.indices, o.values[l + 1], nc).toarray()
        longest = max(len(x) for x in fine.folds)
        assert (np.abs(have - want) <= (longest + 2) * MU.EPS * size).all() and np.abs(want).max() > 0
        assert ((want != 0) <= (to_bsr(coarse.indptr, coarse.indices, np.ones_like(o.values[l + 1]), nc).toarray() != 0)).all()
    # a constrained dof adds 1.0 to its aggregate's diagonal: the coarse diagonal of direction z counts the constrained z dofs
    agg = o.levels[0].agg
    for a in range(o.levels[0].roots.size):
        held = mask.reshape(-1, 3)[agg == a]
        if held[:, 2].all():
            kd = int(np.flatnonzero((np.repeat(np.arange(o.levels[1].indptr.size - 1), np.diff(o.levels[1].indptr)) == a) & (o.levels[1].indices == a))[0])
            assert o.values[1][kd][2, 2] == float(held[:, 2].sum())


@pytest.mark.parametrize("cycle", CYCLES)
@pytest.mark.parametrize("coarsest", [3000, 20, 1], ids=["1 level", "2 levels", "3 levels"])
def test_cycles_are_symmetric_and_positive(cycle, coarsest, small_cube):
    k, indptr, indices, blocks, mask = small_cube
    o = MU.Oracle(indptr, indices, cycle=cycle, coarsest_nodes=coarsest, mask=mask).setup(blocks)
    assert len(o.levels) == {3000: 1, 20: 2, 1: 3}[coarsest] and not o.singular
    rng = np.random.default_rng(3)
    for _ in range(4):
        u, v = (np.where(mask, 0.0, rng.normal(size=mask.size)) for _ in range(2))
        mu, mv = o.apply(u), o.apply(v)
        # to rounding: a few hundred operations per entry, each within 2^-52 of sums bounded by |u|.|M^-1 v|
        scale = np.abs(u) @ np.abs(mv) + np.abs(v) @ np.abs(mu)
        assert abs(u @ mv - v @ mu) <= 1e3 * MU.EPS * scale
        assert u @ mu > 0 and v @ mv > 0
        assert (mu[mask].view(np.uint64) == 0).all() and (mv[mask].view(np.uint64) == 0).all()  # exactly +0.0


@pytest.mark.parametrize("cycle", CYCLES)
def test_oracle_solve_against_the_direct_solver(cycle, small_cube):
    import scipy.sparse.linalg as spla

    k, indptr, indices, blocks, mask = small_cube
    b = np.where(mask, 0.0, np.random.default_rng(5).normal(size=mask.size))
    want = spla.spsolve(to_bsr(indptr, indices, blocks, k.n_nodes).tocsc(), b)
    for coarsest in (3000, 20, 1):
        res = MU.conjugate_gradient(MU.Oracle(indptr, indices, cycle=cycle, coarsest_nodes=coarsest, mask=mask), blocks, b, rtol=1e-12)
        assert res.converged and res.status == "converged" and res.iterations > 0
        assert np.linalg.norm(res.x - want) <= 1e-6 * np.linalg.norm(want)
    zero = MU.conjugate_gradient(MU.Oracle(indptr, indices, cycle=cycle, coarsest_nodes=20, mask=mask), blocks, np.zeros(b.size))
    assert zero.status == "converged" and zero.iterations == 0
    x0 = np.random.default_rng(1).normal(size=b.size)
    sing = MU.conjugate_gradient(MU.Oracle(indptr, indices, cycle=cycle, coarsest_nodes=20, mask=mask), np.zeros_like(blocks), b, x0=x0)
    assert sing.status == "singular_block" and sing.iterations == 0 and np.array_equal(sing.x, x0)


def test_iterations_on_the_cube_of_twelve():
    """The issue's condition: elastic cube of 12^3 cells, tension constraints, seeded normal right-hand side zeroed at the
    constrained dofs, rtol 1e-8, coarsest_nodes 32 (levels 2197, 125, 8): the multiplicative cycle needs at most half of
    block-Jacobi's iterations, the additive cycle at most three quarters."""
    mesh = FE.Cube(12, 12, 12)
    k, indptr, indices, blocks, mask = cube_matrix(mesh)
    b = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mask.size))
    jacobi = conjugate_gradient(indptr, indices, blocks, b, rtol=1e-8)
    counts = {}
    for cycle in CYCLES:
        o = MU.Oracle(indptr, indices, cycle=cycle, coarsest_nodes=32, mask=mask)
        res = MU.conjugate_gradient(o, blocks, b, rtol=1e-8)
        assert [lv.indptr.size - 1 for lv in o.levels] == [2197, 125, 8]
        assert res.converged
        counts[cycle] = res.iterations
    print(f"cube of 12^3 cells: block-Jacobi {jacobi.iterations} iterations, multilevel {counts}")
    assert jacobi.converged
    assert 2 * counts["multiplicative"] <= jacobi.iterations, (counts, jacobi.iterations)
    assert 4 * counts["additive"] <= 3 * jacobi.iterations, (counts, jacobi.iterations)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. validation comes before any upload or launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_validation_errors(small_cube):
    torch = pytest.importorskip("torch")
    k = small_cube[0]
    other = cube_matrix(FE.Cube(1, 1, 2))[0]
    t = random_inputs("tet_p2", 5, 3, False, True)
    lonely = fc.TangentMatrix(fc.InternalForce(fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"]), t["weights"]))
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        ML = fc.MultilevelPreconditioner
        with pytest.raises(TypeError):
            ML(k.force)
        with pytest.raises(ValueError, match="no diagonal block"):
            ML(lonely)
        with pytest.raises(ValueError, match="cycle"):
            ML(k, cycle="w")
        with pytest.raises(ValueError, match="omega"):
            ML(k, omega=0.0)
        with pytest.raises(ValueError, match="omega"):
            ML(k, omega=math.inf)
        with pytest.raises(TypeError):
            ML(k, omega="half")
        with pytest.raises(TypeError):
            ML(k, smoothing=1.0)
        with pytest.raises(ValueError, match="smoothing"):
            ML(k, smoothing=0)
        with pytest.raises(ValueError, match="coarsest_nodes"):
            ML(k, coarsest_nodes=0)
        with pytest.raises(ValueError, match="coarsest_sweeps"):
            ML(k, coarsest_sweeps=0)
        with pytest.raises(TypeError):
            ML(k, max_levels=True)
        with pytest.raises(ValueError, match="max_levels"):
            ML(k, max_levels=0)
        pc = ML(k, cycle="additive", coarsest_nodes=8)
        with pytest.raises(ValueError, match="another matrix"):
            fc.ConjugateGradient(other, preconditioner=pc)
        with pytest.raises(ValueError, match="preconditioner"):
            fc.ConjugateGradient(k, preconditioner="Multilevel")
        with pytest.raises(ValueError, match="preconditioner"):
            fc.ConjugateGradient(k, preconditioner=object())
        with pytest.raises(ValueError, match="no level"):
            pc.pattern(2)
        with pytest.raises(ValueError, match="coarser"):
            pc.aggregates(1)
        n, nnz = k.shape[0], k.nnz
        host = lambda m: torch.zeros(m, dtype=torch.float64)  # noqa: E731
        with pytest.raises(TypeError):
            pc.setup(np.zeros(nnz))
        with pytest.raises(ValueError, match="cuda"):
            pc.setup(host(nnz))
        with pytest.raises(TypeError):
            pc.apply(host(nnz).float(), host(n))
        with pytest.raises(ValueError, match="cuda"):
            pc.apply(host(nnz), host(n))
        cg = fc.ConjugateGradient(k, preconditioner=pc)
        with pytest.raises(ValueError, match="cuda"):
            cg(host(nnz), host(n))
    finally:
        jit.launch = real
    assert not launches
    assert not pc._on and not cg._work and not k._on  # nothing was uploaded
