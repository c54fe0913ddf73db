"""The multilevel preconditioner of a matrix-free operator without a GPU (fenics_constitutive_amd.MultilevelPreconditioner on a
TangentOperator, csrc/jit/multilevel_free.hip): the programs compile for gfx950 without scratch and with the LDS the modules state;
the hierarchy is the one of the assembled route; every refusal comes before any upload or launch; the oracle's level-1 values
(multilevel_free_util.py) against the assembled route's Galerkin step within the rounding of two orders of one sum, on the bits for
every chunk size and exactly on integer inputs; and the oracle conjugate gradients in the Newton loop of
examples/cube_tension_matrix_free_multilevel.py against the direct solve."""

import os
import sys

import numpy as np
import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import gradient, jit, matrix, multilevel, solver
from fenics_constitutive_amd.force import kernel_resources

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_test_device_solve  # noqa: E402
from cube_tension_matrix_free import cube_operators  # noqa: E402
from fe_gpu_util import bits, tables_of  # noqa: E402
from gradient_util import SHAPES, cube_operator_tables  # noqa: E402
from matrix_util import matrix_oracle  # noqa: E402
import multilevel_free_util as MF  # noqa: E402
import multilevel_util as MU  # noqa: E402
from tangent_operator_util import distinct_inputs, random_mask  # noqa: E402

CYCLES = ("multiplicative", "additive")
ORACLE_SHAPES = ("hex8", "tet_p2", "tri_p2", "interval")
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}


def operator(shape="tet_p2", n_cells=9, seed=3, affine=True, every_node=True, **kwargs):
    t = distinct_inputs(shape, n_cells, seed, False, affine, every_node=every_node)
    f = fc.InternalForce(fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"]), t["weights"])
    return fc.TangentOperator(f, **kwargs), t


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. compilation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "per_point"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_program_compiles_without_scratch(shape, affine):
    d_, a_, q_, _ = SHAPES[shape]
    gather = multilevel.compile_free_kernels(d_, a_)
    r = kernel_resources(gather.log, multilevel.FREE_GALERKIN_KERNEL)
    assert r["scratch_bytes"] == 0 and r["lds_bytes"] == multilevel.lds_bytes(multilevel.FREE_GALERKIN_KERNEL) == 0, r
    before = jit.compile_count()
    assert multilevel.compile_free_kernels(d_, a_) is gather and jit.compile_count() == before  # once per program text
    # the element matrices: the assembled route's element kernel, compiled without a TangentMatrix
    element = matrix.compile_kernels(d_, a_, q_, affine)
    r = kernel_resources(element.log, matrix.ELEMENT_KERNEL)
    assert r["scratch_bytes"] == 0 and r["lds_bytes"] == matrix.lds_bytes(d_, a_, q_, affine, element.slab) <= gradient.LDS_CAP, r
    # the cycle: the program of the assembled route, as it is
    code = multilevel.compile_kernels(d_)
    for kernel in solver.KERNELS + multilevel.KERNELS:
        r = kernel_resources(code.log, kernel)
        assert r["scratch_bytes"] == 0 and r["lds_bytes"] == multilevel.lds_bytes(kernel), (kernel, r)
    # and the object holds exactly these
    a, t = operator(shape, 5, 3, affine)
    pc = fc.MultilevelPreconditioner(a, coarsest_nodes=2)
    assert pc._code is code and pc._seam.gather_code is gather and pc._seam.element_code is element
    assert pc.resources["free_galerkin"]["scratch_bytes"] == 0 and pc.resources["free_element"]["scratch_bytes"] == 0
    assert pc.K is a and pc.device == a.device and pc.lds_bytes() == 8 * 258 and all(kernel in pc.compile_log for kernel in multilevel.KERNELS)
    with pytest.raises(ValueError, match="dofs per node"):
        multilevel.compile_free_kernels(4, 4)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the hierarchy is the assembled route's
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_the_hierarchy_is_that_of_the_matrix(shape):
    d_, a_, q_, affine = SHAPES[shape]
    for n_cells, coarsest in ((1, 1), (9, 1), (40, 4), (None, 1)):
        if n_cells is None:  # a mesh: Cube(5, 4, 3) has three levels (random cells are one dense neighbourhood)
            if shape != "hex8":
                continue
            mesh = FE.Cube(5, 4, 3)
            a, t, n_cells = fc.TangentOperator(cube_operators(mesh)[1]), {"dofmap": np.ascontiguousarray(mesh.cells, dtype=np.int32)}, mesh.n_cells
        else:
            a, t = operator(shape, n_cells, 7 + n_cells, affine)
        pc = fc.MultilevelPreconditioner(a, coarsest_nodes=coarsest)
        pk = fc.MultilevelPreconditioner(fc.TangentMatrix(a.force), coarsest_nodes=coarsest)
        assert pc.levels == pk.levels and pc.coarse_dofs == pk.coarse_dofs == d_
        for l in range(len(pk.levels)):
            for have, want in zip(pc.pattern(l), pk.pattern(l)):
                assert have.dtype == want.dtype and np.array_equal(have, want)
            assert np.array_equal(pc.diag_block(l), pk.diag_block(l))
        for l in range(len(pk.levels) - 1):
            for have, want in ((pc.aggregates(l), pk.aggregates(l)), (pc.roots(l), pk.roots(l)), *zip(pc.members(l), pk.members(l)), *zip(pc.folds(l), pk.folds(l))):
                assert have.dtype == want.dtype and np.array_equal(have, want)
        if len(pk.levels) > 1:  # the contribution lists of level 1: every (c, a, b) once, in the coarse block of its aggregates, ascending
            seam, agg = pc._seam, pc.aggregates(0)
            indptr1, indices1 = pc.pattern(1)
            rows1 = np.repeat(np.arange(indptr1.size - 1), np.diff(indptr1))
            assert np.array_equal(np.sort(seam.contributions), np.arange(n_cells * a_ * a_)) and seam.blk_ptr[-1] == n_cells * a_ * a_
            for k in range(indices1.size):
                mine = seam.contributions[seam.blk_ptr[k]: seam.blk_ptr[k + 1]].astype(np.int64)
                c, an, bn = mine // (a_ * a_), mine % (a_ * a_) // a_, mine % a_
                assert mine.size and (np.diff(mine) > 0).all()
                assert (agg[t["dofmap"][c, an]] == rows1[k]).all() and (agg[t["dofmap"][c, bn]] == indices1[k]).all()
    assert len(pk.levels) >= (3 if shape == "hex8" else 2)
    # a node of no cell: the hierarchy of the matrix whose pattern gives that node a cell of its own
    from solver_util import full_pattern

    a, t = operator(shape, 9, 3, affine, every_node=False)
    pat, unused = full_pattern(t["dofmap"], t["n_nodes"])
    pc = fc.MultilevelPreconditioner(a, coarsest_nodes=1)
    pk = fc.MultilevelPreconditioner(fc.TangentMatrix(a.force, pattern_dofmap=pat), coarsest_nodes=1)
    assert t["lonely"] in unused.tolist() and pc.levels == pk.levels
    assert all(np.array_equal(x, y) for l in range(len(pk.levels)) for x, y in zip(pc.pattern(l), pk.pattern(l)))
    assert all(np.array_equal(pc.aggregates(l), pk.aggregates(l)) for l in range(len(pk.levels) - 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. every refusal comes before any upload or launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_and_upload_nothing():
    torch = pytest.importorskip("torch")
    a, t = operator()
    other, _ = operator(seed=4)
    lonely, _ = operator(every_node=False)
    k = fc.TangentMatrix(a.force)
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        ML, CG = fc.MultilevelPreconditioner, fc.ConjugateGradient
        pc = ML(a, cycle="additive", coarsest_nodes=4)
        assert CG(a, preconditioner=pc).preconditioner is pc
        # the three refusals the existing tests pin
        with pytest.raises(ValueError, match="multilevel"):
            CG(a, preconditioner="multilevel")
        with pytest.raises(ValueError, match="multilevel"):
            CG(a, preconditioner=ML(k))
        with pytest.raises(TypeError):
            ML(a.force)
        # a preconditioner built on another operator, or on an operator for a matrix
        with pytest.raises(ValueError, match="multilevel"):
            CG(a, preconditioner=ML(other))
        with pytest.raises(ValueError, match="multilevel"):
            CG(a, preconditioner=ML(fc.TangentOperator(a.force)))  # the same force, another object
        with pytest.raises(ValueError, match="another matrix"):
            CG(k, preconditioner=pc)
        # translations only
        with pytest.raises(ValueError, match="translations"):
            ML(a, coarse_space="rigid_body", coordinates=np.zeros((a.n_nodes, 3)))
        # a scratch that does not hold one tile of element matrices (one tile of the diagonal blocks is smaller: the operator takes it)
        m, cw = a.nodes_per_cell * a.gdim, matrix.cells_per_tile(a.gdim, a.nodes_per_cell)
        small = fc.TangentOperator(a.force, scratch_bytes=cw * m * m * 8 - 8)
        with pytest.raises(ValueError, match="scratch_bytes"):
            ML(small)
        assert ML(fc.TangentOperator(a.force, scratch_bytes=cw * m * m * 8), coarsest_nodes=4)._seam.chunk_cells == cw
        # what TangentOperator and MultilevelPreconditioner refuse already
        with pytest.raises(ValueError, match="belongs to no cell"):
            CG(lonely, preconditioner=ML(lonely))  # (the preconditioner alone takes it: a zero block, singular_block at setup)
        with pytest.raises(ValueError, match="cycle"):
            ML(a, cycle="w")
        with pytest.raises(ValueError, match="omega"):
            ML(a, omega=0.0)
        with pytest.raises(TypeError):
            ML(a, smoothing=1.0)
        with pytest.raises(ValueError, match="coarsest_nodes"):
            ML(a, coarsest_nodes=0)
        with pytest.raises(ValueError, match="coordinates"):
            ML(a, coordinates=np.zeros((a.n_nodes, 3)))
        # BiCGStab keeps refusing operators
        with pytest.raises(TypeError):
            fc.BiCGStab(a, preconditioner=pc)
        with pytest.raises(ValueError, match="another matrix"):
            fc.BiCGStab(k, preconditioner=pc)
        # the tensors
        n, nt = a.shape[0], a.tangent_dim * a.n_points
        host = lambda size: torch.zeros(size, dtype=torch.float64)  # noqa: E731
        cg = CG(a, preconditioner=pc)
        for call in (lambda x, y: pc.setup(x), lambda x, y: pc.apply(x, y), lambda x, y: cg(x, y)):
            with pytest.raises(TypeError):
                call(np.zeros(nt), host(n))
            with pytest.raises(TypeError):
                call(host(nt).float(), host(n))
            with pytest.raises(ValueError, match="cuda"):
                call(host(nt), host(n))
        with pytest.raises(AttributeError):
            pc.cycle = "multiplicative"
    finally:
        jit.launch = real
    assert not launches
    assert not pc._on and not cg._work and not cg._op._on and not a._mask_on and not a._scratch and not a.force._on and not a.op._on  # nothing was uploaded


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the oracle's values of level 1
# ---------------------------------------------------------------------------------------------------------------------------------
def level1_case(shape, n_cells, seed, integer, affine):
    """(tables, tangent, mask, hierarchy): random tables with random constrained dofs, every dof of the nodes of one cell constrained
    and every dof of the members of aggregate 0"""
    d_ = SHAPES[shape][0]
    t = distinct_inputs(shape, n_cells, seed, integer, affine)
    indptr, indices = matrix.block_pattern(t["dofmap"], t["n_nodes"])
    levels = MU.hierarchy(indptr, indices, 1)
    mask = random_mask(t, d_, seed + 1, whole_cell=n_cells // 2)
    mask |= np.repeat(levels[0].agg == 0, d_)
    return t, mask, levels


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_oracle_level_one_against_the_assembled_route(shape):
    """Both routes sum the same terms -- the entries ke[c][a][r][b][s] of matrix_util.element_matrices, on the bits, and 1.0 per
    constrained member on a coarse diagonal -- in two orders: block by block and then over the fold list, or in one chain.  Each
    chain of n terms is within (n - 1) 2^-53 sum|terms| of the exact sum (first order), the two of each other within
    (n - 1) 2^-52 sum|terms|; the bound used is (n + 2) 2^-52 S with n the longest chain (the contributions of a coarse block and the
    members its start counts) and S the oracle's own sum with every factor of ke replaced by its absolute value."""
    d_, a_, q_, affine = SHAPES[shape]
    for per_point in (affine, not affine):
        t, mask, levels = level1_case(shape, 40, 5, False, per_point)
        fine, coarse = levels[0], levels[1]
        assert len(levels) >= 2 and mask.reshape(-1, d_)[t["dofmap"][20]].all() and mask.reshape(-1, d_)[fine.agg == 0].all()
        args = (t["tangent"], *tables_of(t), fine.agg, coarse.indptr, coarse.indices)
        have = MF.level1_values(*args, mask=mask)
        size = MF.level1_values(*args, mask=mask, absolute=True)
        _, _, blocks = matrix_oracle(t["tangent"], *tables_of(t), constrained=mask)
        want = MU.galerkin(fine.folds, blocks)
        chain = MF.longest_chain(t["dofmap"], fine.agg, coarse.indptr, coarse.indices)
        error = np.abs(have - want)
        print(f"{shape} affine={per_point}: largest |difference| / bound {np.max(error / np.maximum((chain + 2) * MF.EPS * size, 1e-300)):.3f}, longest chain {chain}, "
              f"share of the largest entry {error.max() / np.abs(want).max():.1e}")
        assert (error <= (chain + 2) * MF.EPS * size).all() and np.abs(want).max() > 0
        # the aggregate whose dofs are all constrained: its coarse diagonal block counts its members, its other blocks are +0.0
        rows1 = np.repeat(np.arange(coarse.indptr.size - 1), np.diff(coarse.indptr))
        for k in np.flatnonzero((rows1 == 0) | (coarse.indices == 0)):
            own = rows1[k] == 0 and coarse.indices[k] == 0
            assert np.array_equal(bits(have[k]), bits(float((fine.agg == 0).sum()) * np.eye(d_) if own else np.zeros((d_, d_)))), k
        # without a mask: the plain sums
        plain = MF.level1_values(*args)
        _, _, blocks = matrix_oracle(t["tangent"], *tables_of(t))
        assert (np.abs(plain - MU.galerkin(fine.folds, blocks)) <= (chain + 2) * MF.EPS * MF.level1_values(*args, absolute=True)).all()


def test_oracle_level_one_on_a_mesh():
    """the same comparison where the hierarchy is deep and the aggregates are many: Cube(3, 2, 4) under the tension constraints
    (60 nodes, levels 60, 4 at coarsest_nodes=4; the preconditioner built on the operator holds the same lists)"""
    from cube_tension_device_solve import tension_constraints
    from solver_util import spd_tangent

    mesh = FE.Cube(3, 2, 4)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    weights = gradient.integration_weights(mesh.nodes[mesh.cells], ref, np.ones(8))
    tables = (dofmap, ref, jinv, weights, mesh.n_nodes)
    mask, _ = tension_constraints(mesh)
    tangent = spd_tangent(mesh.n_points, 6, 1, False)
    o = MF.FreeOracle(*tables, mask=mask, coarsest_nodes=4).setup(tangent)
    fine, coarse = o.levels[0], o.levels[1]
    assert [lv.indptr.size - 1 for lv in o.levels] == [60, 4] and not o.singular
    indptr, indices, blocks = matrix_oracle(tangent, *tables, constrained=mask)
    want = MU.Oracle(indptr, indices, coarsest_nodes=4, mask=mask).setup(blocks)
    size = MF.level1_values(tangent, *tables, fine.agg, coarse.indptr, coarse.indices, mask=mask, absolute=True)
    chain = MF.longest_chain(dofmap, fine.agg, coarse.indptr, coarse.indices)
    error = np.abs(o.values[1] - want.values[1])
    print(f"Cube(3, 2, 4): level-1 values from the elements against the assembled route: {error.max() / np.abs(want.values[1]).max():.1e} of the largest entry")
    assert (error <= (chain + 2) * MF.EPS * size).all()
    assert np.array_equal(bits(o.diagonal), bits(blocks[np.flatnonzero(np.repeat(np.arange(60), np.diff(indptr)) == indices)]))  # level 0: the matrix's own blocks
    # the oracle forms blocks and level 1 from one set of element matrices; chunk by chunk, through the operator's oracle: the same bits
    from tangent_operator_util import diagonal_blocks_oracle

    chunked = MF.FreeOracle(*tables, mask=mask, coarsest_nodes=4, chunk_cells=5).setup(tangent)
    assert np.array_equal(bits(chunked.diagonal), bits(o.diagonal)) and np.array_equal(bits(chunked.values[1]), bits(o.values[1]))
    assert np.array_equal(bits(o.diagonal), bits(diagonal_blocks_oracle(tangent, *tables, mask=mask)))


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_oracle_level_one_does_not_depend_on_the_chunks(shape):
    d_, a_, q_, affine = SHAPES[shape]
    n_cells = 11
    t, mask, levels = level1_case(shape, n_cells, 9, False, affine)
    args = (t["tangent"], *tables_of(t), levels[0].agg, levels[1].indptr, levels[1].indices)
    want = MF.level1_values(*args, mask=mask)
    for chunk in (1, 2, n_cells - 1, n_cells):
        assert np.array_equal(bits(MF.level1_values(*args, mask=mask, chunk_cells=chunk)), bits(want)), (shape, chunk)
    assert np.abs(want).max() > 0


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_oracle_level_one_is_exact_on_integers(shape):
    """Element matrices of small integers: every sum of both routes is exact, so the two orders of summation give the same number.
    (The element matrices of integer TABLES are not integers where D > 1 -- the double of sqrt(0.5) enters twice --, so the rule
    is checked on integer element matrices for every shape, and on integer tables where the whole chain is exact: D = 1.)"""
    from matrix_util import apply_constraints, block_sums

    d_, a_, q_, affine = SHAPES[shape]
    n_cells = 12
    t, mask, levels = level1_case(shape, n_cells, 14, True, affine)
    indptr, indices = matrix.block_pattern(t["dofmap"], t["n_nodes"])
    ke = np.random.default_rng(3).integers(-8, 9, size=(n_cells, a_, d_, a_, d_)).astype(np.float64)
    args = (None, *tables_of(t), levels[0].agg, levels[1].indptr, levels[1].indices)
    for m in (None, mask):
        blocks = block_sums(ke, t["dofmap"], t["n_nodes"], indptr, indices)
        if m is not None:
            blocks = apply_constraints(blocks, indptr, indices, m)
        have = MF.level1_values(*args, mask=m, chunk_cells=5, ke_all=ke)
        assert np.array_equal(have, MU.galerkin(levels[0].folds, blocks)) and np.abs(have).max() > 0 and np.array_equal(have, np.round(have))
        if d_ == 1:
            _, _, blocks = matrix_oracle(t["tangent"], *tables_of(t), constrained=m)
            have = MF.level1_values(t["tangent"], *args[1:], mask=m, chunk_cells=5)
            assert np.array_equal(have, MU.galerkin(levels[0].folds, blocks)) and np.abs(have).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the Newton loop of the example on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", CYCLES)
def test_oracle_solves_of_the_cube_reproduce_the_direct_solver(cycle):
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    weights = gradient.integration_weights(mesh.nodes[mesh.cells], ref, np.ones(8))

    def cpu_state():
        return FE.CopyProtocolState(FE.OracleLaw(O.von_mises_3d, VM_P, {"eps_n": 6, "alpha": 1}), mesh.n_points)

    direct = FE.tension_test(mesh, cpu_state(), steps=8)
    loop = MF.oracle_free_multilevel_loop(cpu_state(), dofmap, ref, jinv, weights, mesh.n_nodes, rtol=1e-12, cycle=cycle, coarsest_nodes=8)
    reactions, norms, u, solves = tension_test_device_solve(mesh, loop, steps=8)
    counts = [len(h) for h in norms]
    difference = np.max(np.abs(reactions - direct[0])) / np.max(np.abs(direct[0]))
    print(f"oracle loop, operator + multilevel {cycle}: Newton iterations {counts}, conjugate-gradient iterations {solves}, "
          f"largest relative reaction difference to the direct solve {difference:.2e}")
    assert counts == [len(h) for h in direct[1]] == [2, 2, 2, 3, 3, 4, 5, 5]
    assert len(loop.systems) == len(solves) == sum(counts) - 8
    assert all(result.converged for _, _, result in loop.systems)
    assert difference <= 1e-8
