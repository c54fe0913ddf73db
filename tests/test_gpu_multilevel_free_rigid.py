"""The rigid-body coarse space on a matrix-free operator on the GPU (fenics_constitutive_amd.MultilevelPreconditioner(A,
coarse_space="rigid_body") with a TangentOperator, csrc/jit/multilevel_free_rigid.hip): the values AND the inverses of every level,
one application of both cycles and whole runs of ConjugateGradient and MatrixFreeBiCGStab compared ON THE BITS with the NumPy oracle
of multilevel_free_rigid_util.py -- for every scratch size, on hierarchies of one, two and three levels, under a grid capped at one
compute unit, for every ``check_every`` --, the status of a tangent that is not finite, the translations of the same operator and
the assembled rigid-body route untouched next to it, and the Newton loop of examples/cube_tension_matrix_free_rigid_body.py.  Every
output a caller hands in lies between canaries."""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_test_device_solve  # noqa: E402
from cube_tension_matrix_free_rigid_body import matrix_free_rigid_body_loop  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import gradient, matrix, multilevel, solver  # noqa: E402
from fenics_constitutive_amd import tangent_operator as to  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402
import bicgstab_free_util as BF  # noqa: E402
from fe_gpu_util import bits, guarded, assert_margins_intact, assert_same_bits, solve_guarded, assert_same_result  # noqa: E402
from fe_gpu_util import tables_of, force_of, status_of, cube_system_of  # noqa: E402
from fe_gpu_util import one_cu  # noqa: E402, F401 (the fixture: pytest finds it in this namespace)
from force_util import MANDEL_DIM, cell_counts  # noqa: E402
import multilevel_free_rigid_util as FR  # noqa: E402
import multilevel_free_util as MF  # noqa: E402
import rigid_body_util as RU  # noqa: E402
from solver_util import SEG, from_format, spd_tangent  # noqa: E402
from tangent_operator_util import TILING_SHAPES as SHAPES  # noqa: E402
from tangent_operator_util import distinct_inputs, random_mask  # noqa: E402

CYCLES = ("multiplicative", "additive")
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
SINGULAR = solver.STATUSES.index("singular_block")
RIGID = {"coarse_space": "rigid_body"}


def coordinates_of(t, d_, seed):
    return np.random.default_rng(seed + 77).normal(size=(t["n_nodes"], d_))


def assert_levels_on_the_bits(pc, o, what):
    """the values of the levels l >= 1 and the inverses of the own blocks of every level"""
    on = pc._on[pc.device]
    for l in range(len(o.levels)):
        if l:
            assert_same_bits(to_host(on.values[l])[: o.values[l].size], o.values[l], f"{what}: the values of level {l}")
        assert_same_bits(to_host(on.inv[l])[: o.inv[l].size], o.inv[l], f"{what}: the inverses of level {l}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. setup: the values and the inverses of every level
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "per_point"])
@pytest.mark.parametrize("shape", ("hex8", "tet_p2", "tri_p2"))
def test_setup_on_the_bits(shape, affine):
    d_, a_, q_, _ = SHAPES[shape]
    dc = RU.coarse_dofs(d_)
    cw = matrix.cells_per_tile(d_, a_)
    tile = cw * (a_ * d_) ** 2 * 8
    deepest = 0
    for n_cells in cell_counts(cw, q_):
        t = distinct_inputs(shape, n_cells, 3 + n_cells, False, affine, every_node=True)
        x = coordinates_of(t, d_, n_cells)
        f = force_of(t)
        agg = fc.MultilevelPreconditioner(fc.TangentOperator(f), coarsest_nodes=1, coordinates=x, **RIGID).aggregates(0)
        # random constrained dofs, every dof of a cell's nodes, every dof of the members of aggregate 0
        held = random_mask(t, d_, n_cells, whole_cell=n_cells // 2) | np.repeat(agg == 0, d_)
        some = random_mask(t, d_, n_cells + 1, whole_cell=n_cells // 2)
        unsymmetric = BF.unsymmetric_tangent(n_cells * q_, d_, 5 + n_cells)
        for mask, values, scratches in ((None, t["tangent"], (tile, 2 * tile + 8, None)), (held, t["tangent"], (tile, 2 * tile + 8, None)),
                                        (some, unsymmetric, (tile, None))):
            tangent = to_device(values, "cuda")
            o = FR.FreeRigidOracle(*tables_of(t), x, mask=mask, coarsest_nodes=1).setup(values)
            for scratch in scratches:  # one tile of element matrices, two, everything
                what = f"{shape} affine={affine} cells={n_cells} scratch={scratch} mask={'no' if mask is None else 'aggregate' if mask is held else 'random'}"
                a = fc.TangentOperator(f, scratch_bytes=scratch)
                a.set_constrained(mask)
                pc = fc.MultilevelPreconditioner(a, coarsest_nodes=1, coordinates=x, **RIGID)
                assert len(pc._seam.chunks()) == {tile: -(-n_cells // cw), 2 * tile + 8: -(-n_cells // (2 * cw)), None: 1}[scratch], what
                coarse = pc.setup(tangent)
                assert status_of(pc) == (SINGULAR if o.singular else 0), what
                assert len(coarse) == len(o.levels) - 1 == len(pc.levels) - 1, what
                for l, have in enumerate(coarse, 1):
                    assert have.numel() == dc * dc * pc.levels[l]["blocks"]
                    assert_same_bits(to_host(have), o.values[l], f"{what} level {l}")
                assert_levels_on_the_bits(pc, o, what)
                assert_same_bits(to_host(pc._on[a.device].blocks), o.diagonal, f"{what}: the nodes' own blocks")
                deepest = max(deepest, len(pc.levels))
            assert_same_bits(to_host(pc.setup(tangent)[0]), o.values[1], f"{what}: a second setup")
            assert_same_bits(to_host(tangent), values, "the tangent was written")
    assert deepest >= 2


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. one application
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_cube():
    """the tension-test operator of Cube(5, 4, 3) (120 nodes) on a random positive definite tangent; the scratch holds 16 of the 60
    element matrices"""
    mesh = FE.Cube(5, 4, 3)
    return (mesh,) + cube_system_of(mesh, 1, scratch_bytes=16 * 576 * 8)


@pytest.mark.parametrize("cycle", CYCLES)
def test_apply_on_the_bits(cycle, small_cube):
    mesh, f, tables, mask, a, tangent = small_cube
    n = a.shape[0]
    rng = np.random.default_rng(8)
    r = np.where(mask, 0.0, rng.normal(size=n))
    tangent_dev = to_device(tangent, "cuda")
    for coarsest, depth in ((3000, 1), (20, 2), (1, 3)):
        for smoothing in (1, 2):
            what = f"{cycle} levels={depth} smoothing={smoothing}"
            options = dict(cycle=cycle, smoothing=smoothing, coarsest_nodes=coarsest)
            pc = fc.MultilevelPreconditioner(a, coordinates=mesh.nodes, **RIGID, **options)
            assert len(pc.levels) == depth and len(pc._seam.chunks()) == 4, what
            o = FR.FreeRigidOracle(*tables, mesh.nodes, mask=mask, **options).setup(tangent)
            r_dev = to_device(r, "cuda")
            buf, out = guarded(n)
            assert pc.apply(tangent_dev, r_dev, out=out).data_ptr() == out.data_ptr()
            torch.cuda.synchronize()
            assert_margins_intact(buf, n)
            have = to_host(out)
            assert_levels_on_the_bits(pc, o, what)
            assert_same_bits(have, o.apply(r), what)
            assert np.isfinite(have).all() and np.abs(have).max() > 0 and status_of(pc) == 0 and (bits(have[mask]) == 0).all(), what
            # a second right-hand side in the same tensors: the cached plan; and without out
            plans = dict(pc._on[a.device].plans)
            second = rng.normal(size=n)
            r_dev.copy_(to_device(second, "cuda"))
            pc.apply(tangent_dev, r_dev, out=out)
            torch.cuda.synchronize()
            assert_margins_intact(buf, n)
            assert list(pc._on[a.device].plans.values())[-1] is list(plans.values())[-1], what  # the same launch list, replayed
            assert_same_bits(to_host(out), o.apply(second), f"{what}: a second right-hand side through the cached plan")
            assert_same_bits(to_host(pc.apply(tangent_dev, r_dev)), to_host(out), f"{what}: without out")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. exactly k iterations on three levels, 2-D and 3-D, both solvers
# ---------------------------------------------------------------------------------------------------------------------------------
def strip_2d(nx=12, ny=6, seed=21):
    """tri_p2 tables (random, per cell) on a structured dofmap: the nodes of an nx x ny grid, the cell (i, j) names the six nodes of
    the window 2 x 3 at (i, j) -- a sparse node graph, so the hierarchy is deep --; the coordinates are the grid's, sheared"""
    cells = [[(i + di) * ny + (j + dj) for di in range(2) for dj in range(3)] for i in range(nx - 1) for j in range(ny - 2)]
    t = distinct_inputs("tri_p2", len(cells), seed, False, True, every_node=True)
    t["dofmap"], t["n_nodes"] = np.array(cells, dtype=np.int32), nx * ny
    i, j = np.divmod(np.arange(nx * ny), ny)
    return t, np.stack([i + 0.25 * j, 0.5 * j - 0.125 * i], axis=1).astype(np.float64)


def k_system(dim):
    """(operator, tables, coordinates, mask, symmetric tangent, unsymmetric tangent)"""
    if dim == 2:
        t, x = strip_2d()
        tables, n_points = tables_of(t), t["dofmap"].shape[0] * SHAPES["tri_p2"][2]
        a = fc.TangentOperator(force_of(t))
        mask = random_mask(t, 2, 26)
    else:
        mesh = FE.Cube(5, 4, 3)
        f, tables, mask, a, _ = cube_system_of(mesh, 1)
        a, x, n_points = fc.TangentOperator(f), mesh.nodes, mesh.n_points
    a.set_constrained(mask)
    return a, tables, x, mask, spd_tangent(n_points, MANDEL_DIM[dim], 21, False), BF.unsymmetric_tangent(n_points, dim, 21)


@pytest.mark.parametrize("dim", [2, 3])
def test_exactly_k_iterations(dim):
    a, tables, x, mask, symmetric, unsymmetric = k_system(dim)
    n = a.shape[0]
    rng = np.random.default_rng(4)
    b = np.where(mask, 0.0, rng.normal(size=n))
    start = rng.normal(size=n)
    coarsest = {2: 2, 3: 1}[dim]  # three levels: 72, 8, 2 nodes on the strip and 120, 8, 1 on the cube
    for cycle in CYCLES:
        pc = fc.MultilevelPreconditioner(a, cycle=cycle, coarsest_nodes=coarsest, coordinates=x, **RIGID)
        assert len(pc.levels) == 3 and pc.coarse_dofs == RU.coarse_dofs(dim)
        for S, tangent, solve in ((fc.ConjugateGradient, symmetric, FR.conjugate_gradient), (fc.MatrixFreeBiCGStab, unsymmetric, FR.bicgstab)):
            o = FR.FreeRigidOracle(*tables, x, mask=mask, cycle=cycle, coarsest_nodes=coarsest)
            tangent_dev = to_device(tangent, "cuda")
            for its in (1, 2, 7):
                s = S(a, preconditioner=pc, rtol=0.0, maxiter=its)
                for x0 in (None, start):
                    what = f"{dim}-D {S.__name__} {cycle} k={its} x0={'yes' if x0 is not None else 'no'}"
                    want = solve(o, tangent, b, x0=x0, rtol=0.0, maxiter=its)
                    res, got = solve_guarded(s, tangent_dev, b, x0)
                    assert want.status == "maxiter" and want.iterations == its, what
                    assert_same_result(res, got, want, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. a cube with two segments: check_every, the status of a tangent that is not finite, the other routes next to it
# ---------------------------------------------------------------------------------------------------------------------------------
KWS = ((("rtol", 0.0), ("maxiter", 11)), (("rtol", 1e-6),))


@pytest.fixture(scope="module")
def cube_system():
    """the tension-test operator of a 10 x 10 x 9 cube (3630 dofs: two segments; three levels at coarsest_nodes=32), its right-hand
    side and the oracle's solves"""
    mesh = FE.Cube(10, 10, 9)
    f, tables, mask, a, tangent = cube_system_of(mesh, 1)
    assert SEG < mesh.n_dofs <= 2 * SEG
    b = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mesh.n_dofs))
    oracle = {(cycle, kw): FR.conjugate_gradient(FR.FreeRigidOracle(*tables, mesh.nodes, mask=mask, cycle=cycle, coarsest_nodes=32), tangent, b, **dict(kw))
              for cycle in CYCLES for kw in KWS}
    return mesh, f, tables, mask, a, tangent, b, oracle


@pytest.mark.parametrize("cycle", CYCLES)
def test_check_every_changes_nothing(cycle, cube_system):
    mesh, f, tables, mask, a, tangent, b, oracle = cube_system
    pc = fc.MultilevelPreconditioner(a, cycle=cycle, coarsest_nodes=32, coordinates=mesh.nodes, **RIGID)
    assert len(pc.levels) == 3
    tangent_dev = to_device(tangent, "cuda")
    for kw in KWS:
        want = oracle[(cycle, kw)]
        assert want.status == ("maxiter" if "maxiter" in dict(kw) else "converged") and want.iterations >= 11
        for every in (1, 3, 16):  # (11 iterations end in the middle of a batch of 3 and of 16)
            res, x = solve_guarded(fc.ConjugateGradient(a, preconditioner=pc, check_every=every, **dict(kw)), tangent_dev, b)
            assert_same_result(res, x, want, f"{cycle} {dict(kw)} check_every={every}")
            assert res.looks == 1 + -(-want.iterations // every)


def test_a_tangent_that_is_not_finite_is_a_singular_block(cube_system):
    """one entry of the tangent is NaN: it reaches the nodes' own blocks of its cell and, through the first Galerkin step, a coarse
    block; the inverse kernels report it through the control block -- no iteration, x is x0, nothing faults"""
    mesh, f, tables, mask, a, tangent, b, oracle = cube_system
    bad = tangent.copy()
    bad[36 * 8 * 400 + 7] = np.nan
    start = np.random.default_rng(2).normal(size=b.size)
    for cycle in CYCLES:
        pc = fc.MultilevelPreconditioner(a, cycle=cycle, coarsest_nodes=32, coordinates=mesh.nodes, **RIGID)
        o = FR.FreeRigidOracle(*tables, mesh.nodes, mask=mask, cycle=cycle, coarsest_nodes=32).setup(bad)
        assert o.singular and not np.isfinite(o.values[1]).all()
        bad_dev = to_device(bad, "cuda")
        pc.setup(bad_dev)
        assert status_of(pc) == SINGULAR
        assert_same_bits(to_host(pc._on[a.device].values[1])[: o.values[1].size], o.values[1], f"{cycle}: level 1 of a tangent with a NaN")
        for S in (fc.ConjugateGradient, fc.MatrixFreeBiCGStab):
            s = S(a, preconditioner=pc, rtol=1e-6)
            res, x = solve_guarded(s, bad_dev, b, start)
            assert (res.status, res.iterations, res.converged) == ("singular_block", 0, False), (cycle, S.__name__)
            assert_same_bits(x, start, f"{cycle} {S.__name__}: singular block")
        # and the object solves again afterwards
        res, x = solve_guarded(fc.ConjugateGradient(a, preconditioner=pc, **dict(KWS[1])), tangent, b)
        assert_same_result(res, x, oracle[(cycle, KWS[1])], f"{cycle}: after the status")


def test_side_by_side_with_the_translations_and_the_assembled_routes(cube_system):
    """a translation and a rigid-body instance of ONE operator alternating on the same vectors, each on its own oracle's bits; and in
    the same process MultilevelPreconditioner(K, coarse_space="rigid_body") and MultilevelPreconditioner(A), on theirs"""
    from matrix_util import matrix_oracle

    mesh, f, tables, mask, a, tangent, b, oracle = cube_system
    n = b.size
    tangent_dev = to_device(tangent, "cuda")
    rng = np.random.default_rng(5)
    for cycle in CYCLES:
        options = dict(cycle=cycle, coarsest_nodes=32)
        rigid = fc.MultilevelPreconditioner(a, coordinates=mesh.nodes, **RIGID, **options)
        plain = fc.MultilevelPreconditioner(a, **options)
        assert plain._code is multilevel.compile_kernels(3) and plain._seam.gather_code is multilevel.compile_free_kernels(3, 8)
        assert rigid._seam.gather_code is multilevel.compile_free_rigid_kernels(3, 8)
        o_rigid = FR.FreeRigidOracle(*tables, mesh.nodes, mask=mask, **options).setup(tangent)
        o_plain = MF.FreeOracle(*tables, mask=mask, **options).setup(tangent)
        r_dev = torch.zeros(n, dtype=torch.float64, device="cuda")
        buf, out = guarded(n)
        for turn in range(2):
            r = np.where(mask, 0.0, rng.normal(size=n))
            r_dev.copy_(to_device(r, "cuda"))
            for pc, o, name in ((rigid, o_rigid, "rigid body"), (plain, o_plain, "translations")):
                pc.apply(tangent_dev, r_dev, out=out)
                torch.cuda.synchronize()
                assert_margins_intact(buf, n)
                assert_same_bits(to_host(out), o.apply(r), f"{cycle} turn {turn}: {name}")
        res, x = solve_guarded(fc.ConjugateGradient(a, preconditioner=plain, rtol=0.0, maxiter=7), tangent_dev, b)
        assert_same_result(res, x, MF.conjugate_gradient(o_plain, tangent, b, rtol=0.0, maxiter=7, setup=False), f"{cycle}: ConjugateGradient(A, translations)")
        res, x = solve_guarded(fc.ConjugateGradient(a, preconditioner=rigid, rtol=0.0, maxiter=7), tangent_dev, b)
        free = FR.conjugate_gradient(o_rigid, tangent, b, rtol=0.0, maxiter=7, setup=False)
        assert_same_result(res, x, free, f"{cycle}: ConjugateGradient(A, rigid body)")
        # the assembled route with the rigid-body modes
        k = fc.TangentMatrix(f)
        k.set_constrained(mask)
        values = k(tangent_dev)
        blocks = from_format("bsr", k.indptr, k.indices, to_host(values), 3)
        assert_same_bits(blocks, matrix_oracle(tangent, *tables, constrained=mask)[2], "the assembled values")
        pk = fc.MultilevelPreconditioner(k, coordinates=mesh.nodes, **RIGID, **options)
        buf, out = guarded(n)
        res = fc.ConjugateGradient(k, preconditioner=pk, rtol=0.0, maxiter=7)(values, to_device(b, "cuda"), out=out)
        assert_margins_intact(buf, n)
        want = RU.conjugate_gradient(RU.Oracle(k.indptr, k.indices, mesh.nodes, mask=mask, **options), blocks, b, rtol=0.0, maxiter=7)
        assert_same_result(res, to_host(out), want, f"{cycle}: ConjugateGradient(K, rigid body)")
        assert np.allclose(to_host(out), free.x, rtol=1e-7, atol=1e-10 * np.abs(want.x).max())  # one preconditioner, to rounding


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. one compute unit
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_cube():
    """the tension-test operator of a cube of 32^3 hexahedra (35 937 nodes; levels 35937, 1331, 64); the scratch of 64 MiB holds
    14 562 of the 32 768 element matrices: three chunks"""
    import copy

    mesh = FE.Cube(32, 32, 32)
    f, tables, mask, a, tangent = cube_system_of(mesh, 2, scratch_bytes=64 * 1024 * 1024)
    assert -(-mesh.n_dofs // SEG) > 2 * gradient.BLOCKS_PER_CU
    first = FR.FreeRigidOracle(*tables, mesh.nodes, mask=mask, cycle=CYCLES[0]).setup(tangent)
    oracles = {CYCLES[0]: first, CYCLES[1]: copy.copy(first)}  # (the values and inverses do not depend on the cycle: formed once)
    oracles[CYCLES[1]].cycle = CYCLES[1]
    return mesh, tables, mask, a, tangent, oracles


@pytest.mark.parametrize("cycle", CYCLES)
def test_apply_on_one_compute_unit(cycle, big_cube, one_cu):
    mesh, tables, mask, a, tangent, oracles = big_cube
    o = oracles[cycle]
    assert [lv.indptr.size - 1 for lv in o.levels] == [35937, 1331, 64]
    n = a.shape[0]
    r = np.where(mask, 0.0, np.random.default_rng(3).normal(size=n))
    pc = fc.MultilevelPreconditioner(a, cycle=cycle, coordinates=mesh.nodes, **RIGID)
    assert len(pc._seam.chunks()) == 3
    tangent_dev = to_device(tangent, "cuda")
    buf, out = guarded(n)
    del one_cu[:]
    pc.apply(tangent_dev, to_device(r, "cuda"), out=out)
    torch.cuda.synchronize()
    assert_margins_intact(buf, n)
    assert_levels_on_the_bits(pc, o, f"cube 32 {cycle}, one compute unit")
    assert_same_bits(to_host(out), o.apply(r), f"cube 32 {cycle}, one compute unit")
    assert max(nb for _, nb in one_cu) == gradient.BLOCKS_PER_CU  # the launches really were capped
    capped = {name for name, nb in one_cu if nb == gradient.BLOCKS_PER_CU}
    assert {multilevel.FREE_RIGID_GALERKIN_KERNEL, matrix.ELEMENT_KERNEL, multilevel.RIGID_GALERKIN_KERNEL, multilevel.SMOOTH_KERNEL, multilevel.RIGID_PROLONG_KERNEL,
            multilevel.RIGID_RESTRICT_KERNEL, solver.INVERSE_KERNEL, to.DIAGONAL_ELEMENT_KERNEL, to.DIAGONAL_NODE_KERNEL} <= capped
    assert ({to.ELEMENT_KERNEL, to.NODE_KERNEL} <= capped) == (cycle == "multiplicative")  # level-0 products: the operator's two launches
    assert sum(name == multilevel.FREE_RIGID_GALERKIN_KERNEL for name, _ in one_cu) == 3  # one gather per chunk
    assert not any(name == multilevel.FREE_GALERKIN_KERNEL for name, _ in one_cu)
    # two iterations of the whole solve under the cap
    del one_cu[:]
    res, x = solve_guarded(fc.ConjugateGradient(a, preconditioner=pc, rtol=0.0, maxiter=2, check_every=2), tangent_dev, r)
    assert_same_result(res, x, FR.conjugate_gradient(o, tangent, r, rtol=0.0, maxiter=2, setup=False), f"cube 32 {cycle}, two iterations on one compute unit")
    assert (multilevel.CLOSE_KERNEL, gradient.BLOCKS_PER_CU) in one_cu


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the Newton loop of the example
# ---------------------------------------------------------------------------------------------------------------------------------
def test_in_the_loop_of_the_example():
    """The tension test of examples/cube_tension_matrix_free_rigid_body.py on Cube(3, 2, 4), eight load steps, both cycles, against
    ``fe_mini.tension_test`` on the CPU with the oracle law and SciPy's direct solver: the direct solve's Newton counts, the largest
    relative reaction difference at most 1e-8, and no matrix anywhere in the loop."""
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    cpu = FE.CopyProtocolState(FE.OracleLaw(O.von_mises_3d, VM_P, {"eps_n": 6, "alpha": 1}), mesh.n_points)
    r_direct, norms_direct, _ = FE.tension_test(mesh, cpu, steps=8)
    for cycle in CYCLES:
        loop = matrix_free_rigid_body_loop(mesh, fc.VonMises3D(VM_P), cycle, coarsest_nodes=8)
        pc = loop.cg.preconditioner
        assert len(pc.levels) == 2 and pc.K is loop.K and (pc.coarse_space, pc.coarse_dofs) == ("rigid_body", 6)
        r_gpu, norms_gpu, u, solves = tension_test_device_solve(mesh, loop, steps=8)  # (raises where a solve or a load step does not converge)
        difference = np.max(np.abs(r_gpu - r_direct)) / np.max(np.abs(r_direct))
        counts = [len(h) for h in norms_gpu]
        print(f"matrix-free rigid-body tension test, {cycle}: GPU against direct {difference:.3e}, Newton iterations {counts}, conjugate-gradient iterations {solves}")
        assert counts == [len(h) for h in norms_direct] == [2, 2, 2, 3, 3, 4, 5, 5]
        assert difference <= 1e-8, difference
        assert not any(isinstance(x, fc.TangentMatrix) for x in vars(loop).values())
