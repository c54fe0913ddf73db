"""The multilevel preconditioner of a matrix-free operator on the GPU (fenics_constitutive_amd.MultilevelPreconditioner on a
TangentOperator, csrc/jit/multilevel_free.hip): the values of every coarse level and the nodes' own blocks, one application of both
cycles and whole conjugate-gradient runs compared ON THE BITS with the NumPy oracle of multilevel_free_util.py -- for every scratch
size, on hierarchies of one, two and three levels, under a grid capped at one compute unit, for every ``check_every`` --, the
statuses and refusals, the assembled route and block-Jacobi untouched next to it, and the Newton loop of
examples/cube_tension_matrix_free_multilevel.py.  Every output a caller hands in lies between canaries.  The setup also runs at
``q3``, ``q5`` and ``wide`` of tangent_operator_util.TILING_SHAPES: A = 4 with tiles of 20 and 12 cells, and A*D = 66 columns."""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_test_device_solve  # noqa: E402
from cube_tension_matrix_free_multilevel import matrix_free_multilevel_loop  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import gradient, jit, matrix, multilevel, solver  # noqa: E402
from fenics_constitutive_amd import tangent_operator as to  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402
from fe_gpu_util import CANARY, MARGIN, bits, guarded, assert_margins_intact, assert_same_bits, solve_guarded, assert_same_result  # noqa: E402
from fe_gpu_util import tables_of, force_of, status_of, cube_system_of  # noqa: E402
from fe_gpu_util import one_cu  # noqa: E402, F401 (the fixture: pytest finds it in this namespace)
from force_util import MANDEL_DIM, cell_counts  # noqa: E402
import multilevel_free_util as MF  # noqa: E402
import multilevel_util as MU  # noqa: E402
from solver_util import SEG, from_format, spd_tangent  # noqa: E402
from tangent_operator_util import TILING_SHAPES as SHAPES  # noqa: E402
from tangent_operator_util import distinct_inputs, operator_solve, random_mask  # noqa: E402

ML_SHAPES = ("hex8", "tet_p2", "tri_p2", "interval")
CYCLES = ("multiplicative", "additive")
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
SINGULAR = solver.STATUSES.index("singular_block")


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. setup: the values of every coarse level and the nodes' own blocks
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "per_point"])
@pytest.mark.parametrize("shape", ML_SHAPES + ("q3", "q5", "wide"))
def test_setup_on_the_bits(shape, affine):
    d_, a_, q_, _ = SHAPES[shape]
    cw = matrix.cells_per_tile(d_, a_)
    tile = cw * (a_ * d_) ** 2 * 8
    deepest = 0
    for n_cells in cell_counts(cw, q_):
        t = distinct_inputs(shape, n_cells, 3 + n_cells, False, affine)  # (node ``lonely`` is in no cell and not constrained)
        f = force_of(t)
        tangent = to_device(t["tangent"], "cuda")
        agg = fc.MultilevelPreconditioner(fc.TangentOperator(f), coarsest_nodes=1).aggregates(0)
        # random constrained dofs, every dof of a cell's nodes, every dof of the members of aggregate 0
        held = random_mask(t, d_, n_cells, whole_cell=n_cells // 2) | np.repeat(agg == 0, d_)
        for mask in (None, held):
            o = MF.FreeOracle(*tables_of(t), mask=mask, coarsest_nodes=1).setup(t["tangent"])
            assert o.singular  # the unused node's own block is zero
            for scratch in (tile, 2 * tile + 8, None):  # one tile of element matrices, two, everything
                what = f"{shape} affine={affine} cells={n_cells} scratch={scratch} mask={'yes' if mask is not None else 'no'}"
                a = fc.TangentOperator(f, scratch_bytes=scratch)
                a.set_constrained(mask)
                pc = fc.MultilevelPreconditioner(a, coarsest_nodes=1)
                assert len(pc._seam.chunks()) == {tile: -(-n_cells // cw), 2 * tile + 8: -(-n_cells // (2 * cw)), None: 1}[scratch], what
                coarse = pc.setup(tangent)
                assert status_of(pc) == SINGULAR, what
                assert len(coarse) == len(o.levels) - 1 == len(pc.levels) - 1, what
                for l, have in enumerate(coarse, 1):
                    assert have.numel() == d_ * d_ * pc.levels[l]["blocks"]
                    assert_same_bits(to_host(have), o.values[l], f"{what} level {l}")
                assert_same_bits(to_host(pc._on[a.device].blocks), o.diagonal, f"{what}: the nodes' own blocks")
                if mask is not None and coarse:  # the aggregate whose dofs are all constrained: its coarse diagonal block counts its members
                    own = to_host(coarse[0]).reshape(-1, d_, d_)[int(pc.diag_block(1)[0])]
                    assert np.array_equal(own, float((agg == 0).sum()) * np.eye(d_)), what
                deepest = max(deepest, len(pc.levels))
            assert_same_bits(to_host(pc.setup(tangent)[0]), o.values[1], f"{what}: a second setup")
    assert deepest >= 2
    assert_same_bits(to_host(tangent), t["tangent"], "the tangent was written")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. one application
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_cube():
    """the tension-test operator of Cube(5, 4, 3) (120 nodes) on a random positive definite tangent; the scratch holds 16 of the 60
    element matrices"""
    return cube_system_of(FE.Cube(5, 4, 3), 1, scratch_bytes=16 * 576 * 8)


def check_apply(a, tables, tangent, mask, r, what, **options):
    n = a.shape[0]
    pc = fc.MultilevelPreconditioner(a, **options)
    buf, out = guarded(n)
    tangent_dev = to_device(tangent, "cuda")
    got = pc.apply(tangent_dev, to_device(r, "cuda"), out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert_margins_intact(buf, n)
    o = MF.FreeOracle(*tables, mask=mask, **options).setup(tangent)
    assert [lv["nodes"] for lv in pc.levels] == [lv.indptr.size - 1 for lv in o.levels]
    have = to_host(out)
    assert_same_bits(have, o.apply(r), what)
    assert np.isfinite(have).all() and np.abs(have).max() > 0 and status_of(pc) == 0
    return pc, o, tangent_dev, have


@pytest.mark.parametrize("cycle", CYCLES)
def test_apply_on_the_bits(cycle, small_cube):
    f, tables, mask, a, tangent = small_cube
    assert len(fc.MultilevelPreconditioner(a, coarsest_nodes=1)._seam.chunks()) == 4
    rng = np.random.default_rng(8)
    r = np.where(mask, 0.0, rng.normal(size=a.shape[0]))
    for coarsest, depth in ((3000, 1), (20, 2), (1, 3)):
        for smoothing in (1, 2):
            what = f"{cycle} levels={depth} smoothing={smoothing}"
            pc, o, tangent_dev, have = check_apply(a, tables, tangent, mask, r, what, cycle=cycle, smoothing=smoothing, coarsest_nodes=coarsest)
            assert len(pc.levels) == depth, what
            assert (bits(have[mask]) == 0).all(), what  # +0.0 at the constrained dofs
            # a second right-hand side in the same tensors: the cached plan; and one that is not zero at the constrained dofs, without out
            r_dev = to_device(r, "cuda")
            buf, out = guarded(r.size)
            pc.apply(tangent_dev, r_dev, out=out)
            plans = dict(pc._on[a.device].plans)
            second = rng.normal(size=r.size)
            r_dev.copy_(to_device(second, "cuda"))
            pc.apply(tangent_dev, r_dev, out=out)
            torch.cuda.synchronize()
            assert_margins_intact(buf, r.size)
            assert list(pc._on[a.device].plans.values())[-1] is list(plans.values())[-1], what  # the same launch list, replayed
            assert_same_bits(to_host(out), o.apply(second), f"{what}: a second right-hand side through the cached plan")
            assert_same_bits(to_host(pc.apply(tangent_dev, r_dev)), to_host(out), f"{what}: without out")


@pytest.fixture(scope="module")
def big_cube():
    """the tension-test operator of a cube of 32^3 hexahedra (35 937 nodes: 36 segments, more than two trips of the 16 blocks a single
    compute unit is capped at; levels 35937, 1331, 64); the scratch of 64 MiB holds 14 562 of the 32 768 element matrices: three chunks"""
    mesh = FE.Cube(32, 32, 32)
    f, tables, mask, a, tangent = cube_system_of(mesh, 2, scratch_bytes=64 * 1024 * 1024)
    assert -(-mesh.n_dofs // SEG) > 2 * gradient.BLOCKS_PER_CU
    import copy

    first = MF.FreeOracle(*tables, mask=mask, cycle=CYCLES[0]).setup(tangent)
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
    pc = fc.MultilevelPreconditioner(a, cycle=cycle)
    assert len(pc._seam.chunks()) == 3
    tangent_dev = to_device(tangent, "cuda")
    buf, out = guarded(n)
    del one_cu[:]
    pc.apply(tangent_dev, to_device(r, "cuda"), out=out)
    torch.cuda.synchronize()
    assert_margins_intact(buf, n)
    for l in (1, 2):
        assert_same_bits(to_host(pc._on[a.device].values[l])[: o.values[l].size], o.values[l], f"cube 32 level {l}, one compute unit")
    assert_same_bits(to_host(out), o.apply(r), f"cube 32 {cycle}, one compute unit")
    assert max(nb for _, nb in one_cu) == gradient.BLOCKS_PER_CU  # the launches really were capped
    capped = {name for name, nb in one_cu if nb == gradient.BLOCKS_PER_CU}
    assert {multilevel.FREE_GALERKIN_KERNEL, matrix.ELEMENT_KERNEL, multilevel.GALERKIN_KERNEL, multilevel.SMOOTH_KERNEL, multilevel.PROLONG_KERNEL,
            multilevel.RESTRICT_KERNEL, solver.INVERSE_KERNEL, to.DIAGONAL_ELEMENT_KERNEL, to.DIAGONAL_NODE_KERNEL} <= capped
    assert ({to.ELEMENT_KERNEL, to.NODE_KERNEL} <= capped) == (cycle == "multiplicative")  # level-0 products: the operator's two launches
    assert sum(name == multilevel.FREE_GALERKIN_KERNEL for name, _ in one_cu) == 3  # one gather per chunk
    # two iterations of the whole solve under the cap
    del one_cu[:]
    res, x = solve_guarded(fc.ConjugateGradient(a, preconditioner=pc, rtol=0.0, maxiter=2, check_every=2), tangent_dev, r)
    assert_same_result(res, x, MF.conjugate_gradient(o, tangent, r, rtol=0.0, maxiter=2, setup=False), f"cube 32 {cycle}, two iterations on one compute unit")
    assert (multilevel.CLOSE_KERNEL, gradient.BLOCKS_PER_CU) in one_cu


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. exactly k iterations
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ML_SHAPES)
def test_exactly_k_iterations(shape):
    d_, a_, q_, affine = SHAPES[shape]
    n_cells = -(-257 // q_)
    t = distinct_inputs(shape, n_cells, 21, False, affine, every_node=True)
    a = fc.TangentOperator(force_of(t))
    mask = random_mask(t, d_, 26)
    a.set_constrained(mask)
    tangent = spd_tangent(n_cells * q_, MANDEL_DIM[d_], 21, False)
    rng = np.random.default_rng(4)
    b = np.where(mask, 0.0, rng.normal(size=a.shape[0]))
    start = rng.normal(size=a.shape[0])
    for cycle in CYCLES:
        pc = fc.MultilevelPreconditioner(a, cycle=cycle, coarsest_nodes=4)
        o = MF.FreeOracle(*tables_of(t), mask=mask, cycle=cycle, coarsest_nodes=4)
        assert len(pc.levels) >= 2
        for its in (1, 2, 7):
            cg = fc.ConjugateGradient(a, preconditioner=pc, rtol=0.0, maxiter=its)
            for x0 in (None, start):
                what = f"{shape} {cycle} k={its} x0={'yes' if x0 is not None else 'no'}"
                want = MF.conjugate_gradient(o, tangent, b, x0=x0, rtol=0.0, maxiter=its)
                res, x = solve_guarded(cg, tangent, b, x0)
                assert want.status == "maxiter" and want.iterations == its, what
                assert_same_result(res, x, want, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. a cube with two segments: check_every, the statuses, the other routes next to it
# ---------------------------------------------------------------------------------------------------------------------------------
KWS = ((("rtol", 0.0), ("maxiter", 11)), (("rtol", 1e-6),))


@pytest.fixture(scope="module")
def cube_system():
    """the tension-test operator of a 10 x 10 x 9 cube (3630 dofs: two segments; levels 1210, 48, 4 at coarsest_nodes=32), its
    right-hand side and the oracle's solves"""
    mesh = FE.Cube(10, 10, 9)
    f, tables, mask, a, tangent = cube_system_of(mesh, 1)
    assert SEG < mesh.n_dofs <= 2 * SEG
    b = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mesh.n_dofs))
    oracle = {(cycle, kw): MF.conjugate_gradient(MF.FreeOracle(*tables, mask=mask, cycle=cycle, coarsest_nodes=32), tangent, b, **dict(kw))
              for cycle in CYCLES for kw in KWS}
    oracle["block_jacobi"] = operator_solve(tangent, b, *tables, mask=mask, rtol=1e-6)
    return mesh, f, tables, mask, a, tangent, b, oracle


@pytest.mark.parametrize("cycle", CYCLES)
def test_check_every_changes_nothing(cycle, cube_system):
    mesh, f, tables, mask, a, tangent, b, oracle = cube_system
    pc = fc.MultilevelPreconditioner(a, cycle=cycle, coarsest_nodes=32)
    assert len(pc.levels) == 3
    jacobi = oracle["block_jacobi"]
    for kw in KWS:
        want = oracle[(cycle, kw)]
        assert want.status == ("maxiter" if "maxiter" in dict(kw) else "converged") and want.iterations >= 11
        for every in (1, 3, 16):  # (11 iterations end in the middle of a batch of 3 and of 16)
            res, x = solve_guarded(fc.ConjugateGradient(a, preconditioner=pc, check_every=every, **dict(kw)), tangent, b)
            assert_same_result(res, x, want, f"{cycle} {dict(kw)} check_every={every}")
            assert res.looks == 1 + -(-want.iterations // every)
    print(f"Cube(10, 10, 9), operator: block-Jacobi {jacobi.iterations} iterations, multilevel {cycle} {want.iterations}")
    assert want.iterations < jacobi.iterations


def test_statuses(cube_system):
    mesh, f, tables, mask, a, tangent, b, oracle = cube_system
    n = b.size
    start = np.random.default_rng(2).normal(size=n)
    for cycle in CYCLES:
        pc = fc.MultilevelPreconditioner(a, cycle=cycle, coarsest_nodes=32)
        cg = fc.ConjugateGradient(a, preconditioner=pc, rtol=1e-6)
        # an all-zero tangent: every free node's own block is zero -- no iteration, x is x0
        res, x = solve_guarded(cg, np.zeros_like(tangent), b, start)
        assert (res.status, res.iterations, res.converged, res.looks) == ("singular_block", 0, False, 1)
        assert_same_bits(x, start, f"{cycle}: singular block")
        # b = 0: converged at once
        res, x = solve_guarded(cg, tangent, np.zeros(n))
        assert (res.status, res.iterations, res.converged, res.residual_norm, res.looks) == ("converged", 0, True, 0.0, 1)
        assert (bits(x) == 0).all()
        # a negated tangent: the cycle gives r . z < 0 at the start: indefinite, x is x0 (the oracle says the same)
        want = MF.conjugate_gradient(MF.FreeOracle(*tables, mask=mask, cycle=cycle, coarsest_nodes=32), -tangent, b, x0=start, rtol=1e-6)
        res, x = solve_guarded(cg, -tangent, b, start)
        assert want.status == "indefinite" and want.iterations == 0
        assert_same_result(res, x, want, f"{cycle}: indefinite")
        assert_same_bits(x, start, f"{cycle}: indefinite")
        # a right-hand side that is not finite
        bad = b.copy()
        bad[17] = np.nan
        res, x = solve_guarded(cg, tangent, bad)
        assert res.status == "nonfinite" and res.iterations == 0
        res, x = solve_guarded(fc.ConjugateGradient(a, preconditioner=pc, maxiter=0), tangent, b, start)
        assert (res.status, res.iterations, res.looks) == ("maxiter", 0, 1)
        assert_same_bits(x, start, f"{cycle}: maxiter 0")
        # and the object solves again afterwards
        res, x = solve_guarded(cg, tangent, b)
        assert_same_result(res, x, oracle[(cycle, KWS[1])], f"{cycle}: after the statuses")


@pytest.mark.parametrize("cycle", CYCLES)
def test_a_second_solver_for_the_same_preconditioner(cycle, cube_system):
    """A solver is dropped and another built for the same preconditioner: its control block and partial sums lie elsewhere (the first
    solver's are kept allocated here, filled with ones -- a status that is not "running"), so the cached launch plan must not be
    replayed on the old pointers.  The second solve gives the oracle's bits, and the first solver's control block is not touched."""
    import gc

    mesh, f, tables, mask, a, tangent, b, oracle = cube_system
    pc = fc.MultilevelPreconditioner(a, cycle=cycle, coarsest_nodes=32)
    tangent_dev = to_device(tangent, "cuda")
    first = fc.ConjugateGradient(a, preconditioner=pc, **dict(KWS[1]))
    res, x = solve_guarded(first, tangent_dev, b)
    assert_same_result(res, x, oracle[(cycle, KWS[1])], f"{cycle}: the first solver")
    control = first._work[a.device][0]
    held = (control.device_block, control.partials)
    old = tuple(t.data_ptr() for t in held)
    del first, control, res
    gc.collect()
    for t in held:
        t.fill_(1.0)
    shift = [torch.zeros(n, dtype=torch.float64, device="cuda") for n in (1, 12, 3, 64)]
    second = fc.ConjugateGradient(a, preconditioner=pc, **dict(KWS[1]))
    res, x = solve_guarded(second, tangent_dev, b)
    new = second._work[a.device][0]
    assert new.device_block.data_ptr() != old[0] and new.partials.data_ptr() != old[1]
    assert_same_result(res, x, oracle[(cycle, KWS[1])], f"{cycle}: the second solver")
    assert all((to_host(t) == 1.0).all() for t in held) and all((to_host(t) == 0.0).all() for t in shift)
    # the standalone application (the preconditioner's own control block) and the solver again, one after the other
    r = to_device(b, "cuda")
    z = to_host(pc.apply(tangent_dev, r))
    res, x = solve_guarded(second, tangent_dev, b)
    assert_same_result(res, x, oracle[(cycle, KWS[1])], f"{cycle}: behind apply")
    assert_same_bits(to_host(pc.apply(tangent_dev, r)), z, f"{cycle}: apply behind the solve")


def test_the_other_routes_keep_their_bits_next_to_it(cube_system):
    """in the process that has run the operator's multilevel solves: ConjugateGradient(K, preconditioner=MultilevelPreconditioner(K))
    and ConjugateGradient(A) with block-Jacobi, each on its own oracle's bits"""
    mesh, f, tables, mask, a, tangent, b, oracle = cube_system
    tangent_dev = to_device(tangent, "cuda")
    for cycle in CYCLES:
        free, _ = solve_guarded(fc.ConjugateGradient(a, preconditioner=fc.MultilevelPreconditioner(a, cycle=cycle, coarsest_nodes=32), rtol=0.0, maxiter=7),
                                tangent_dev, b)
        k = fc.TangentMatrix(f)
        k.set_constrained(mask)
        values = k(tangent_dev)
        blocks = from_format("bsr", k.indptr, k.indices, to_host(values), 3)
        buf, out = guarded(b.size)
        res = fc.ConjugateGradient(k, preconditioner=fc.MultilevelPreconditioner(k, cycle=cycle, coarsest_nodes=32), rtol=0.0, maxiter=7)(
            values, to_device(b, "cuda"), out=out)
        assert_margins_intact(buf, b.size)
        want = MU.conjugate_gradient(MU.Oracle(k.indptr, k.indices, cycle=cycle, coarsest_nodes=32, mask=mask), blocks, b, rtol=0.0, maxiter=7)
        assert_same_result(res, to_host(out), want, f"ConjugateGradient(K, multilevel {cycle})")
        assert np.allclose(to_host(out), to_host(free.x), rtol=1e-7, atol=1e-10 * np.abs(want.x).max())  # one preconditioner, to rounding
    res, x = solve_guarded(fc.ConjugateGradient(a, rtol=1e-6), tangent_dev, b)
    assert_same_result(res, x, oracle["block_jacobi"], "ConjugateGradient(A), block-Jacobi")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. refusals come before any launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(cube_system, small_cube):
    mesh, f, tables, mask, a, tangent, b, oracle = cube_system
    n, nt = a.shape[0], tangent.size
    pc = fc.MultilevelPreconditioner(a, coarsest_nodes=32)
    cg = fc.ConjugateGradient(a, preconditioner=pc)
    tangent_dev, b_dev = to_device(tangent, "cuda"), to_device(b, "cuda")
    assert cg(tangent_dev, b_dev).converged  # tables uploaded, kernels loaded: what follows can only add launches
    other = fc.MultilevelPreconditioner(small_cube[3], coarsest_nodes=8)
    fresh = fc.MultilevelPreconditioner(a, coarsest_nodes=32)
    buf, out = guarded(n)
    spare = torch.zeros(2 * max(n, nt) + 2, dtype=torch.float64, device="cuda")
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        with pytest.raises(ValueError, match="multilevel"):
            fc.ConjugateGradient(a, preconditioner=other)  # built on another operator
        with pytest.raises(ValueError, match="multilevel"):
            fc.ConjugateGradient(a, preconditioner="multilevel")
        with pytest.raises(ValueError, match="multilevel"):
            fc.ConjugateGradient(a, preconditioner=fc.MultilevelPreconditioner(fc.TangentMatrix(f)))
        with pytest.raises(ValueError, match="scratch_bytes"):
            fc.MultilevelPreconditioner(fc.TangentOperator(f, scratch_bytes=2 * 576 * 8 - 8))
        for call in (lambda **kw: fresh.apply(kw["tangent"], kw["v"], out=kw["out"]), lambda **kw: cg(kw["tangent"], kw["v"], out=kw["out"])):
            ok = dict(tangent=tangent_dev, v=b_dev, out=out)
            with pytest.raises(ValueError, match="aligned"):
                call(**{**ok, "out": buf[MARGIN + 1: MARGIN + 1 + n]})
            with pytest.raises(ValueError, match="entries"):
                call(**{**ok, "out": buf[MARGIN: MARGIN + n - 3]})
            with pytest.raises(ValueError, match="contiguous"):
                call(**{**ok, "out": spare[: 2 * n: 2]})
            with pytest.raises(TypeError):
                call(**{**ok, "out": out.float()})
            with pytest.raises(ValueError, match="alias"):
                call(**{**ok, "out": b_dev})
            with pytest.raises(ValueError, match="entries"):
                call(**{**ok, "tangent": tangent_dev[:-36]})
            with pytest.raises(ValueError, match="aligned"):
                call(**{**ok, "tangent": spare[1: 1 + nt]})
            with pytest.raises(ValueError, match="entries"):
                call(**{**ok, "v": b_dev[:-3]})
            with pytest.raises(TypeError):
                call(**{**ok, "v": b})
        with pytest.raises(ValueError, match="entries"):
            fresh.setup(tangent_dev[:-36])
        with pytest.raises(TypeError):
            fresh.setup(tangent)
    finally:
        jit.launch = real
    torch.cuda.synchronize()
    assert launches == [] and not fresh._on
    assert (bits(to_host(buf)) == CANARY).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the Newton loop of the example
# ---------------------------------------------------------------------------------------------------------------------------------
def test_in_the_loop_of_the_example():
    """The tension test of examples/cube_tension_matrix_free_multilevel.py on Cube(3, 2, 4), eight load steps, both cycles, against
    ``fe_mini.tension_test`` on the CPU with the oracle law and SciPy's direct solver: the direct solve's Newton counts, the largest
    relative reaction difference at most 1e-8, and no matrix anywhere in the loop."""
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    cpu = FE.CopyProtocolState(FE.OracleLaw(O.von_mises_3d, VM_P, {"eps_n": 6, "alpha": 1}), mesh.n_points)
    r_direct, norms_direct, _ = FE.tension_test(mesh, cpu, steps=8)
    for cycle in CYCLES:
        loop = matrix_free_multilevel_loop(mesh, fc.VonMises3D(VM_P), cycle, coarsest_nodes=8)
        assert len(loop.cg.preconditioner.levels) == 2 and loop.cg.preconditioner.K is loop.K
        r_gpu, norms_gpu, u, solves = tension_test_device_solve(mesh, loop, steps=8)  # (raises where a solve or a load step does not converge)
        difference = np.max(np.abs(r_gpu - r_direct)) / np.max(np.abs(r_direct))
        counts = [len(h) for h in norms_gpu]
        print(f"matrix-free multilevel tension test, {cycle}: GPU against direct {difference:.3e}, Newton iterations {counts}, conjugate-gradient iterations {solves}")
        assert counts == [len(h) for h in norms_direct] == [2, 2, 2, 3, 3, 4, 5, 5]
        assert difference <= 1e-8, difference
        assert not any(isinstance(x, fc.TangentMatrix) for x in vars(loop).values())
