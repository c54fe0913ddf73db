"""The multilevel preconditioner on the GPU (fenics_constitutive_amd.MultilevelPreconditioner, csrc/jit/multilevel.hip): the Galerkin
values of every level, one application of both cycles and whole conjugate-gradient runs compared ON THE BITS with the NumPy oracle
of multilevel_util.py -- in both formats of K, on hierarchies of one, two and three levels, under a grid capped at one compute
unit, for every ``check_every`` --, the statuses and refusals, block-Jacobi untouched behind it, and the Newton loop of
examples/cube_tension_multilevel.py."""

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
from cube_tension_multilevel import multilevel_loop  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import gradient, jit, multilevel, solver  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402
from fe_gpu_util import CANARY, MARGIN, bits, guarded, assert_margins_intact, assert_same_bits, solve_guarded, assert_same_result  # noqa: E402
from fe_gpu_util import one_cu  # noqa: E402, F401 (the fixture: pytest finds it in this namespace)
from force_util import MANDEL_DIM, random_inputs  # noqa: E402
from gradient_util import SHAPES  # noqa: E402
import multilevel_util as MU  # noqa: E402
from solver_util import SEG, conjugate_gradient, from_format, full_pattern, spd_tangent  # noqa: E402

FORMATS = ("bsr", "csr")
ML_SHAPES = ("hex8", "tet_p2", "tri_p2", "interval")
CYCLES = ("multiplicative", "additive")
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}


def assembled(shape, n_cells, seed, fmt, fraction=0.2):
    """(K, values on the device, blocks on the host, mask): an assembled matrix of random tables in which every node has a block of
    its own (the nodes no cell touches: rows of one block at the end of the pattern, constrained), with random constrained dofs and
    all dofs of the members of aggregate 0 constrained"""
    d_, a_, q_, affine = SHAPES[shape]
    t = random_inputs(shape, n_cells, seed, False, affine)
    f = fc.InternalForce(fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"]), t["weights"])
    pat, unused = full_pattern(t["dofmap"], t["n_nodes"])
    k = fc.TangentMatrix(f, format=fmt, pattern_dofmap=pat)
    used = np.ones(t["n_nodes"], dtype=bool)
    used[unused] = False
    mask = ((np.random.default_rng(seed + 5).random(d_ * t["n_nodes"]) < fraction) & np.repeat(used, d_)) | np.repeat(~used, d_)
    agg, _ = multilevel.aggregate(k.indptr, k.indices)
    mask |= np.repeat(agg == 0, d_)
    k.set_constrained(mask)
    values = k(to_device(spd_tangent(n_cells * q_, MANDEL_DIM[d_], seed, False), "cuda"))
    torch.cuda.synchronize()
    return k, values, from_format(fmt, k.indptr, k.indices, to_host(values), d_), mask


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. setup: the Galerkin values of every level
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", ML_SHAPES)
def test_setup_on_the_bits(shape, fmt):
    d_, a_, q_, _ = SHAPES[shape]
    deepest = 0
    for n_cells in (1, 5, -(-257 // q_)):
        k, values, blocks, mask = assembled(shape, n_cells, 3 + n_cells, fmt)
        pc = fc.MultilevelPreconditioner(k, coarsest_nodes=1)
        coarse = pc.setup(values)
        torch.cuda.synchronize()
        o = MU.Oracle(k.indptr, k.indices, coarsest_nodes=1, mask=mask).setup(blocks)
        assert len(coarse) == len(o.levels) - 1 == len(pc.levels) - 1
        for l, have in enumerate(coarse, 1):
            assert have.numel() == d_ * d_ * pc.levels[l]["blocks"]
            assert_same_bits(to_host(have), o.values[l], f"{shape} {fmt} cells={n_cells} level {l}")
        # the aggregate whose dofs are all constrained: its coarse diagonal block counts its members
        if coarse:
            own = to_host(coarse[0]).reshape(-1, d_, d_)[int(pc.diag_block(1)[0])]
            assert np.array_equal(own, float((pc.aggregates(0) == 0).sum()) * np.eye(d_))
        deepest = max(deepest, len(pc.levels))
    assert deepest >= 3


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. one application
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_cube():
    """the tension-test matrix of Cube(5, 4, 3) (120 nodes) in both formats"""
    mesh = FE.Cube(5, 4, 3)
    op, f = cube_operators(mesh)
    mask, _ = tension_constraints(mesh)
    tangent = to_device(spd_tangent(mesh.n_points, 6, 1, False), "cuda")
    out = {}
    for fmt in FORMATS:
        k = fc.TangentMatrix(f, format=fmt)
        k.set_constrained(mask)
        values = k(tangent)
        torch.cuda.synchronize()
        out[fmt] = (k, values, from_format(fmt, k.indptr, k.indices, to_host(values), 3))
    assert_same_bits(out["bsr"][2], out["csr"][2], "the two formats hold one matrix")
    return mesh, mask, out


def check_apply(k, values, blocks, mask, r, what, **options):
    n = k.shape[0]
    pc = fc.MultilevelPreconditioner(k, **options)
    buf, out = guarded(n)
    got = pc.apply(values, to_device(r, "cuda"), out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert_margins_intact(buf, n)
    o = MU.Oracle(k.indptr, k.indices, mask=mask, **options).setup(blocks)
    assert [lv["nodes"] for lv in pc.levels] == [lv.indptr.size - 1 for lv in o.levels]
    have = to_host(out)
    assert_same_bits(have, o.apply(r), what)
    assert np.isfinite(have).all() and np.abs(have).max() > 0
    return pc, have


@pytest.mark.parametrize("cycle", CYCLES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_apply_on_the_bits(fmt, cycle, small_cube):
    mesh, mask, systems = small_cube
    k, values, blocks = systems[fmt]
    r = np.where(mask, 0.0, np.random.default_rng(8).normal(size=k.shape[0]))
    for coarsest, depth in ((3000, 1), (20, 2), (1, 3)):
        for smoothing in (1, 2):
            for sweeps in (1, 8):
                what = f"{fmt} {cycle} levels={depth} smoothing={smoothing} coarsest_sweeps={sweeps}"
                pc, have = check_apply(k, values, blocks, mask, r, what, cycle=cycle, smoothing=smoothing, coarsest_nodes=coarsest, coarsest_sweeps=sweeps)
                assert len(pc.levels) == depth, what
                assert (bits(have[mask]) == 0).all(), what  # +0.0 at the constrained dofs
    # a right-hand side that is not zero at the constrained dofs, and without out
    r = np.random.default_rng(9).normal(size=k.shape[0])
    pc, have = check_apply(k, values, blocks, mask, r, f"{fmt} {cycle}: any r", cycle=cycle, coarsest_nodes=1)
    assert_same_bits(to_host(pc.apply(values, to_device(r, "cuda"))), have, f"{fmt} {cycle}: without out")


@pytest.fixture(scope="module")
def big_cube():
    """the tension-test matrix of a cube of 32^3 hexahedra (35 937 nodes: 36 segments, more than two trips of the 16 blocks a single
    compute unit is capped at; levels 35937, 1331, 64), scalar CSR"""
    mesh = FE.Cube(32, 32, 32)
    op, f = cube_operators(mesh)
    assert -(-mesh.n_dofs // SEG) > 2 * gradient.BLOCKS_PER_CU
    k = fc.TangentMatrix(f, format="csr")
    mask, _ = tension_constraints(mesh)
    k.set_constrained(mask)
    values = k(to_device(spd_tangent(mesh.n_points, 6, 2, False), "cuda"))
    torch.cuda.synchronize()
    blocks = from_format("csr", k.indptr, k.indices, to_host(values), 3)
    oracles = {cycle: MU.Oracle(k.indptr, k.indices, cycle=cycle, mask=mask).setup(blocks) for cycle in CYCLES}
    return mesh, mask, k, values, blocks, oracles


@pytest.mark.parametrize("cycle", CYCLES)
def test_apply_on_one_compute_unit(cycle, big_cube, one_cu):
    mesh, mask, k, values, blocks, oracles = big_cube
    o = oracles[cycle]
    assert [lv.indptr.size - 1 for lv in o.levels] == [35937, 1331, 64]
    r = np.where(mask, 0.0, np.random.default_rng(3).normal(size=k.shape[0]))
    n = k.shape[0]
    pc = fc.MultilevelPreconditioner(k, cycle=cycle)
    buf, out = guarded(n)
    del one_cu[:]
    pc.apply(values, to_device(r, "cuda"), out=out)
    torch.cuda.synchronize()
    assert_margins_intact(buf, n)
    assert_same_bits(to_host(out), o.apply(r), f"cube 32 {cycle}, one compute unit")
    assert max(nb for _, nb in one_cu) == gradient.BLOCKS_PER_CU  # the launches really were capped
    capped = {name for name, nb in one_cu if nb == gradient.BLOCKS_PER_CU}
    assert {multilevel.GALERKIN_KERNEL, multilevel.SMOOTH_KERNEL, multilevel.PROLONG_KERNEL, multilevel.RESTRICT_KERNEL, solver.INVERSE_KERNEL} <= capped
    assert (solver.MATVEC_KERNEL in capped) == (cycle == "multiplicative")
    # two iterations of the whole solve under the cap: the closing kernel's grid-stride loop makes more than two trips
    del one_cu[:]
    res, x = solve_guarded(fc.ConjugateGradient(k, preconditioner=pc, rtol=0.0, maxiter=2, check_every=2), values, r)
    assert_same_result(res, x, MU.conjugate_gradient(o, blocks, r, rtol=0.0, maxiter=2), f"cube 32 {cycle}, two iterations on one compute unit")
    assert (multilevel.CLOSE_KERNEL, gradient.BLOCKS_PER_CU) in one_cu


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. exactly k iterations
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", ML_SHAPES)
def test_exactly_k_iterations(shape, fmt):
    d_, a_, q_, _ = SHAPES[shape]
    k, values, blocks, mask = assembled(shape, -(-257 // q_), 21, fmt)
    rng = np.random.default_rng(4)
    b = np.where(mask, 0.0, rng.normal(size=k.shape[0]))
    start = rng.normal(size=k.shape[0])
    for cycle in CYCLES:
        pc = fc.MultilevelPreconditioner(k, cycle=cycle, coarsest_nodes=4)
        o = MU.Oracle(k.indptr, k.indices, cycle=cycle, coarsest_nodes=4, mask=mask)
        assert len(pc.levels) >= 3
        for its in (1, 2, 7):
            cg = fc.ConjugateGradient(k, preconditioner=pc, rtol=0.0, maxiter=its)
            for x0 in (None, start):
                what = f"{shape} {fmt} {cycle} k={its} x0={'yes' if x0 is not None else 'no'}"
                want = MU.conjugate_gradient(o, blocks, b, x0=x0, rtol=0.0, maxiter=its)
                res, x = solve_guarded(cg, values, b, x0)
                assert want.status == "maxiter" and want.iterations == its, what
                assert_same_result(res, x, want, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. a cube with two segments: check_every, the statuses, block-Jacobi behind it
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cube_system():
    """the tension-test matrix of a cube of 10^3 hexahedra (3993 dofs: two segments; levels 1331, 64, 8), its right-hand side and the
    oracle solves"""
    mesh = FE.Cube(10, 10, 10)
    op, f = cube_operators(mesh)
    mask, top = tension_constraints(mesh)
    assert SEG < mesh.n_dofs <= 2 * SEG
    tangent = spd_tangent(mesh.n_points, 6, 1, False)
    b = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mesh.n_dofs))
    out = {}
    for fmt in FORMATS:
        k = fc.TangentMatrix(f, format=fmt)
        k.set_constrained(mask)
        values = k(to_device(tangent, "cuda"))
        torch.cuda.synchronize()
        out[fmt] = (k, values, from_format(fmt, k.indptr, k.indices, to_host(values), 3))
    k, _, blocks = out["bsr"]
    oracle = {(cycle, kw): MU.conjugate_gradient(MU.Oracle(k.indptr, k.indices, cycle=cycle, coarsest_nodes=32, mask=mask), blocks, b, **dict(kw))
              for cycle in CYCLES for kw in ((("rtol", 0.0), ("maxiter", 11)), (("rtol", 1e-6),))}
    return mesh, mask, b, out, oracle


@pytest.mark.parametrize("cycle", CYCLES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_check_every_changes_nothing(fmt, cycle, cube_system):
    mesh, mask, b, systems, oracle = cube_system
    k, values, blocks = systems[fmt]
    pc = fc.MultilevelPreconditioner(k, cycle=cycle, coarsest_nodes=32)
    assert [lv["nodes"] for lv in pc.levels] == [1331, 64, 8]
    for kw in ((("rtol", 0.0), ("maxiter", 11)), (("rtol", 1e-6),)):
        want = oracle[(cycle, kw)]
        assert want.status == ("maxiter" if "maxiter" in dict(kw) else "converged") and want.iterations >= 11
        for every in (1, 3, 16):
            res, x = solve_guarded(fc.ConjugateGradient(k, preconditioner=pc, check_every=every, **dict(kw)), values, b)
            assert_same_result(res, x, want, f"{fmt} {cycle} {dict(kw)} check_every={every}")
            assert res.looks == 1 + -(-want.iterations // every)
    jacobi = conjugate_gradient(k.indptr, k.indices, blocks, b, rtol=1e-6)
    assert oracle[(cycle, (("rtol", 1e-6),))].iterations < jacobi.iterations


def test_statuses_and_block_jacobi_behind_it(cube_system):
    mesh, mask, b, systems, oracle = cube_system
    k, values, blocks = systems["bsr"]
    n = b.size
    start = np.random.default_rng(2).normal(size=n)
    for cycle in CYCLES:
        cg = fc.ConjugateGradient(k, preconditioner=fc.MultilevelPreconditioner(k, cycle=cycle, coarsest_nodes=32), rtol=1e-6)
        # all-zero values: a singular block, no iteration, x is x0
        res, x = solve_guarded(cg, torch.zeros_like(values), b, start)
        assert (res.status, res.iterations, res.converged, res.looks) == ("singular_block", 0, False, 1)
        assert_same_bits(x, start, f"{cycle}: singular block")
        # b = 0: converged at once
        res, x = solve_guarded(cg, values, np.zeros(n))
        assert (res.status, res.iterations, res.converged, res.residual_norm, res.looks) == ("converged", 0, True, 0.0, 1)
        assert (bits(x) == 0).all()
        # -K: the cycle gives r . z < 0 at the start: indefinite, x is x0 (the oracle says the same)
        want = MU.conjugate_gradient(MU.Oracle(k.indptr, k.indices, cycle=cycle, coarsest_nodes=32, mask=mask), -blocks, b, x0=start, rtol=1e-6)
        res, x = solve_guarded(cg, -values, b, start)
        assert want.status == "indefinite" and want.iterations == 0
        assert_same_result(res, x, want, f"{cycle}: indefinite")
        assert_same_bits(x, start, f"{cycle}: indefinite")
        # and the object solves again afterwards
        res, x = solve_guarded(cg, values, b)
        assert_same_result(res, x, oracle[(cycle, (("rtol", 1e-6),))], f"{cycle}: after the statuses")
    # block-Jacobi and the plain solver, in the same process behind the multilevel solves: their oracle's bits
    for pc in ("block_jacobi", None):
        res, x = solve_guarded(fc.ConjugateGradient(k, preconditioner=pc, rtol=1e-6), values, b)
        assert_same_result(res, x, conjugate_gradient(k.indptr, k.indices, blocks, b, preconditioner=pc, rtol=1e-6), f"{pc} behind multilevel")


@pytest.mark.parametrize("cycle", CYCLES)
def test_a_second_solver_for_the_same_preconditioner(cycle, cube_system):
    """The preconditioner replays the launch list of its last cycle while the device pointers in it stay the same.  A solver is
    dropped and another built for the same preconditioner: its control block and partial sums lie elsewhere (the first solver's
    are kept allocated here, filled with ones -- a status that is not "running" --, and small allocations shift the rest), while the
    Python objects, the values and the vectors may well come back at the old addresses.  The second solve gives the oracle's bits,
    and the first solver's control block is not touched."""
    import gc

    mesh, mask, b, systems, oracle = cube_system
    k, values, blocks = systems["bsr"]
    kw = (("rtol", 1e-6),)
    pc = fc.MultilevelPreconditioner(k, cycle=cycle, coarsest_nodes=32)
    first = fc.ConjugateGradient(k, preconditioner=pc, **dict(kw))
    res, x = solve_guarded(first, values, b)
    assert_same_result(res, x, oracle[(cycle, kw)], f"{cycle}: the first solver")
    control = first._work[k.device][0]
    held = (control.device_block, control.partials)
    old = tuple(t.data_ptr() for t in held)
    del first, control, res
    gc.collect()
    for t in held:
        t.fill_(1.0)
    shift = [torch.zeros(n, dtype=torch.float64, device="cuda") for n in (1, 12, 3, 64)]
    second = fc.ConjugateGradient(k, preconditioner=pc, **dict(kw))
    res, x = solve_guarded(second, values, b)
    new = second._work[k.device][0]
    assert new.device_block.data_ptr() != old[0] and new.partials.data_ptr() != old[1]
    assert_same_result(res, x, oracle[(cycle, kw)], f"{cycle}: the second solver")
    assert all((to_host(t) == 1.0).all() for t in held) and all((to_host(t) == 0.0).all() for t in shift)
    # the standalone application (the preconditioner's own control block) and the solver again, one after the other
    r = to_device(b, "cuda")
    z = to_host(pc.apply(values, r))
    res, x = solve_guarded(second, values, b)
    assert_same_result(res, x, oracle[(cycle, kw)], f"{cycle}: behind apply")
    assert_same_bits(to_host(pc.apply(values, r)), z, f"{cycle}: apply behind the solve")
    with pytest.raises(AttributeError):
        pc.omega = 1.0


def test_an_instance_of_another_matrix_is_refused(cube_system, small_cube):
    mesh, mask, b, systems, oracle = cube_system
    k, values, blocks = systems["bsr"]
    other = small_cube[2]["bsr"][0]
    same_pattern = fc.TangentMatrix(k.force)
    pc = fc.MultilevelPreconditioner(other, coarsest_nodes=8)
    assert fc.ConjugateGradient(k, preconditioner="multilevel")(values, to_device(b, "cuda")).converged  # everything loaded
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        with pytest.raises(ValueError, match="another matrix"):
            fc.ConjugateGradient(k, preconditioner=pc)
        with pytest.raises(ValueError, match="another matrix"):
            fc.ConjugateGradient(same_pattern, preconditioner=fc.MultilevelPreconditioner(k))
        with pytest.raises(ValueError, match="preconditioner"):
            fc.ConjugateGradient(k, preconditioner="amg")
        ml = fc.MultilevelPreconditioner(k)
        buf, out = guarded(b.size)
        with pytest.raises(ValueError, match="entries"):
            ml.apply(values, to_device(b, "cuda")[:-3], out=out)
        with pytest.raises(ValueError, match="entries"):
            ml.setup(values[:-9])
        r = to_device(b, "cuda")
        with pytest.raises(ValueError, match="alias"):
            ml.apply(values, r, out=r)
        with pytest.raises(ValueError, match="aligned"):
            ml.apply(values, r, out=buf[MARGIN + 1: MARGIN + 1 + b.size])
        with pytest.raises(TypeError):
            ml.apply(values, to_host(r), out=out)
    finally:
        jit.launch = real
    torch.cuda.synchronize()
    assert launches == [] and not ml._on
    assert (bits(to_host(buf)) == CANARY).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the Newton loop of the example
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear_elasticity", "von_mises_3d"])
def test_in_the_loop_of_the_example(kind):
    """The tension test of examples/cube_tension_multilevel.py on Cube(3, 2, 4), eight load steps, both cycles, against
    ``fe_mini.tension_test`` on the CPU with the oracle law and SciPy's direct solver: equal Newton counts, and the largest relative
    reaction difference at most 1e-8, the bound cube_tension_device_solve.py asserts."""
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    n = mesh.n_points
    if kind == "von_mises_3d":
        oracle_law, hist, law, params = O.von_mises_3d, {"eps_n": 6, "alpha": 1}, (lambda: fc.VonMises3D(VM_P)), VM_P
    else:
        params = {"E": 42.0, "nu": 0.3}
        oracle_law, hist, law = O.linear_elasticity, None, (lambda: fc.LinearElasticityModel(params, fc.StressStrainConstraint.FULL))
    r_direct, norms_direct, _ = FE.tension_test(mesh, FE.CopyProtocolState(FE.OracleLaw(oracle_law, params, hist), n), steps=8)
    scale = np.max(np.abs(r_direct))
    for cycle in CYCLES:
        loop = multilevel_loop(mesh, law(), cycle, coarsest_nodes=8)
        assert len(loop.cg.preconditioner.levels) == 2
        r_gpu, norms_gpu, u, solves = tension_test_device_solve(mesh, loop, steps=8)  # (raises where a solve or a load step does not converge)
        difference = np.max(np.abs(r_gpu - r_direct)) / scale
        counts = [len(h) for h in norms_gpu]
        print(f"multilevel tension test, {kind} {cycle}: GPU against direct {difference:.3e}, Newton iterations {counts}, conjugate-gradient iterations {solves}")
        assert counts == [len(h) for h in norms_direct]
        if kind == "von_mises_3d":
            assert counts == [2, 2, 2, 3, 3, 4, 5, 5]
        assert difference <= 1e-8, difference
