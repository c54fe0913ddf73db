"""The rigid-body coarse space of the multilevel preconditioner on the GPU (fenics_constitutive_amd.MultilevelPreconditioner with
``coarse_space="rigid_body"``, csrc/jit/multilevel_rigid.hip, the 6 x 6 inverse of conjugate_gradient.hip): the Galerkin values and
block inverses of every level, one application of both cycles and whole runs of ``ConjugateGradient`` and ``BiCGStab`` compared ON THE
BITS with the NumPy oracle of rigid_body_util.py -- in both formats of K, in 2-D (3 x 3 coarse blocks) and 3-D (6 x 6), under a grid
capped at one compute unit, for every ``check_every`` --, ``singular_block`` from the coarse levels, a translation and a rigid-body
instance of one matrix side by side, and the Newton loops of the examples."""

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
from cube_tension_multilevel import VM_P, multilevel_loop  # noqa: E402
from cube_tension_nonsymmetric import DP_P, TOP_DISPLACEMENT, drucker_prager, nonsymmetric_loop  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import gradient, jit, multilevel, solver  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402
from bicgstab_util import bicgstab as oracle_bicgstab  # noqa: E402
from fe_gpu_util import bits, guarded, assert_margins_intact, assert_same_bits, solve_guarded, assert_same_result  # noqa: E402
from fe_gpu_util import one_cu  # noqa: E402, F401 (the fixture: pytest finds it in this namespace)
from force_util import MANDEL_DIM, random_inputs  # noqa: E402
from gradient_util import SHAPES  # noqa: E402
import multilevel_util as MU  # noqa: E402
import rigid_body_util as RU  # noqa: E402
from solver_util import SEG, from_format, spd_tangent  # noqa: E402

FORMATS = ("bsr", "csr")
RIGID_SHAPES = ("hex8", "tet_p2", "tri_p2")
CYCLES = ("multiplicative", "additive")
SINGULAR = solver.STATUSES.index("singular_block")


def assembled(shape, n_cells, seed, fmt, symmetric=False, fraction=0.2):
    """(K, values on the device, blocks on the host, mask, coordinates): the matrix of force_util's UNSYMMETRIC random tangent (or
    a symmetric positive definite one) over random tables, renumbered to the nodes their cells use -- no node is alone --, with
    random constrained dofs and seeded random coordinates"""
    d_, a_, q_, affine = SHAPES[shape]
    t = random_inputs(shape, n_cells, seed, False, affine)
    used, dofmap = np.unique(t["dofmap"], return_inverse=True)
    dofmap, n_nodes = np.ascontiguousarray(dofmap.reshape(t["dofmap"].shape), dtype=np.int32), int(used.size)
    k = fc.TangentMatrix(fc.InternalForce(fc.DisplacementGradient(dofmap, t["ref"], t["jinv"], n_nodes), t["weights"]), format=fmt)
    mask = np.random.default_rng(seed + 5).random(d_ * n_nodes) < fraction
    k.set_constrained(mask)
    tangent = spd_tangent(n_cells * q_, MANDEL_DIM[d_], seed, False) if symmetric else t["tangent"]
    values = k(to_device(tangent, "cuda"))
    torch.cuda.synchronize()
    return k, values, from_format(fmt, k.indptr, k.indices, to_host(values), d_), mask, np.random.default_rng(seed + 77).normal(size=(n_nodes, d_))


def rigid(k, x, **options):
    return fc.MultilevelPreconditioner(k, coarse_space="rigid_body", coordinates=x, **options)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. setup: the Galerkin values and the inverses of every level
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", RIGID_SHAPES)
def test_setup_on_the_bits(shape, fmt):
    d_, a_, q_, _ = SHAPES[shape]
    dc = RU.coarse_dofs(d_)
    deepest = 0
    for n_cells in (1, 5, -(-257 // q_)):
        k, values, blocks, mask, x = assembled(shape, n_cells, 3 + n_cells, fmt)
        pc = rigid(k, x, coarsest_nodes=1)
        assert pc.coarse_dofs == dc
        coarse = pc.setup(values)
        torch.cuda.synchronize()
        o = RU.Oracle(k.indptr, k.indices, x, coarsest_nodes=1, mask=mask).setup(blocks)
        assert len(coarse) == len(o.levels) - 1 == len(pc.levels) - 1 >= 1
        what = f"{shape} {fmt} cells={n_cells}"
        for l, have in enumerate(coarse, 1):
            assert have.numel() == dc * dc * pc.levels[l]["blocks"]
            assert_same_bits(to_host(have), o.values[l], f"{what} level {l}")
        on = pc._device(k.device)
        for l, lv in enumerate(pc.levels):
            size = (d_ if l == 0 else dc)**2 * lv["nodes"]
            assert np.isfinite(o.inv[l]).all(), what
            assert_same_bits(to_host(on.inv[l][:size]), o.inv[l], f"{what} inverses of level {l}")
        assert not o.singular
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


@pytest.mark.parametrize("cycle", CYCLES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_apply_on_the_bits(fmt, cycle, small_cube):
    mesh, mask, systems = small_cube
    k, values, blocks = systems[fmt]
    n = k.shape[0]
    for seed, r in ((8, np.where(mask, 0.0, np.random.default_rng(8).normal(size=n))), (9, np.random.default_rng(9).normal(size=n))):
        for coarsest, depth in ((3000, 1), (20, 2), (1, 3)):
            for smoothing, sweeps in ((1, 8), (2, 1)):
                options = dict(cycle=cycle, smoothing=smoothing, coarsest_nodes=coarsest, coarsest_sweeps=sweeps)
                what = f"{fmt} {cycle} levels={depth} smoothing={smoothing} coarsest_sweeps={sweeps} r{seed}"
                pc = rigid(k, mesh.nodes, **options)
                assert len(pc.levels) == depth, what
                buf, out = guarded(n)
                assert pc.apply(values, to_device(r, "cuda"), out=out).data_ptr() == out.data_ptr()
                torch.cuda.synchronize()
                assert_margins_intact(buf, n)
                o = RU.Oracle(k.indptr, k.indices, mesh.nodes, mask=mask, **options).setup(blocks)
                have = to_host(out)
                assert_same_bits(have, o.apply(r), what)
                assert np.isfinite(have).all() and np.abs(have).max() > 0
                if seed == 8:
                    assert (bits(have[mask]) == 0).all(), what  # +0.0 at the constrained dofs
                if depth == 3 and seed == 9:  # the rotations matter: the translation hierarchy gives another vector
                    assert not np.array_equal(have, MU.Oracle(k.indptr, k.indices, mask=mask, **options).setup(blocks).apply(r))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. exactly k iterations of both solvers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", ["hex8", "tri_p2"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_exactly_k_iterations(method, shape, fmt):
    d_, a_, q_, _ = SHAPES[shape]
    k, values, blocks, mask, x = assembled(shape, -(-257 // q_), 21, fmt, symmetric=method == "cg")
    rng = np.random.default_rng(4)
    b = np.where(mask, 0.0, rng.normal(size=k.shape[0]))
    start = rng.normal(size=k.shape[0])
    for cycle in CYCLES:
        pc = rigid(k, x, cycle=cycle, coarsest_nodes=1)
        o = RU.Oracle(k.indptr, k.indices, x, cycle=cycle, coarsest_nodes=1, mask=mask)
        assert len(pc.levels) >= 3  # (both pairs of block sizes take part: (D, Dc) and (Dc, Dc))
        for its in (1, 2, 7):
            s = (fc.ConjugateGradient if method == "cg" else fc.BiCGStab)(k, preconditioner=pc, rtol=0.0, maxiter=its)
            for x0 in (None, start):
                what = f"{method} {shape} {fmt} {cycle} k={its} x0={'yes' if x0 is not None else 'no'}"
                if method == "cg":
                    want = RU.conjugate_gradient(o, blocks, b, x0=x0, rtol=0.0, maxiter=its)
                else:
                    want = oracle_bicgstab(k.indptr, k.indices, blocks, b, x0=x0, preconditioner=o, rtol=0.0, maxiter=its)
                res, got = solve_guarded(s, values, b, x0)
                assert want.status == "maxiter" and want.iterations == its, what
                assert_same_result(res, got, want, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the cube of 10^3 cells: check_every, singular blocks on the coarse levels, two instances side by side
# ---------------------------------------------------------------------------------------------------------------------------------
RUNS = ((("rtol", 0.0), ("maxiter", 11)), (("rtol", 1e-6),))


@pytest.fixture(scope="module")
def cube_system():
    """the tension-test matrix of a cube of 10^3 hexahedra (3993 dofs: two segments; levels 1331, 64, 8), block CSR, its right-hand
    side and the oracles of both coarse spaces"""
    mesh = FE.Cube(10, 10, 10)
    op, f = cube_operators(mesh)
    mask, top = tension_constraints(mesh)
    assert SEG < mesh.n_dofs <= 2 * SEG
    b = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mesh.n_dofs))
    k = fc.TangentMatrix(f, format="bsr")
    k.set_constrained(mask)
    values = k(to_device(spd_tangent(mesh.n_points, 6, 1, False), "cuda"))
    torch.cuda.synchronize()
    blocks = from_format("bsr", k.indptr, k.indices, to_host(values), 3)
    oracles = {("rigid_body", cycle): RU.Oracle(k.indptr, k.indices, mesh.nodes, cycle=cycle, coarsest_nodes=32, mask=mask) for cycle in CYCLES}
    oracles.update({("translations", cycle): MU.Oracle(k.indptr, k.indices, cycle=cycle, coarsest_nodes=32, mask=mask) for cycle in CYCLES})
    return mesh, mask, b, k, values, blocks, oracles


@pytest.mark.parametrize("cycle", CYCLES)
def test_check_every_changes_nothing(cycle, cube_system):
    mesh, mask, b, k, values, blocks, oracles = cube_system
    pc = rigid(k, mesh.nodes, cycle=cycle, coarsest_nodes=32)
    assert [lv["nodes"] for lv in pc.levels] == [1331, 64, 8] and pc._dofs == [3, 6, 6]
    for kw in RUNS:
        want = RU.conjugate_gradient(oracles[("rigid_body", cycle)], blocks, b, **dict(kw))
        assert want.status == ("maxiter" if "maxiter" in dict(kw) else "converged") and want.iterations >= 11
        for every in (1, 3, 16):
            res, x = solve_guarded(fc.ConjugateGradient(k, preconditioner=pc, check_every=every, **dict(kw)), values, b)
            assert_same_result(res, x, want, f"{cycle} {dict(kw)} check_every={every}")
            assert res.looks == 1 + -(-want.iterations // every)
    plain = MU.conjugate_gradient(oracles[("translations", cycle)], blocks, b, rtol=1e-6)
    print(f"cube of 10^3 cells, random SPD tangent, {cycle}, rtol 1e-6: translations {plain.iterations} iterations, rigid body {want.iterations}")


@pytest.mark.parametrize("case", ["3-D", "2-D"])
def test_singular_block_on_a_coarse_level(case, cube_system):
    """Level 0 stays regular; the coarse level's own block is what the inverse kernel of the coarse program refuses: (a) the block of
    a coarse node zeroed in the values ``setup`` left and the inverse launch of that level repeated (6 x 6: a zero pivot; 3 x 3: a zero
    determinant); (b) a whole solve in which an infinite entry in an off-diagonal block between two members of aggregate 0 makes
    that aggregate's coarse block non-finite: ``singular_block``, no iteration, x is x0 -- as the oracle says."""
    if case == "3-D":
        mesh, mask, b, k, values, blocks, oracles = cube_system
        x, oracle = mesh.nodes, oracles[("rigid_body", "multiplicative")]
        pc = rigid(k, x, coarsest_nodes=32)
    else:
        k, values, blocks, mask, x = assembled("tri_p2", 43, 21, "bsr", symmetric=True)
        b = np.where(mask, 0.0, np.random.default_rng(1).normal(size=k.shape[0]))
        pc = rigid(k, x, coarsest_nodes=4)
        oracle = RU.Oracle(k.indptr, k.indices, x, coarsest_nodes=4, mask=mask)
    dev, dc = k.device, pc.coarse_dofs
    assert dc == (6 if case == "3-D" else 3) and len(pc.levels) >= 2
    # (a)
    coarse = pc.setup(values)
    control = pc._device(dev).control
    control.download(dev)
    assert int(control.ints[solver._STATUS]) == 0
    own = int(pc.diag_block(1)[pc.levels[1]["nodes"] // 2])
    coarse[0][dc * dc * own: dc * dc * (own + 1)] = 0.0
    jit.launch(pc._coarse_code, dev, 1, pc._level_args(dev, 1, values, control), "the inverse launch of level 1", kernel=solver.INVERSE_KERNEL)
    control.download(dev)
    assert int(control.ints[solver._STATUS]) == SINGULAR
    # (b)
    members = np.flatnonzero(pc.aggregates(0) == 0)
    rows = np.repeat(np.arange(k.n_nodes), np.diff(k.indptr))
    inside = np.flatnonzero(np.isin(rows, members) & np.isin(k.indices, members) & (rows != k.indices))
    bad = blocks.copy()
    bad[inside[0], 0, 0] = np.inf
    start = np.random.default_rng(2).normal(size=b.size)
    want = RU.conjugate_gradient(oracle, bad, b, x0=start)
    refused = [bool((~(det != 0.0) | ~np.isfinite(det)).any()) for det in oracle.det]
    assert want.status == "singular_block" and not refused[0] and refused[1]  # level 0 is regular: the coarse level is what is refused
    for solver_class in (fc.ConjugateGradient, fc.BiCGStab):
        res, got = solve_guarded(solver_class(k, preconditioner=pc), to_device(bad.reshape(-1), "cuda"), b, start)
        assert (res.status, res.iterations, res.converged, res.looks) == ("singular_block", 0, False, 1)
        assert_same_bits(got, start, f"{case} {solver_class.__name__}: singular block")
    # and the object solves again afterwards
    res, got = solve_guarded(fc.ConjugateGradient(k, preconditioner=pc, rtol=0.0, maxiter=2), values, b)
    assert_same_result(res, got, RU.conjugate_gradient(oracle, blocks, b, rtol=0.0, maxiter=2), f"{case}: after the singular block")


@pytest.mark.parametrize("cycle", CYCLES)
def test_two_coarse_spaces_of_one_matrix_side_by_side(cycle, cube_system):
    """A translation instance and a rigid-body instance of the same K, used alternately in one process with the same vectors: each
    stays on its own oracle's bits, and each keeps its own launch plans."""
    mesh, mask, b, k, values, blocks, oracles = cube_system
    n, dev = k.shape[0], k.device
    pcs = {"translations": fc.MultilevelPreconditioner(k, cycle=cycle, coarsest_nodes=32), "rigid_body": rigid(k, mesh.nodes, cycle=cycle, coarsest_nodes=32)}
    assert pcs["translations"]._code is not pcs["rigid_body"]._code and pcs["translations"].coarse_space == "translations"
    r = to_device(b, "cuda")
    buf, out = guarded(n)
    want = {space: oracles[(space, cycle)].setup(blocks).apply(b) for space in pcs}
    assert not np.array_equal(want["translations"], want["rigid_body"])
    solves = {space: MU.conjugate_gradient(oracles[(space, cycle)], blocks, b, rtol=0.0, maxiter=3) for space in pcs}
    cgs = {space: fc.ConjugateGradient(k, preconditioner=pc, rtol=0.0, maxiter=3) for space, pc in pcs.items()}
    for turn in range(3):
        for space, pc in pcs.items():
            pc.apply(values, r, out=out)  # (the same r and out for both: the keys differ in nothing but the coarse space)
            torch.cuda.synchronize()
            assert_margins_intact(buf, n)
            assert_same_bits(to_host(out), want[space], f"{cycle} {space} turn {turn}: apply")
            res, x = solve_guarded(cgs[space], values, b)
            assert_same_result(res, x, solves[space], f"{cycle} {space} turn {turn}: solve")
    plans = {space: pc._device(dev).plans for space, pc in pcs.items()}
    assert plans["translations"] is not plans["rigid_body"]
    for space in pcs:
        assert 2 <= len(plans[space]) <= multilevel.PLANS and all(key[-1] == space for key in plans[space])
        programs = {code for ops, _ in plans[space].values() for code, *_ in ops}
        assert programs == ({pcs[space]._code} if space == "translations" else {pcs[space]._code, pcs[space]._coarse_code})
    assert not set(plans["translations"]) & set(plans["rigid_body"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. one compute unit's blocks on the cube of 32^3 cells
# ---------------------------------------------------------------------------------------------------------------------------------
def test_two_iterations_on_one_compute_unit(one_cu):
    """35 937 nodes: 36 segments, more than two trips of the 16 blocks a single compute unit is capped at; levels 35937, 1331, 64"""
    mesh = FE.Cube(32, 32, 32)
    op, f = cube_operators(mesh)
    assert -(-mesh.n_dofs // SEG) > 2 * gradient.BLOCKS_PER_CU
    k = fc.TangentMatrix(f, format="csr")
    mask, _ = tension_constraints(mesh)
    k.set_constrained(mask)
    values = k(to_device(spd_tangent(mesh.n_points, 6, 2, False), "cuda"))
    torch.cuda.synchronize()
    blocks = from_format("csr", k.indptr, k.indices, to_host(values), 3)
    b = np.where(mask, 0.0, np.random.default_rng(3).normal(size=k.shape[0]))
    o = RU.Oracle(k.indptr, k.indices, mesh.nodes, mask=mask)
    assert [lv.indptr.size - 1 for lv in o.levels] == [35937, 1331, 64]
    pc = rigid(k, mesh.nodes)
    del one_cu[:]
    res, x = solve_guarded(fc.ConjugateGradient(k, preconditioner=pc, rtol=0.0, maxiter=2, check_every=2), values, b)
    assert_same_result(res, x, RU.conjugate_gradient(o, blocks, b, rtol=0.0, maxiter=2), "cube 32, two iterations on one compute unit")
    assert max(nb for _, nb in one_cu) == gradient.BLOCKS_PER_CU  # the launches really were capped
    capped = {name for name, nb in one_cu if nb == gradient.BLOCKS_PER_CU}
    assert set(multilevel.RIGID_KERNELS) | {multilevel.SMOOTH_KERNEL, multilevel.CLOSE_KERNEL, solver.INVERSE_KERNEL, solver.MATVEC_KERNEL} <= capped
    assert not {multilevel.GALERKIN_KERNEL, multilevel.RESTRICT_KERNEL, multilevel.PROLONG_KERNEL} & {name for name, _ in one_cu}


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the Newton loops of the examples
# ---------------------------------------------------------------------------------------------------------------------------------
def test_von_mises_loop_under_conjugate_gradients():
    """examples/cube_tension_multilevel.py on Cube(3, 2, 4) with the rigid-body instance, eight load steps, both cycles, against
    ``fe_mini.tension_test`` on the CPU with the oracle law and SciPy's direct solver: equal Newton counts, reactions within 1e-8"""
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    r_direct, norms_direct, _ = FE.tension_test(mesh, FE.CopyProtocolState(FE.OracleLaw(O.von_mises_3d, VM_P, {"eps_n": 6, "alpha": 1}), mesh.n_points), steps=8)
    for cycle in CYCLES:
        loop = multilevel_loop(mesh, fc.VonMises3D(VM_P), cycle, coarsest_nodes=8, coarse_space="rigid_body", coordinates=mesh.nodes)
        pc = loop.cg.preconditioner
        assert len(pc.levels) == 2 and pc.coarse_space == "rigid_body" and pc.coarse_dofs == 6
        r_gpu, norms_gpu, u, solves = tension_test_device_solve(mesh, loop, steps=8)  # (raises where a solve or a load step does not converge)
        difference = np.max(np.abs(r_gpu - r_direct)) / np.max(np.abs(r_direct))
        counts = [len(h) for h in norms_gpu]
        print(f"rigid-body tension test, von Mises {cycle}: GPU against direct {difference:.3e}, Newton iterations {counts}, conjugate-gradient iterations {solves}")
        assert counts == [len(h) for h in norms_direct] == [2, 2, 2, 3, 3, 4, 5, 5]
        assert difference <= 1e-8, difference


def test_drucker_prager_loop_under_bicgstab():
    """examples/cube_tension_nonsymmetric.py on Cube(3, 2, 4) with the rigid-body instance: non-associated DruckerPrager3D, eight load
    steps, BiCGStab(rtol=1e-12), both cycles, against the CPU run with the oracle law and SciPy's direct solver"""
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    state = FE.CopyProtocolState(FE.OracleLaw(O.comfe_drucker_prager, DP_P, {"history": 7}), mesh.n_points)
    with np.errstate(all="ignore"):
        r_direct, norms_direct, _ = FE.tension_test(mesh, state, steps=8, top_displacement=TOP_DISPLACEMENT)
    for cycle in CYCLES:
        loop = nonsymmetric_loop(mesh, drucker_prager(), cycle, rtol=1e-12, coarsest_nodes=8, coarse_space="rigid_body", coordinates=mesh.nodes)
        assert isinstance(loop.cg, fc.BiCGStab) and loop.cg.preconditioner.coarse_dofs == 6 and len(loop.cg.preconditioner.levels) == 2
        r_gpu, norms_gpu, u, solves = tension_test_device_solve(mesh, loop, steps=8, top_displacement=TOP_DISPLACEMENT)
        difference = np.max(np.abs(r_gpu - r_direct)) / np.max(np.abs(r_direct))
        counts = [len(h) for h in norms_gpu]
        print(f"rigid-body nonsymmetric tension test, {cycle}: GPU against direct {difference:.3e}, Newton iterations {counts}, BiCGStab iterations {solves}")
        assert counts == [len(h) for h in norms_direct] == [2, 3, 3, 4, 6, 6, 6, 6]
        assert difference <= 1e-8, difference
