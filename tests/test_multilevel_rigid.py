"""The rigid-body coarse space of the multilevel preconditioner without a GPU (fenics_constitutive_amd.multilevel,
csrc/jit/multilevel_rigid.hip): both programs compile for gfx950 without scratch and with the LDS the module states; the refusals
come before any compilation, upload or launch; ``coarse_space="translations"`` is the object built without the argument and 1-D
gives the translation hierarchy; the property itself on the oracle of rigid_body_util.py -- P reproduces the rigid-body fields of
every level pair, the Galerkin matrices of the free elastic cube annihilate the coarse rigid modes --; and the oracle's conjugate
gradients on the tension cube take fewer iterations with the rigid-body modes than with the translations."""

import os
import sys

import numpy as np
import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import gradient, jit, multilevel, solver
from fenics_constitutive_amd.force import kernel_resources

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_constraints  # noqa: E402
from force_util import random_inputs  # noqa: E402
from gradient_util import SHAPES, cube_operator_tables  # noqa: E402
from matrix_util import matrix_oracle  # noqa: E402
import multilevel_util as MU  # noqa: E402
import rigid_body_util as RU  # noqa: E402
from solver_util import full_pattern, matvec  # noqa: E402

CYCLES = ("multiplicative", "additive")


def elastic_tangent(e_modulus=210000.0, nu=0.3):
    lam, mu = e_modulus * nu / ((1 + nu) * (1 - 2 * nu)), e_modulus / (2 * (1 + nu))
    c = 2 * mu * np.eye(6)
    c[:3, :3] += lam
    return c


def cube_matrix(mesh, constrained=True):
    """(TangentMatrix, indptr, indices, blocks, mask): the elastic cube, with the tension test's constraints or free, on the CPU"""
    dofmap, ref, jinv = cube_operator_tables(mesh)
    weights = gradient.integration_weights(mesh.nodes[mesh.cells], ref, np.ones(8))
    mask, _ = tension_constraints(mesh)
    if not constrained:
        mask[:] = False
    tangent = np.tile(elastic_tangent().reshape(-1), mesh.n_points)
    indptr, indices, blocks = matrix_oracle(tangent, dofmap, ref, jinv, weights, mesh.n_nodes, constrained=mask)
    k = fc.TangentMatrix(fc.InternalForce(fc.DisplacementGradient(dofmap, ref, jinv, mesh.n_nodes), weights))
    k.set_constrained(mask)
    return k, indptr, indices, blocks, mask


def random_matrix(shape, n_cells, seed, lonely=False):
    """(TangentMatrix, coordinates): random tables over the nodes their cells use (``lonely``: and the node no cell touches, alone in
    its row) with seeded random coordinates"""
    d_, a_, q_, affine = SHAPES[shape]
    t = random_inputs(shape, n_cells, seed, False, affine)
    if lonely:
        dofmap, n_nodes = t["dofmap"], t["n_nodes"]
        pat, _ = full_pattern(dofmap, n_nodes)
    else:
        used, dofmap = np.unique(t["dofmap"], return_inverse=True)
        dofmap, n_nodes = dofmap.reshape(t["dofmap"].shape).astype(np.int32), int(used.size)
        pat = None
    k = fc.TangentMatrix(fc.InternalForce(fc.DisplacementGradient(dofmap, t["ref"], t["jinv"], n_nodes), t["weights"]), pattern_dofmap=pat)
    return k, np.random.default_rng(seed + 77).normal(size=(n_nodes, d_))


@pytest.fixture(scope="module")
def small_cube():
    mesh = FE.Cube(3, 2, 4)
    return (mesh,) + cube_matrix(mesh)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. compilation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gdim", [2, 3])
def test_both_programs_compile_without_scratch(gdim):
    k, x = random_matrix({2: "tri_p2", 3: "hex8"}[gdim], 40, 9)
    pc = fc.MultilevelPreconditioner(k, coarsest_nodes=1, coarse_space="rigid_body", coordinates=x)
    fine, coarse = multilevel.compile_rigid_kernels(gdim)
    assert pc._code is fine and pc._coarse_code is coarse  # the two programs of an object
    assert fine is not coarse and multilevel.coarse_dofs(gdim) == {2: 3, 3: 6}[gdim]
    for code in (fine, coarse):
        for kernel in solver.KERNELS + multilevel.KERNELS + multilevel.RIGID_KERNELS:
            r = kernel_resources(code.log, kernel)
            assert r["scratch_bytes"] == 0, (kernel, r)
            assert r["lds_bytes"] == multilevel.lds_bytes(kernel) <= 64 * 1024, (kernel, r)
    assert all(multilevel.lds_bytes(kernel) == 0 for kernel in multilevel.RIGID_KERNELS)
    before = jit.compile_count()
    assert multilevel.compile_rigid_kernels(gdim) == (fine, coarse) and jit.compile_count() == before
    # the translation program and the solver's own are other programs and still compile as they did
    assert multilevel.compile_kernels(gdim) not in (fine, coarse)
    with pytest.raises(ValueError, match="dofs per node"):
        multilevel.compile_kernels(4)
    with pytest.raises(ValueError, match="2 or 3"):
        multilevel.compile_rigid_kernels(1)
    assert f"#define FCAMD_CG_D {gdim}\n" in multilevel.rigid_program(gdim, gdim) and f"#define FCAMD_ML_GDIM {gdim}\n" in multilevel.rigid_program(gdim, gdim)


def test_object_reports_what_was_built(small_cube):
    mesh, k = small_cube[:2]
    pc = fc.MultilevelPreconditioner(k, coarsest_nodes=1, coarse_space="rigid_body", coordinates=mesh.nodes)
    assert (pc.coarse_space, pc.coarse_dofs, len(pc.levels)) == ("rigid_body", 6, 3)
    assert set(pc.resources) == {"galerkin", "restrict", "prolong", "smooth", "close", "rigid_galerkin", "rigid_restrict", "rigid_prolong", "coarse"}
    assert all(r["scratch_bytes"] == 0 for name, r in pc.resources.items() if name != "coarse")
    assert all(r["scratch_bytes"] == 0 for r in pc.resources["coarse"].values())
    assert all(kernel in pc.compile_log and kernel in pc.coarse_compile_log for kernel in multilevel.RIGID_KERNELS + multilevel.KERNELS + solver.KERNELS)
    want = RU.Oracle(k.indptr, k.indices, mesh.nodes, coarsest_nodes=1)
    for l in range(3):
        assert np.array_equal(pc.positions(l), want.positions[l]) and pc.positions(l).shape == (pc.levels[l]["nodes"], 3)
    for l in range(2):
        assert np.array_equal(pc.offsets(l), want.offsets[l])
        assert np.array_equal(pc.aggregates(l), want.levels[l].agg)
    with pytest.raises(ValueError, match="coarser"):
        pc.offsets(2)
    with pytest.raises(AttributeError):
        pc.coarse_space = "translations"
    assert fc.ConjugateGradient(k, preconditioner=pc).preconditioner is pc and fc.BiCGStab(k, preconditioner=pc).preconditioner is pc
    default = fc.ConjugateGradient(k, preconditioner="multilevel").preconditioner
    assert (default.coarse_space, default.coarse_dofs) == ("translations", 3)
    with pytest.raises(ValueError, match="rigid_body"):
        default.positions(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. refusals: before anything is compiled, uploaded or launched
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_launch_counter_at_zero(small_cube):
    mesh, k = small_cube[:2]
    x = mesh.nodes
    lonely, lonely_x = random_matrix("tet_p2", 5, 3, lonely=True)
    # the first aggregate of the cube (the neighbourhood of node 0) laid on one line
    agg, _ = multilevel.aggregate(k.indptr, k.indices)
    first = np.flatnonzero(agg == 0)
    line = x.copy()
    line[first] = x[first[0]] + np.arange(first.size)[:, None] * np.array([0.25, -0.5, 0.125])
    point = x.copy()
    point[first] = x[first[0]]
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    ML = fc.MultilevelPreconditioner
    ML(k, coarse_space="rigid_body", coordinates=x)  # (everything this pattern needs is compiled now)
    compiled = jit.compile_count()
    try:
        with pytest.raises(ValueError, match="needs coordinates"):
            ML(k, coarse_space="rigid_body")
        with pytest.raises(ValueError, match="shape"):
            ML(k, coarse_space="rigid_body", coordinates=x[:-1])
        with pytest.raises(ValueError, match="shape"):
            ML(k, coarse_space="rigid_body", coordinates=x[:, :2])
        with pytest.raises(ValueError, match="shape"):
            ML(k, coarse_space="rigid_body", coordinates=x.reshape(-1))
        with pytest.raises(TypeError, match="float64"):
            ML(k, coarse_space="rigid_body", coordinates=x.astype(np.float32))
        with pytest.raises(TypeError, match="NumPy"):
            ML(k, coarse_space="rigid_body", coordinates=x.tolist())
        for bad in (np.nan, np.inf):
            y = x.copy()
            y[7, 1] = bad
            with pytest.raises(ValueError, match="finite"):
                ML(k, coarse_space="rigid_body", coordinates=y)
        with pytest.raises(ValueError, match="coordinates"):
            ML(k, coordinates=x)
        with pytest.raises(ValueError, match="coordinates"):
            ML(k, coarse_space="translations", coordinates=x)
        for unknown in ("rigid", "Rigid_Body", None, 3):
            with pytest.raises(ValueError, match="coarse_space"):
                ML(k, coarse_space=unknown, coordinates=x)
        # degenerate aggregates: the message names the aggregate
        assert lonely.n_nodes > 1
        with pytest.raises(ValueError, match=r"aggregate \d+ of level 0 .*lone node"):
            ML(lonely, coarsest_nodes=1, coarse_space="rigid_body", coordinates=lonely_x)
        with pytest.raises(ValueError, match=r"aggregate 0 of level 0 .*one line"):
            ML(k, coarsest_nodes=8, coarse_space="rigid_body", coordinates=line)
        with pytest.raises(ValueError, match=r"aggregate 0 of level 0 .*one point"):
            ML(k, coarsest_nodes=8, coarse_space="rigid_body", coordinates=point)
        # one level: there is no aggregate, nothing to refuse
        assert len(ML(k, coarsest_nodes=3000, coarse_space="rigid_body", coordinates=line).levels) == 1
    finally:
        jit.launch = real
    assert not launches and jit.compile_count() == compiled and not k._on and not lonely._on


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the translations are today's object; 1-D has no rotation
# ---------------------------------------------------------------------------------------------------------------------------------
def test_translations_is_the_object_without_the_argument(small_cube):
    mesh, k = small_cube[:2]
    plain, named = fc.MultilevelPreconditioner(k, coarsest_nodes=1), fc.MultilevelPreconditioner(k, coarsest_nodes=1, coarse_space="translations")
    rigid = fc.MultilevelPreconditioner(k, coarsest_nodes=1, coarse_space="rigid_body", coordinates=mesh.nodes)
    assert named._code is plain._code is multilevel.compile_kernels(3) and named._coarse_code is named._code and not named._rigid
    assert rigid._code is not plain._code and rigid._coarse_code is not rigid._code
    assert named.coarse_space == plain.coarse_space == "translations" and named.coarse_dofs == plain.coarse_dofs == 3
    assert named.levels == plain.levels == rigid.levels and named._dofs == plain._dofs == [3, 3, 3] and rigid._dofs == [3, 6, 6]
    for l in range(2):
        for other in (named, rigid):  # the aggregation, patterns, fold and members are the existing ones, whatever the coarse space
            for have, want in ((other.aggregates(l), plain.aggregates(l)), (other.roots(l), plain.roots(l)), *zip(other.members(l), plain.members(l)),
                               *zip(other.folds(l), plain.folds(l)), *zip(other.pattern(l + 1), plain.pattern(l + 1))):
                assert have.dtype == want.dtype and np.array_equal(have, want)
    assert multilevel.program(3) == "#define FCAMD_CG_D 3\n#define FCAMD_CG_PRECOND 2\n#define FCAMD_CG_SLAB 1024\n#include \"multilevel.hip\"\n"


def test_one_dimension_gives_the_translation_hierarchy():
    k, x = random_matrix("interval", 40, 5)
    assert k.gdim == 1 and x.shape == (k.n_nodes, 1)
    plain = fc.MultilevelPreconditioner(k, coarsest_nodes=1)
    rigid = fc.MultilevelPreconditioner(k, coarsest_nodes=1, coarse_space="rigid_body", coordinates=x)
    assert rigid.coarse_space == "rigid_body" and rigid.coarse_dofs == 1 and rigid._dofs == plain._dofs and not rigid._rigid
    assert rigid._code is plain._code and rigid._coarse_code is plain._code and len(rigid.levels) == len(plain.levels) >= 3
    for l in range(len(plain.levels) - 1):
        assert np.array_equal(rigid.aggregates(l), plain.aggregates(l)) and np.array_equal(rigid.folds(l)[1], plain.folds(l)[1])
    assert np.array_equal(rigid.positions(0), x)
    with pytest.raises(ValueError, match="needs coordinates"):
        fc.MultilevelPreconditioner(k, coarse_space="rigid_body")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the property itself, on the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def dense_prolongator(agg, p, n_agg):
    n, df, dc = p.shape
    out = np.zeros((n * df, n_agg * dc))
    for i in range(n):
        out[df * i: df * i + df, dc * agg[i]: dc * agg[i] + dc] = p[i]
    return out


@pytest.mark.parametrize("case", ["cube", "tri_p2"])
def test_prolongation_reproduces_the_rigid_body_fields(case, small_cube):
    """For every level pair: P applied to the coarse rigid-body modes about any x0 is the fine field t + theta x (x - x0) (and, on
    a level l >= 1, the rotation itself), to rounding: an entry is one sum of two products of offsets bounded by the diameter."""
    if case == "cube":
        mesh, k = small_cube[:2]
        x = mesh.nodes
    else:
        k, x = random_matrix("tri_p2", 40, 11)
    g = x.shape[1]
    o = RU.Oracle(k.indptr, k.indices, x, coarsest_nodes=1)
    pc = fc.MultilevelPreconditioner(k, coarsest_nodes=1, coarse_space="rigid_body", coordinates=x)
    assert len(o.levels) >= 3 and pc._dofs == o.dofs == [g] + [RU.coarse_dofs(g)] * (len(o.levels) - 1)
    for l in range(len(o.levels) - 1):  # the object's own placement is the oracle's, on the bits
        assert np.array_equal(pc.positions(l + 1), o.positions[l + 1]) and np.array_equal(pc.offsets(l), o.offsets[l])
    x0 = np.random.default_rng(2).normal(size=g)
    size = 1.0 + np.abs(x - x0).max()
    for l in range(len(o.levels) - 1):
        lv = o.levels[l]
        # the coarse position is the centroid, the offsets sum to rounding
        counts = np.bincount(lv.agg)
        sums = np.zeros((lv.roots.size, g))
        np.add.at(sums, lv.agg, o.offsets[l])
        assert o.positions[l + 1].shape == (lv.roots.size, g) and np.abs(sums).max() <= 8 * counts.max() * RU.EPS * size
        p = dense_prolongator(lv.agg, o.p[l], lv.roots.size)
        coarse, fine = RU.rigid_modes(o.positions[l + 1], x0, o.dofs[l + 1]), RU.rigid_modes(o.positions[l], x0, o.dofs[l])
        assert fine.shape == (o.dofs[l] * lv.agg.size, o.dofs[l + 1]) and np.linalg.matrix_rank(fine) == o.dofs[l + 1]
        assert np.abs(p @ coarse - fine).max() <= 8 * RU.EPS * size, l
        # the oracle's own prolongation and restriction are this matrix and its transpose
        v = np.random.default_rng(l).normal(size=coarse.shape[0])
        w = np.random.default_rng(l + 9).normal(size=fine.shape[0])
        assert np.abs(RU.prolong(lv.agg, np.zeros(fine.shape[0]), v, o.p[l]) - p @ v).max() <= 16 * RU.EPS * (np.abs(p) @ np.abs(v)).max()
        assert np.abs(RU.restrict(lv.agg, lv.roots.size, w, o.p[l]) - p.T @ w).max() <= 4 * counts.max() * g * RU.EPS * (np.abs(p.T) @ np.abs(w)).max()


def test_galerkin_matrices_annihilate_the_coarse_rigid_modes():
    """The free elastic Cube(3, 2, 4): K has the six rigid-body modes in its kernel, P reproduces them, so every Galerkin matrix
    times a coarse rigid mode is zero up to the rounding of the sums.  The oracle's own value is 5.6e-15 |K|_max on level 1 and
    1.8e-14 |K|_max on level 2 (summation order is the only source of error); the bound is ten times the larger."""
    import scipy.sparse  # noqa: F401  (matrix_util's to_bsr)
    from matrix_util import to_bsr

    mesh = FE.Cube(3, 2, 4)
    k, indptr, indices, blocks, mask = cube_matrix(mesh, constrained=False)
    assert not mask.any()
    o = RU.Oracle(indptr, indices, mesh.nodes, coarsest_nodes=1).setup(blocks)
    pc = fc.MultilevelPreconditioner(k, coarsest_nodes=1, coarse_space="rigid_body", coordinates=mesh.nodes)
    assert [lv.indptr.size - 1 for lv in o.levels] == [lv["nodes"] for lv in pc.levels] == [60, 4, 1]
    assert all(np.array_equal(pc.offsets(l), o.offsets[l]) for l in range(2))
    scale = np.abs(blocks).max()
    x0 = np.array([0.3, -0.2, 0.7])
    fine = RU.rigid_modes(mesh.nodes, x0, 3)
    assert max(np.abs(matvec(indptr, indices, blocks, fine[:, c])).max() for c in range(6)) <= 1e-13 * scale  # K itself
    for l in (1, 2):
        lv = o.levels[l]
        modes = RU.rigid_modes(o.positions[l], x0, 6)
        worst = max(np.abs(matvec(lv.indptr, lv.indices, o.values[l], modes[:, c])).max() for c in range(6))
        print(f"level {l}: |K_l m| / |K|_max = {worst / scale:.3e}")
        assert worst <= 10 * 1.8e-14 * scale, (l, worst / scale)
        # and it is the triple product: against SciPy's, entry by entry
        p = dense_prolongator(o.levels[l - 1].agg, o.p[l - 1], lv.indptr.size - 1)
        kf = to_bsr(o.levels[l - 1].indptr, o.levels[l - 1].indices, o.values[l - 1], o.levels[l - 1].indptr.size - 1).toarray()
        want, size = p.T @ kf @ p, np.abs(p.T) @ np.abs(kf) @ np.abs(p)
        have = to_bsr(lv.indptr, lv.indices, o.values[l], lv.indptr.size - 1).toarray()
        assert (np.abs(have - want) <= kf.shape[0] * RU.EPS * size).all() and np.abs(want).max() > 0
    # the level-1 matrix is not zero, and with the translations alone the rotations are not in the coarse space at all
    assert np.abs(o.values[1]).max() >= 0.1 * scale


def test_six_by_six_inverse_against_numpy(small_cube):
    mesh, k = small_cube[:2]
    assert fc.MultilevelPreconditioner(k, coarsest_nodes=8, coarse_space="rigid_body", coordinates=mesh.nodes).coarse_dofs == 6  # the block size in question
    rng = np.random.default_rng(6)
    m = rng.normal(size=(50, 6, 6)) + 6.0 * np.eye(6)
    inv, det = RU.block_inverses(m)
    assert (det == 1.0).all() and np.abs(inv @ m - np.eye(6)).max() <= 1e-12
    m[3, 2] = 0.0  # (a zero pivot turns up in the elimination: no search)
    m[3, :, 2] = 0.0
    m[7, 0, 0] = np.inf
    inv, det = RU.block_inverses(m)
    assert det[3] == 0.0 and det[7] == 0.0 and det.sum() == 48.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the iteration counts
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", CYCLES)
def test_fewer_iterations_than_the_translations(cycle):
    """The elastic cube with the tension test's constraints, a seeded normal right-hand side zeroed at the constrained dofs, rtol
    1e-8, coarsest_nodes 32: the oracle's conjugate gradients take strictly fewer iterations with the rigid-body modes.  Measured
    (translations -> rigid body): 6^3 cells: multiplicative 42 -> 35, additive 80 -> 68; 10^3: multiplicative 61 -> 42, additive 123 -> 90; 16^3 (not run
    here, half a minute): multiplicative 95 -> 71, additive 191 -> 149."""
    for m in (6, 10):
        mesh = FE.Cube(m, m, m)
        k, indptr, indices, blocks, mask = cube_matrix(mesh)
        b = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mask.size))
        plain = MU.conjugate_gradient(MU.Oracle(indptr, indices, cycle=cycle, coarsest_nodes=32, mask=mask), blocks, b, rtol=1e-8)
        o = RU.Oracle(indptr, indices, mesh.nodes, cycle=cycle, coarsest_nodes=32, mask=mask)
        pc = fc.MultilevelPreconditioner(k, cycle=cycle, coarsest_nodes=32, coarse_space="rigid_body", coordinates=mesh.nodes)
        assert [lv["nodes"] for lv in pc.levels] == [lv.indptr.size - 1 for lv in o.levels]  # the hierarchy the device solver would use
        assert all(np.array_equal(pc.offsets(l), o.offsets[l]) for l in range(len(o.levels) - 1))
        rigid = RU.conjugate_gradient(o, blocks, b, rtol=1e-8)
        print(f"cube of {m}^3 cells, {cycle}: translations {plain.iterations}, rigid body {rigid.iterations}")
        assert plain.converged and rigid.converged and len(o.levels) >= 2
        assert rigid.iterations < plain.iterations, (m, cycle, plain.iterations, rigid.iterations)
        if m == 10:
            assert (plain.iterations, rigid.iterations) == {"multiplicative": (61, 42), "additive": (123, 90)}[cycle]
