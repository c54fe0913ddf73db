"""The rigid-body coarse space on a matrix-free operator without a GPU (fenics_constitutive_amd.MultilevelPreconditioner(A,
coarse_space="rigid_body") with a TangentOperator, csrc/jit/multilevel_free_rigid.hip): the gather compiles for gfx950 without scratch
and with the LDS the module states; positions and offsets are the assembled route's; every refusal comes before any compilation,
upload or launch; the translations on an operator stay the object built without the argument; the oracle's level-1 values
(multilevel_free_rigid_util.py) against the assembled rigid-body Galerkin step within the rounding of two orders of one sum, on the
bits for every chunk size and exactly on integer inputs; the Galerkin matrix of the free elastic cube annihilates the coarse rigid
modes; the oracle solvers in the Newton loops of the examples against the direct solve; and the iteration counts against the
translations'."""

import os
import sys

import numpy as np
import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import gradient, hostio, jit, matrix, multilevel, solver
from fenics_constitutive_amd.force import kernel_resources

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_constraints, tension_test_device_solve  # noqa: E402
from cube_tension_matrix_free import cube_operators  # noqa: E402
from fe_gpu_util import bits, tables_of  # noqa: E402
from gradient_util import SHAPES, cube_operator_tables  # noqa: E402
from matrix_util import matrix_oracle  # noqa: E402
import multilevel_free_rigid_util as FR  # noqa: E402
import multilevel_free_util as MF  # noqa: E402
import multilevel_util as MU  # noqa: E402
import rigid_body_util as RU  # noqa: E402
from solver_util import matvec  # noqa: E402
from tangent_operator_util import distinct_inputs, random_mask  # noqa: E402

CYCLES = ("multiplicative", "additive")
RIGID_SHAPES = tuple(name for name in sorted(SHAPES) if SHAPES[name][0] > 1)  # every shape of 2 and 3 dimensions
ORACLE_SHAPES = ("hex8", "tet_p2", "tri_p2")
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
KERNEL = "fcamd_mfr_galerkin_kernel"  # multilevel.FREE_RIGID_GALERKIN_KERNEL


def operator(shape="tet_p2", n_cells=9, seed=3, affine=True, every_node=True, **kwargs):
    """(TangentOperator, tables, coordinates): random cells over distinct nodes with seeded random coordinates"""
    t = distinct_inputs(shape, n_cells, seed, False, affine, every_node=every_node)
    f = fc.InternalForce(fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"]), t["weights"])
    return fc.TangentOperator(f, **kwargs), t, np.random.default_rng(seed + 77).normal(size=(t["n_nodes"], SHAPES[shape][0]))


def elastic_tangent(n_points, e_modulus=210000.0, nu=0.3):
    lam, mu = e_modulus * nu / ((1 + nu) * (1 - 2 * nu)), e_modulus / (2 * (1 + nu))
    c = 2 * mu * np.eye(6)
    c[:3, :3] += lam
    return np.tile(c.reshape(-1), n_points)


def cube_tables(mesh):
    dofmap, ref, jinv = cube_operator_tables(mesh)
    return dofmap, ref, jinv, gradient.integration_weights(mesh.nodes[mesh.cells], ref, np.ones(8)), mesh.n_nodes


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. compilation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "per_point"])
@pytest.mark.parametrize("shape", RIGID_SHAPES)
def test_the_gather_compiles_without_scratch(shape, affine):
    d_, a_, q_, _ = SHAPES[shape]
    gather = multilevel.compile_free_rigid_kernels(d_, a_)
    r = kernel_resources(gather.log, KERNEL)
    assert r["scratch_bytes"] == 0 and r["lds_bytes"] == multilevel.lds_bytes(KERNEL, d_) == {2: 5376, 3: 5184}[d_], r
    assert r["vgprs"] <= 128 and r["waves_per_simd"] >= 4, r  # (256-thread blocks: no fewer waves than a block has per SIMD)
    before = jit.compile_count()
    assert multilevel.compile_free_rigid_kernels(d_, a_) is gather and jit.compile_count() == before  # once per program text
    assert multilevel.free_rigid_program(d_, a_) == f'#define FCAMD_MF_D {d_}\n#define FCAMD_MF_A {a_}\n#include "multilevel_free_rigid.hip"\n'
    # the object holds this gather, the element kernel of the assembled route and the two programs of the rigid-body space
    a, t, x = operator(shape, 5, 3, affine)
    pc = fc.MultilevelPreconditioner(a, coarsest_nodes=2, coarse_space="rigid_body", coordinates=x)
    fine, coarse = multilevel.compile_rigid_kernels(d_)
    assert pc._code is fine and pc._coarse_code is coarse and pc._seam.gather_code is gather
    assert pc._seam.element_code is matrix.compile_kernels(d_, a_, q_, affine)
    res = pc.resources
    assert set(res) == {"galerkin", "restrict", "prolong", "smooth", "close", "rigid_galerkin", "rigid_restrict", "rigid_prolong", "coarse",
                        "free_rigid_galerkin", "free_element"}
    assert res["free_rigid_galerkin"] == r and res["free_element"]["scratch_bytes"] == 0
    assert pc.compile_log is fine.log and pc.coarse_compile_log is coarse.log and pc.lds_bytes(KERNEL, d_) == r["lds_bytes"]
    assert (pc.coarse_space, pc.coarse_dofs, pc.K) == ("rigid_body", RU.coarse_dofs(d_), a)
    assert fc.ConjugateGradient(a, preconditioner=pc).preconditioner is pc and fc.MatrixFreeBiCGStab(a, preconditioner=pc).preconditioner is pc
    for bad in (1, 4):
        with pytest.raises(ValueError, match="2 or 3"):
            multilevel.compile_free_rigid_kernels(bad, 4)


def test_one_dimension_gives_the_translation_hierarchy():
    a, t, x = operator("interval", 40, 5)
    plain = fc.MultilevelPreconditioner(a, coarsest_nodes=1)
    rigid = fc.MultilevelPreconditioner(a, coarsest_nodes=1, coarse_space="rigid_body", coordinates=x)
    assert rigid.coarse_space == "rigid_body" and rigid.coarse_dofs == 1 and rigid._dofs == plain._dofs and not rigid._rigid
    assert rigid._code is plain._code and rigid._coarse_code is plain._code and rigid._seam.gather_code is plain._seam.gather_code
    assert len(rigid.levels) == len(plain.levels) >= 2 and np.array_equal(rigid.positions(0), x)
    assert set(rigid.resources) == set(plain.resources)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the hierarchy, the positions and the offsets are the assembled route's
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ORACLE_SHAPES + ("cube",))
def test_positions_and_offsets_are_those_of_the_matrix(case):
    if case == "cube":
        mesh = FE.Cube(5, 4, 3)
        a, x = fc.TangentOperator(cube_operators(mesh)[1]), mesh.nodes
    else:
        a, t, x = operator(case, 40, 47, SHAPES[case][3])
    pc = fc.MultilevelPreconditioner(a, coarsest_nodes=1, coarse_space="rigid_body", coordinates=x)
    pk = fc.MultilevelPreconditioner(fc.TangentMatrix(a.force), coarsest_nodes=1, coarse_space="rigid_body", coordinates=x)
    assert pc.levels == pk.levels and pc.coarse_dofs == pk.coarse_dofs and pc._dofs == pk._dofs and len(pc.levels) >= (3 if case == "cube" else 2)
    for l in range(len(pk.levels)):
        assert np.array_equal(bits(pc.positions(l)), bits(pk.positions(l)))
        assert all(np.array_equal(have, want) for have, want in zip(pc.pattern(l), pk.pattern(l)))
    for l in range(len(pk.levels) - 1):
        assert np.array_equal(bits(pc.offsets(l)), bits(pk.offsets(l))) and np.array_equal(pc.aggregates(l), pk.aggregates(l))
    with pytest.raises(ValueError, match="coarser"):
        pc.offsets(len(pk.levels) - 1)
    o = FR.FreeRigidOracle(*(tables_of(t) if case != "cube" else cube_tables(mesh)), x, coarsest_nodes=1)
    assert all(np.array_equal(bits(pc.offsets(l)), bits(o.offsets[l])) for l in range(len(pk.levels) - 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. every refusal comes before anything is compiled, uploaded or launched
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_compile_launch_and_upload_nothing(monkeypatch):
    mesh = FE.Cube(3, 2, 4)
    a = fc.TangentOperator(cube_operators(mesh)[1])
    x = mesh.nodes
    lonely, _, lonely_x = operator("tet_p2", 5, 3, every_node=False)  # a node in no cell: an aggregate of its own
    agg, _ = multilevel.aggregate(*matrix.block_pattern(np.ascontiguousarray(mesh.cells, dtype=np.int32), mesh.n_nodes))
    first = np.flatnonzero(agg == 0)
    line, point = x.copy(), x.copy()
    line[first] = x[first[0]] + np.arange(first.size)[:, None] * np.array([0.25, -0.5, 0.125])
    point[first] = x[first[0]]
    ML = fc.MultilevelPreconditioner
    ML(a, coarsest_nodes=8, coarse_space="rigid_body", coordinates=x)  # (everything this operator needs is compiled now)
    counts = {"launch": 0, "upload": 0}
    real_launch, real_upload = jit.launch, hostio.upload
    monkeypatch.setattr(jit, "launch", lambda *args, **kw: counts.__setitem__("launch", counts["launch"] + 1) or real_launch(*args, **kw))
    monkeypatch.setattr(hostio, "upload", lambda *args, **kw: counts.__setitem__("upload", counts["upload"] + 1) or real_upload(*args, **kw))
    compiled = jit.compile_count()
    with pytest.raises(ValueError, match="needs coordinates"):
        ML(a, coarse_space="rigid_body")
    for wrong in (x[:-1], x[:, :2], x.reshape(-1)):
        with pytest.raises(ValueError, match="shape"):
            ML(a, coarse_space="rigid_body", coordinates=wrong)
    with pytest.raises(TypeError, match="float64"):
        ML(a, coarse_space="rigid_body", coordinates=x.astype(np.float32))
    with pytest.raises(TypeError, match="NumPy"):
        ML(a, coarse_space="rigid_body", coordinates=x.tolist())
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[7, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            ML(a, coarse_space="rigid_body", coordinates=y)
    with pytest.raises(ValueError, match="coordinates"):
        ML(a, coordinates=x)
    for unknown in ("rigid", None, 3):
        with pytest.raises(ValueError, match="coarse_space"):
            ML(a, coarse_space=unknown, coordinates=x)
    # all nodes at one point: the rotations vanish -- whatever the number of levels, and wherever the point is
    for where, coarsest in ((np.zeros_like(x), 64), (np.zeros_like(x), 8), (np.full_like(x, 1.5), 3000)):
        with pytest.raises(ValueError) as info:
            ML(a, coarsest_nodes=coarsest, coarse_space="rigid_body", coordinates=where)
        assert "rotations vanish" in str(info.value) and 'coarse_space="rigid_body"' in str(info.value) and 'coarse_space="translations"' in str(info.value)
    # degenerate aggregates of level 0: the message names the aggregate
    with pytest.raises(ValueError, match=r"aggregate \d+ of level 0 .*lone node"):
        ML(lonely, coarsest_nodes=1, coarse_space="rigid_body", coordinates=lonely_x)
    with pytest.raises(ValueError, match=r"aggregate 0 of level 0 .*one line"):
        ML(a, coarsest_nodes=8, coarse_space="rigid_body", coordinates=line)
    with pytest.raises(ValueError, match=r"aggregate 0 of level 0 .*one point"):
        ML(a, coarsest_nodes=8, coarse_space="rigid_body", coordinates=point)
    # one level: there is no aggregate, nothing to refuse
    assert len(ML(a, coarsest_nodes=3000, coarse_space="rigid_body", coordinates=line).levels) == 1
    # the matrix route keeps its own checks: coordinates at one point are a degenerate aggregate there, and fine on one level
    k = fc.TangentMatrix(a.force)
    with pytest.raises(ValueError, match=r"aggregate 0 of level 0 .*one point"):
        ML(k, coarsest_nodes=8, coarse_space="rigid_body", coordinates=np.zeros_like(x))
    assert len(ML(k, coarsest_nodes=3000, coarse_space="rigid_body", coordinates=np.zeros_like(x)).levels) == 1
    assert counts == {"launch": 0, "upload": 0} and jit.compile_count() == compiled
    assert not a._mask_on and not a._scratch and not a.force._on and not a.op._on and not lonely.force._on and not k._on  # nothing was uploaded


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the translations on an operator are the object built without the argument
# ---------------------------------------------------------------------------------------------------------------------------------
def test_translations_is_the_object_without_the_argument():
    mesh = FE.Cube(3, 2, 4)
    a = fc.TangentOperator(cube_operators(mesh)[1])
    plain, named = fc.MultilevelPreconditioner(a, coarsest_nodes=1), fc.MultilevelPreconditioner(a, coarsest_nodes=1, coarse_space="translations")
    rigid = fc.MultilevelPreconditioner(a, coarsest_nodes=1, coarse_space="rigid_body", coordinates=mesh.nodes)
    assert named._code is plain._code is multilevel.compile_kernels(3) and named._coarse_code is named._code and not named._rigid
    assert named._seam.gather_code is plain._seam.gather_code is multilevel.compile_free_kernels(3, 8) and named._seam.element_code is plain._seam.element_code
    assert rigid._seam.gather_code is not plain._seam.gather_code and rigid._seam.element_code is plain._seam.element_code
    assert set(named.resources) == set(plain.resources) == {"galerkin", "restrict", "prolong", "smooth", "close", "free_galerkin", "free_element"}
    assert named.levels == plain.levels == rigid.levels and named._dofs == plain._dofs == [3, 3, 3] and rigid._dofs == [3, 6, 6]
    for other in (named, rigid):  # the contribution lists and the chunks' block ranges are the same whatever the coarse space
        assert np.array_equal(other._seam.blk_ptr, plain._seam.blk_ptr) and np.array_equal(other._seam.contributions, plain._seam.contributions)
        assert other._seam.chunk_blocks == plain._seam.chunk_blocks and other._seam.chunks() == plain._seam.chunks()
        for l in range(2):
            for have, want in ((other.aggregates(l), plain.aggregates(l)), *zip(other.members(l), plain.members(l)), *zip(other.pattern(l + 1), plain.pattern(l + 1))):
                assert have.dtype == want.dtype and np.array_equal(have, want)
    assert multilevel.free_program(3, 8) == '#define FCAMD_MF_D 3\n#define FCAMD_MF_A 8\n#include "multilevel_free.hip"\n'
    assert multilevel.lds_bytes(multilevel.FREE_GALERKIN_KERNEL) == 0
    with pytest.raises(ValueError, match="rigid_body"):
        named.positions(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the oracle's values of level 1 against the assembled rigid-body route
# ---------------------------------------------------------------------------------------------------------------------------------
def level1_case(shape, n_cells, seed, integer, affine, aggregate=True):
    """(tables, mask, hierarchy, offsets of level 0): random tables and coordinates with random constrained dofs, every dof of the
    nodes of one cell constrained and (``aggregate``) every dof of the members of aggregate 0"""
    d_ = SHAPES[shape][0]
    t = distinct_inputs(shape, n_cells, seed, integer, affine, every_node=True)
    indptr, indices = matrix.block_pattern(t["dofmap"], t["n_nodes"])
    levels = MU.hierarchy(indptr, indices, 1)
    mask = random_mask(t, d_, seed + 1, whole_cell=n_cells // 2)
    if aggregate:
        mask |= np.repeat(levels[0].agg == 0, d_)
    rng = np.random.default_rng(seed + 77)
    x = rng.integers(-4, 5, size=(t["n_nodes"], d_)).astype(np.float64) if integer else rng.normal(size=(t["n_nodes"], d_))
    return t, mask, levels, RU.place(levels, x)[1][0]


def assembled_level1(t, levels, offsets, mask, blocks=None):
    """rigid_body_util's Galerkin step applied to the assembled matrix of the same tangent and constraints"""
    fine = levels[0]
    if blocks is None:
        _, _, blocks = matrix_oracle(t["tangent"], *tables_of(t), constrained=mask)
    rows = np.repeat(np.arange(fine.indptr.size - 1), np.diff(fine.indptr))
    return RU.galerkin(fine.folds, blocks, rows, fine.indices, RU.p_blocks(offsets, offsets.shape[1]))


def assert_within_the_bound(have, want, size, chain, what):
    error = np.abs(have - want)
    print(f"{what}: largest |difference| / bound {np.max(error / np.maximum((chain + 2) * FR.EPS * size, 1e-300)):.4f}, longest chain {chain} operations, "
          f"share of the largest entry {error.max() / np.abs(want).max():.1e}")
    assert (error <= (chain + 2) * FR.EPS * size).all() and np.abs(want).max() > 0, what


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_oracle_level_one_against_the_assembled_route(shape):
    """Both routes sum the same terms -- P_i[a'][r] ke[c][a][a'][b][b'] P_j[b'][s] with ke on the bits of matrix_util.element_matrices,
    and P_i[a][r] 1.0 P_i[a][s] per constrained dof on a coarse diagonal -- in two orders: the fine block first and the triple
    product over the fold list, or the triple product per contribution in one chain.  A term passes through at most n floating-point
    operations on either route (multilevel_free_rigid_util.longest_chain: two products, 2 D sums, the sums of f), so each value is
    within n 2^-53 S of the exact sum (first order), the two within n 2^-52 S of each other; the bound used is (n + 2) 2^-52 S with S
    the oracle's own sum with every factor replaced by its absolute value."""
    d_, a_, q_, affine = SHAPES[shape]
    for per_point in (affine, not affine):
        for aggregate in (True, False):  # (False: random constrained dofs and a wholly constrained cell only)
            t, mask, levels, offsets = level1_case(shape, 40, 5, False, per_point, aggregate)
            fine, coarse = levels[0], levels[1]
            assert len(levels) >= 2 and mask.reshape(-1, d_)[t["dofmap"][20]].all() and mask.reshape(-1, d_)[fine.agg == 0].all() == aggregate
            args = (t["tangent"], *tables_of(t), fine.agg, coarse.indptr, coarse.indices, offsets)
            chain = FR.longest_chain(t["dofmap"], fine.agg, coarse.indptr, coarse.indices, d_)
            have, size = FR.level1_values(*args, mask=mask), FR.level1_values(*args, mask=mask, absolute=True)
            assert have.shape == (coarse.indices.size, RU.coarse_dofs(d_), RU.coarse_dofs(d_))
            assert_within_the_bound(have, assembled_level1(t, levels, offsets, mask), size, chain, f"{shape} affine={per_point} aggregate={aggregate}")
            if aggregate:  # the aggregate whose dofs are all constrained: its coarse diagonal block is the sum of P_i^T P_i, its other blocks are +0.0
                rows1 = np.repeat(np.arange(coarse.indptr.size - 1), np.diff(coarse.indptr))
                p = RU.p_blocks(offsets, d_)
                for k in np.flatnonzero((rows1 == 0) | (coarse.indices == 0)):
                    if rows1[k] == 0 and coarse.indices[k] == 0:
                        own = sum(p[i].T @ p[i] for i in np.flatnonzero(fine.agg == 0))
                        assert np.abs(have[k] - own).max() <= 4 * d_ * (fine.agg == 0).sum() * FR.EPS * np.abs(own).max(), k
                    else:
                        assert (bits(have[k]) == 0).all(), k
        # without a mask: the plain sums
        plain = FR.level1_values(*args)
        assert_within_the_bound(plain, assembled_level1(t, levels, offsets, None), FR.level1_values(*args, absolute=True), chain, f"{shape}: no mask")
        # and the start's loop, skipped without a mask, adds only 0.0 under a mask that holds nothing: the same bits
        assert np.array_equal(bits(FR.level1_values(*args, mask=np.zeros_like(mask))), bits(plain))


def test_oracle_level_one_on_a_mesh():
    """the same comparison where the aggregates are many: Cube(3, 2, 4) under the tension constraints (levels 60, 4 at
    coarsest_nodes=4; the preconditioner built on the operator holds the same offsets)"""
    from solver_util import spd_tangent

    mesh = FE.Cube(3, 2, 4)
    tables = cube_tables(mesh)
    mask, _ = tension_constraints(mesh)
    tangent = spd_tangent(mesh.n_points, 6, 1, False)
    o = FR.FreeRigidOracle(*tables, mesh.nodes, mask=mask, coarsest_nodes=4).setup(tangent)
    fine, coarse = o.levels[0], o.levels[1]
    assert [lv.indptr.size - 1 for lv in o.levels] == [60, 4] and not o.singular and o.values[1].shape == (coarse.indices.size, 6, 6)
    indptr, indices, blocks = matrix_oracle(tangent, *tables, constrained=mask)
    want = RU.Oracle(indptr, indices, mesh.nodes, coarsest_nodes=4, mask=mask).setup(blocks)
    size = FR.level1_values(tangent, *tables, fine.agg, coarse.indptr, coarse.indices, o.offsets[0], mask=mask, absolute=True)
    chain = FR.longest_chain(tables[0], fine.agg, coarse.indptr, coarse.indices, 3)
    assert_within_the_bound(o.values[1], want.values[1], size, chain, "Cube(3, 2, 4)")
    assert np.array_equal(bits(o.diagonal), bits(blocks[np.flatnonzero(np.repeat(np.arange(60), np.diff(indptr)) == indices)]))  # level 0: the matrix's own blocks
    pc = fc.MultilevelPreconditioner(fc.TangentOperator(cube_operators(mesh)[1]), coarsest_nodes=4, coarse_space="rigid_body", coordinates=mesh.nodes)
    assert np.array_equal(bits(pc.offsets(0)), bits(o.offsets[0])) and np.array_equal(pc.aggregates(0), fine.agg)
    chunked = FR.FreeRigidOracle(*tables, mesh.nodes, mask=mask, coarsest_nodes=4, chunk_cells=5).setup(tangent)
    assert np.array_equal(bits(chunked.diagonal), bits(o.diagonal)) and np.array_equal(bits(chunked.values[1]), bits(o.values[1]))


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_oracle_level_one_does_not_depend_on_the_chunks(shape):
    d_, a_, q_, affine = SHAPES[shape]
    n_cells = 11
    t, mask, levels, offsets = level1_case(shape, n_cells, 9, False, affine)
    args = (t["tangent"], *tables_of(t), levels[0].agg, levels[1].indptr, levels[1].indices, offsets)
    for m in (None, mask):
        want = FR.level1_values(*args, mask=m)
        for chunk in (1, 2, n_cells - 1, n_cells):
            assert np.array_equal(bits(FR.level1_values(*args, mask=m, chunk_cells=chunk)), bits(want)), (shape, chunk)
        assert np.abs(want).max() > 0


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_oracle_level_one_is_exact_on_integers(shape):
    """Element matrices and offsets of small integers (integer coordinates whose aggregate means are integers: the offsets are taken
    as integers directly): every product and sum of both routes is exact, so the two orders of summation give the same number."""
    from matrix_util import apply_constraints, block_sums

    d_, a_, q_, affine = SHAPES[shape]
    n_cells = 12
    t, mask, levels, _ = level1_case(shape, n_cells, 14, True, affine)
    indptr, indices = matrix.block_pattern(t["dofmap"], t["n_nodes"])
    rng = np.random.default_rng(3)
    ke = rng.integers(-8, 9, size=(n_cells, a_, d_, a_, d_)).astype(np.float64)
    offsets = rng.integers(-4, 5, size=(t["n_nodes"], d_)).astype(np.float64)
    args = (None, *tables_of(t), levels[0].agg, levels[1].indptr, levels[1].indices, offsets)
    for m in (None, mask):
        blocks = block_sums(ke, t["dofmap"], t["n_nodes"], indptr, indices)
        if m is not None:
            blocks = apply_constraints(blocks, indptr, indices, m)
        have = FR.level1_values(*args, mask=m, chunk_cells=5, ke_all=ke)
        want = assembled_level1(t, levels, offsets, m, blocks=blocks)
        assert np.array_equal(have, want) and np.abs(have).max() > 0 and np.array_equal(have, np.round(have))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the property itself
# ---------------------------------------------------------------------------------------------------------------------------------
def test_level_one_annihilates_the_coarse_rigid_modes():
    """The FREE elastic Cube(3, 2, 4) (no mask): K has the six rigid-body modes in its kernel and P reproduces them, so the level-1
    matrix gathered from the element matrices times a coarse rigid mode is zero up to the rounding of the sums.  The bound is the one
    test_multilevel_rigid.py uses for the assembled route (ten times 1.8e-14 |K|_max): the same quantity in another order of summation."""
    mesh = FE.Cube(3, 2, 4)
    tables = cube_tables(mesh)
    tangent = elastic_tangent(mesh.n_points)
    o = FR.FreeRigidOracle(*tables, mesh.nodes, coarsest_nodes=1).setup(tangent)
    assert [lv.indptr.size - 1 for lv in o.levels] == [60, 4, 1]
    scale = np.abs(matrix_oracle(tangent, *tables)[2]).max()
    x0 = np.array([0.3, -0.2, 0.7])
    for l in (1, 2):
        lv = o.levels[l]
        modes = RU.rigid_modes(o.positions[l], x0, 6)
        worst = max(np.abs(matvec(lv.indptr, lv.indices, o.values[l], modes[:, c])).max() for c in range(6))
        print(f"level {l}: |K_l m| / |K|_max = {worst / scale:.3e}")
        assert worst <= 10 * 1.8e-14 * scale, (l, worst / scale)
    assert np.abs(o.values[1]).max() >= 0.1 * scale


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the Newton loops of the examples on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", CYCLES)
def test_oracle_conjugate_gradients_in_the_newton_loop(cycle):
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    tables = cube_tables(mesh)

    def cpu_state():
        return FE.CopyProtocolState(FE.OracleLaw(O.von_mises_3d, VM_P, {"eps_n": 6, "alpha": 1}), mesh.n_points)

    direct = FE.tension_test(mesh, cpu_state(), steps=8)
    loop = FR.oracle_loop(cpu_state(), *tables, mesh.nodes, rtol=1e-12, cycle=cycle, coarsest_nodes=8)
    reactions, norms, u, solves = tension_test_device_solve(mesh, loop, steps=8)
    counts = [len(h) for h in norms]
    difference = np.max(np.abs(reactions - direct[0])) / np.max(np.abs(direct[0]))
    print(f"oracle loop, operator + rigid body {cycle}: Newton iterations {counts}, conjugate-gradient iterations {solves}, "
          f"largest relative reaction difference to the direct solve {difference:.2e}")
    assert counts == [len(h) for h in direct[1]] == [2, 2, 2, 3, 3, 4, 5, 5]
    assert len(loop.systems) == len(solves) == sum(counts) - 8 and all(result.converged for _, _, result in loop.systems)
    assert difference <= 1e-8


@pytest.mark.parametrize("cycle", CYCLES)
def test_oracle_bicgstab_in_the_newton_loop_of_an_unsymmetric_law(cycle):
    from cube_tension_nonsymmetric import DP_P, TOP_DISPLACEMENT
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    tables = cube_tables(mesh)

    def cpu_state():
        return FE.CopyProtocolState(FE.OracleLaw(O.comfe_drucker_prager, DP_P, {"history": 7}), mesh.n_points)

    with np.errstate(all="ignore"):
        direct = FE.tension_test(mesh, cpu_state(), steps=8, top_displacement=TOP_DISPLACEMENT)
        loop = FR.oracle_loop(cpu_state(), *tables, mesh.nodes, solver="bicgstab", rtol=1e-12, cycle=cycle, coarsest_nodes=8)
        reactions, norms, u, solves = tension_test_device_solve(mesh, loop, steps=8, top_displacement=TOP_DISPLACEMENT)
    counts = [len(h) for h in norms]
    difference = np.max(np.abs(reactions - direct[0])) / np.max(np.abs(direct[0]))
    print(f"oracle loop, operator + rigid body {cycle}, BiCGStab: Newton iterations {counts}, BiCGStab iterations {solves}, "
          f"largest relative reaction difference to the direct solve {difference:.2e}")
    assert counts == [len(h) for h in direct[1]] == [2, 3, 3, 4, 6, 6, 6, 6]
    assert all(result.converged for _, _, result in loop.systems)
    c = loop.systems[-1][0].reshape(-1, 6, 6)
    assert np.abs(c - c.transpose(0, 2, 1)).max() >= 1e-3 * np.abs(c).max()  # the last tangent is not symmetric
    assert difference <= 1e-8


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the iteration counts
# ---------------------------------------------------------------------------------------------------------------------------------
#: conjugate-gradient iterations on the cube of 10^3 cells, (translations, rigid body) on the operator's oracle
PINNED = {"multiplicative": (61, 42), "additive": (123, 90)}


@pytest.mark.parametrize("cycle", CYCLES)
def test_fewer_iterations_than_the_translations(cycle):
    """The elastic cube with the tension test's constraints, a seeded normal right-hand side zeroed at the constrained dofs, rtol
    1e-8, coarsest_nodes 32 (the setting of test_multilevel_rigid.py, whose assembled route measured 6^3 cells: multiplicative 42 ->
    35, additive 80 -> 68; 10^3: multiplicative 61 -> 42, additive 123 -> 90): on the operator's oracles the rigid-body modes take
    strictly fewer iterations than the translations, with that margin."""
    for m in (6, 10):
        mesh = FE.Cube(m, m, m)
        tables = cube_tables(mesh)
        mask, _ = tension_constraints(mesh)
        tangent = elastic_tangent(mesh.n_points)
        b = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mask.size))
        plain = MF.conjugate_gradient(MF.FreeOracle(*tables, mask=mask, cycle=cycle, coarsest_nodes=32), tangent, b, rtol=1e-8)
        rigid = FR.conjugate_gradient(FR.FreeRigidOracle(*tables, mesh.nodes, mask=mask, cycle=cycle, coarsest_nodes=32), tangent, b, rtol=1e-8)
        print(f"cube of {m}^3 cells, {cycle}, operator: translations {plain.iterations}, rigid body {rigid.iterations}")
        assert plain.converged and rigid.converged
        assert rigid.iterations < plain.iterations, (m, cycle, plain.iterations, rigid.iterations)
        if m == 10:
            assert rigid.iterations <= 0.8 * plain.iterations  # (the assembled route: 0.69 and 0.73)
            assert (plain.iterations, rigid.iterations) == PINNED[cycle]
