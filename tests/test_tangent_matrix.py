"""The assembled tangent stiffness without a GPU (fenics_constitutive_amd.matrix, csrc/jit/tangent_matrix.hip): every shape
compiles for gfx950 without scratch at the register budget the ladder keeps, the sparsity pattern and the contribution lists, the
ordered oracle (matrix_util.py) against fe_mini's assembly, against the oracle of the tangent action and column by column on the
bits, the constraint rule, and the host-side validation."""

import os
import sys

import numpy as np
import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import gradient, jit, matrix

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import fe_mini  # noqa: E402
from fe_gpu_util import bits  # noqa: E402
from force_util import chain_length, random_inputs, tangent_action_oracle  # noqa: E402
from gradient_util import EPS, SHAPES, cube_operator_tables, oracle  # noqa: E402
from matrix_util import (apply_constraints, contributions, csr_values, matrix_oracle, max_contributions, pattern, to_bsr)  # noqa: E402

#: gradient_util's shapes, the odd ones of the force operator's tests and one with more than 64 columns (66: two passes)
ALL_SHAPES = dict({k: v[:3] for k, v in SHAPES.items()}, q3=(3, 4, 3), odd33_1d=(1, 2, 33), odd33_3d=(3, 4, 33), wide=(3, 22, 2))


def operators(shape, n_cells=3, affine=True, seed=0, **kwargs):
    t = random_inputs(ALL_SHAPES[shape] + (affine,), n_cells, seed, False, affine)
    op = fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"])
    f = fc.InternalForce(op, t["weights"])
    return fc.TangentMatrix(f, **kwargs), f, t


@pytest.mark.parametrize("affine", [True, False], ids=["per_cell", "per_point"])
@pytest.mark.parametrize("shape", list(ALL_SHAPES))
def test_every_shape_compiles_without_scratch(shape, affine):
    d_, a_, q_ = ALL_SHAPES[shape]
    k, _, _ = operators(shape, affine=affine)
    r = k.resources
    assert r["scratch_bytes"] == 0 and r["gather"]["scratch_bytes"] == 0, r
    assert r["waves"] in gradient.WAVES_LADDER and r["vgprs"] + (r["agprs"] or 0) <= 512 // r["waves"], r
    s_ = {1: 1, 2: 4, 3: 6}[d_]
    even = lambda n: (n + 1) // 2 * 2  # noqa: E731
    slab = r["slab"]
    region = even(slab * s_ * s_) + (0 if affine else even(slab * d_ * d_)) + even(slab * a_ * d_) + even(slab)
    assert r["lds_bytes"] == k.lds_bytes() == 8 * (even(d_ * a_ * q_) + 4 * region) <= gradient.LDS_CAP
    assert r["gather"]["lds_bytes"] == 0
    assert k.cells_per_tile == max(1, 64 // (a_ * d_)) and (shape != "wide" or a_ * d_ == 66)
    assert matrix.ELEMENT_KERNEL in k.compile_log and matrix.GATHER_KERNEL in k.compile_log


def test_same_shape_compiles_once():
    operators("tet_p2", n_cells=2, seed=1)
    before = jit.compile_count()
    k, _, _ = operators("tet_p2", n_cells=7, seed=2, format="csr", scratch_bytes=10**6)  # other mesh, format, scratch: the same program
    assert jit.compile_count() == before and k.resources["scratch_bytes"] == 0


def test_a_shape_that_does_not_fit_is_refused():
    assert matrix.lds_bytes(3, 8, 8, False, 16) == 37376
    before = jit.compile_count()
    with pytest.raises(ValueError, match="LDS"):
        matrix.compile_kernels(3, 64, 40, True)  # the reference table alone is 61440 bytes
    assert jit.compile_count() == before


def cube_case(seed):
    mesh = fe_mini.Cube(3, 2, 4)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    weights = gradient.integration_weights(mesh.nodes[mesh.cells], ref, np.ones(8))
    return mesh, dofmap, ref, jinv, weights, np.random.default_rng(seed)


def test_pattern_of_the_cube():
    mesh, dofmap, ref, jinv, weights, rng = cube_case(1)
    f = fc.InternalForce(fc.DisplacementGradient(dofmap, ref, jinv, mesh.n_nodes), weights)
    for fmt in matrix.FORMATS:
        k = fc.TangentMatrix(f, format=fmt)
        assert k.nnzb == 910 and k.shape == (mesh.n_dofs, mesh.n_dofs) and k.nnz == 9 * 910
        assert k.indptr.dtype == np.int32 and k.indices.dtype == np.int32 and k.indptr.shape == (mesh.n_nodes + 1,)
        assert np.diff(k.indptr).max() == 27 and np.diff(k.blk_ptr).max() == 8 and k.blk_ptr[-1] == dofmap.shape[0] * 64
        for v in range(mesh.n_nodes):
            row = k.indices[k.indptr[v]: k.indptr[v + 1]]
            assert (np.diff(row) > 0).all()  # ascending and unique
            assert k.indices[k.diag_block[v]] == v and k.indptr[v] <= k.diag_block[v] < k.indptr[v + 1]
        indptr, indices = pattern(dofmap, mesh.n_nodes)
        assert np.array_equal(indptr, k.indptr) and np.array_equal(indices, k.indices)
        order, block, rank = contributions(dofmap, mesh.n_nodes, indptr, indices)
        assert np.array_equal(order, k.contributions) and np.array_equal(np.bincount(block, minlength=910), np.diff(k.blk_ptr))
        for b in range(0, 910, 37):  # ascending within a block, and under the right pair of nodes
            mine = k.contributions[k.blk_ptr[b]: k.blk_ptr[b + 1]]
            assert (np.diff(mine) > 0).all()
            c, ab = mine // 64, mine % 64
            assert (dofmap[c, ab // 8] == k.block_row[b]).all() and (dofmap[c, ab % 8] == k.indices[b]).all()
        ref_csr = mesh.stiffness(rng.normal(size=36 * mesh.n_points))
        ref_csr.sort_indices()
        assert np.array_equal(k.csr_indptr, ref_csr.indptr) and np.array_equal(k.csr_indices, ref_csr.indices)
        # to_scipy of an ndarray: the two formats describe one matrix
        _, _, values = matrix_oracle(rng.normal(size=36 * mesh.n_points), dofmap, ref, jinv, weights, mesh.n_nodes)
        have = k.to_scipy(values.reshape(-1) if fmt == "bsr" else csr_values(indptr, indices, values))
        assert (have != to_bsr(indptr, indices, values, mesh.n_nodes)).nnz == 0


def test_pattern_of_random_tables():
    """the untouched node has an empty row; a cell that names a node twice contributes every pair"""
    k, f, t = operators("tet_p2", n_cells=9, seed=4)
    dofmap, lonely = t["dofmap"], t["lonely"]
    twice = [c for c in range(9) if np.unique(dofmap[c]).size < 10]
    assert twice, "the tables must hold a cell that names a node twice"
    assert k.indptr[lonely] == k.indptr[lonely + 1] and k.diag_block[lonely] == -1
    assert k.blk_ptr[-1] == 9 * 100 == k.contributions.size and np.array_equal(np.sort(k.contributions), np.arange(900))
    c = twice[0]
    node = [v for v in dofmap[c] if (dofmap[c] == v).sum() > 1][0]
    b = k.diag_block[node]
    mine = k.contributions[k.blk_ptr[b]: k.blk_ptr[b + 1]]
    assert (mine // 100 == c).sum() == (dofmap[c] == node).sum() ** 2  # (a, b), (a, a), (b, a), (b, b)
    # a global pattern: more blocks, the same lists; a pattern that misses a pair is refused
    wider = np.concatenate([dofmap, np.array([[lonely] * 10], dtype=np.int32)])
    kw = fc.TangentMatrix(f, pattern_dofmap=wider)
    assert kw.nnzb == k.nnzb + 1 and kw.diag_block[lonely] >= 0 and kw.blk_ptr[-1] == 900
    b = kw.diag_block[lonely]
    assert kw.blk_ptr[b] == kw.blk_ptr[b + 1]
    with pytest.raises(ValueError, match="missing"):
        fc.TangentMatrix(f, pattern_dofmap=np.ascontiguousarray(dofmap[:-1]))


def test_oracle_against_the_cube_stiffness():
    mesh, dofmap, ref, jinv, weights, rng = cube_case(8)
    cu = rng.normal(scale=1e4, size=(mesh.n_points, 6, 6))  # unsymmetric
    indptr, indices, values = matrix_oracle(cu.reshape(-1), dofmap, ref, jinv, weights, mesh.n_nodes)
    _, _, k_abs = matrix_oracle(cu.reshape(-1), dofmap, ref, jinv, weights, mesh.n_nodes, absolute=True)
    got = to_bsr(indptr, indices, values, mesh.n_nodes).toarray()
    want = mesh.stiffness(cu.reshape(-1)).toarray()
    assert chain_length(3, 8, 8, action=True) == 35
    bound = 35 * EPS * to_bsr(indptr, indices, k_abs, mesh.n_nodes).toarray()
    err = np.abs(got - want)
    assert (err <= bound).all(), (err[bound > 0] / bound[bound > 0]).max()
    print("oracle against Cube.stiffness: worst entry at", (err[bound > 0] / bound[bound > 0]).max(), "of the bound")
    _, _, vt = matrix_oracle(cu.transpose(0, 2, 1).reshape(-1).copy(), dofmap, ref, jinv, weights, mesh.n_nodes)
    wrong = to_bsr(indptr, indices, vt, mesh.n_nodes).toarray()
    assert err.max() <= 1e-12 * np.abs(want).max() < 1e-3 * np.abs(wrong - want).max()


@pytest.mark.parametrize("affine", [True, False], ids=["per_cell", "per_point"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_oracle_against_the_action(shape, affine):
    d_, a_, q_ = ALL_SHAPES[shape]
    worst = 0.0
    for n_cells in (1, 9, 40):
        t = random_inputs(shape, n_cells, 3 + n_cells, False, affine)
        tables = (t["dofmap"], t["ref"], t["jinv"], t["weights"], t["n_nodes"])
        indptr, indices, values = matrix_oracle(t["tangent"], *tables)
        _, _, k_abs = matrix_oracle(t["tangent"], *tables, absolute=True)
        v = np.random.default_rng(n_cells).normal(scale=1e-3, size=d_ * t["n_nodes"])
        got = to_bsr(indptr, indices, values, t["n_nodes"]) @ v
        want = tangent_action_oracle(t["tangent"], oracle(v, *tables[:3], "grad"), *tables, "grad")
        chain = chain_length(d_, q_, max_contributions(t["dofmap"], t["n_nodes"], indptr, indices), True) + d_ * int(np.diff(indptr).max()) + a_
        bound = chain * EPS * (to_bsr(indptr, indices, k_abs, t["n_nodes"]) @ np.abs(v))
        err = np.abs(got - want)
        assert (err <= bound).all(), (shape, n_cells, (err[bound > 0] / bound[bound > 0]).max())
        worst = max(worst, (err[bound > 0] / bound[bound > 0]).max())
        assert (values[indptr[t["lonely"]]: indptr[t["lonely"] + 1]].size == 0) and np.abs(want).max() > 0
    print(f"{shape} affine={affine}: K v against the action at most {worst:.3f} of the bound")


def test_columns_on_the_cube_on_the_bits():
    mesh, dofmap, ref, jinv, weights, rng = cube_case(9)
    cu = rng.normal(scale=1e4, size=36 * mesh.n_points)
    indptr, indices, values = matrix_oracle(cu, dofmap, ref, jinv, weights, mesh.n_nodes)
    dense = to_bsr(indptr, indices, values, mesh.n_nodes).toarray()
    for j in rng.choice(mesh.n_dofs, size=26, replace=False):
        unit = np.zeros(mesh.n_dofs)
        unit[j] = 1.0
        column = tangent_action_oracle(cu, oracle(unit, dofmap, ref, jinv, "grad"), dofmap, ref, jinv, weights, mesh.n_nodes, "grad")
        assert np.array_equal(bits(column + 0.0), bits(dense[:, j] + 0.0)), j  # (+ 0.0: an entry outside the pattern has no sign)
        assert np.abs(column).max() > 0


def test_constraint_rule():
    mesh, dofmap, ref, jinv, weights, rng = cube_case(10)
    cu = rng.normal(scale=1e4, size=36 * mesh.n_points)
    mask = rng.random(mesh.n_dofs) < 0.2
    indptr, indices, free = matrix_oracle(cu, dofmap, ref, jinv, weights, mesh.n_nodes)
    _, _, con = matrix_oracle(cu, dofmap, ref, jinv, weights, mesh.n_nodes, constrained=mask)
    a, b = to_bsr(indptr, indices, free, mesh.n_nodes).toarray(), to_bsr(indptr, indices, con, mesh.n_nodes).toarray()
    assert np.array_equal(b[mask][:, mask], np.eye(mask.sum())) and not b[mask][:, ~mask].any() and not b[~mask][:, mask].any()
    assert np.array_equal(bits(b[~mask][:, ~mask]), bits(a[~mask][:, ~mask]))
    assert np.array_equal(bits(apply_constraints(con, indptr, indices, mask)), bits(con))  # idempotent
    # a constrained dof needs a diagonal block to carry its 1.0
    k, f, t = operators("tet_p2", n_cells=9, seed=4)
    bad = np.zeros(k.shape[0], dtype=bool)
    bad[3 * t["lonely"] + 1] = True
    with pytest.raises(ValueError, match="diagonal block"):
        k.set_constrained(bad)
    bad[:] = False
    bad[0] = True
    k.set_constrained(bad)
    version = k._mask_version
    k.set_constrained(bad.copy())  # unchanged: no new upload
    assert k._mask_version == version
    k.set_constrained(None)
    assert k._mask is None and k._mask_version == version + 1


def test_validation_errors():
    torch = pytest.importorskip("torch")
    k, f, t = operators("tet_p2", n_cells=5, seed=3)
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        TM = fc.TangentMatrix
        with pytest.raises(TypeError):
            TM(f.op)  # not a force operator
        with pytest.raises(ValueError, match="format"):
            TM(f, format="coo")
        with pytest.raises(TypeError):
            TM(f, pattern_dofmap=t["dofmap"].astype(np.int64))
        with pytest.raises(TypeError):
            TM(f, pattern_dofmap=t["dofmap"].tolist())
        with pytest.raises(ValueError, match="pattern_dofmap"):
            TM(f, pattern_dofmap=t["dofmap"].reshape(-1))
        with pytest.raises(ValueError, match="pattern_dofmap"):
            TM(f, pattern_dofmap=t["dofmap"] + np.int32(t["n_nodes"]))
        with pytest.raises(ValueError, match="one tile"):
            TM(f, scratch_bytes=2 * 900 * 8 - 1)  # a tile of tet_p2 is two cells of 30 x 30 doubles
        TM(f, scratch_bytes=2 * 900 * 8)
        with pytest.raises(TypeError):
            TM(f, scratch_bytes=1e9)
        with pytest.raises(TypeError):
            k.set_constrained(np.zeros(k.shape[0], dtype=np.uint8))
        with pytest.raises(TypeError):
            k.set_constrained([False] * k.shape[0])
        with pytest.raises(ValueError, match="shape"):
            k.set_constrained(np.zeros(k.shape[0] + 1, dtype=bool))
        n = k.n_points
        with pytest.raises(TypeError):
            k(t["tangent"])  # an ndarray
        with pytest.raises(TypeError):
            k(torch.zeros(36 * n, dtype=torch.float32))
        with pytest.raises(ValueError, match="cuda"):
            k(torch.zeros(36 * n, dtype=torch.float64))  # on the host
        with pytest.raises(ValueError, match="accumulate"):
            k(torch.zeros(36 * n, dtype=torch.float64), accumulate=True)
        with pytest.raises(ValueError, match="cuda"):
            k.diagonal_blocks(torch.zeros(k.nnz, dtype=torch.float64))
        with pytest.raises(ValueError, match="entries"):
            k.to_scipy(np.zeros(k.nnz - 1))
    finally:
        jit.launch = real
    assert not launches
    assert not k._on and not k._scratch and not k._mask_on and not f._on and not f.op._on  # nothing was uploaded
    assert "TangentMatrix" in fc.__all__


def test_block_ranges_of_the_chunks():
    """a later chunk's gather visits the blocks between the first and the last its cells touch: every contribution lies inside"""
    mesh, dofmap, ref, jinv, weights, _ = cube_case(2)
    f = fc.InternalForce(fc.DisplacementGradient(dofmap, ref, jinv, mesh.n_nodes), weights)
    k = fc.TangentMatrix(f, scratch_bytes=6 * 576 * 8)  # chunks of six cells
    assert k.chunk_cells == 6 and len(k.chunks()) == 4 == len(k.chunk_blocks)
    block_of = np.repeat(np.arange(k.nnzb), np.diff(k.blk_ptr))
    for (c0, c1), (b0, b1) in zip(k.chunks(), k.chunk_blocks):
        mine = block_of[(k.contributions >= 64 * c0) & (k.contributions < 64 * c1)]
        assert mine.min() == b0 and mine.max() + 1 == b1 and 0 <= b0 < b1 <= k.nnzb
    assert k.chunk_blocks[1][0] > 0 and k.chunk_blocks[-2][1] < k.nnzb  # narrower than the whole pattern
