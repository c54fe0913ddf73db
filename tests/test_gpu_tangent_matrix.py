"""The assembled tangent stiffness on the GPU (fenics_constitutive_amd.TangentMatrix, csrc/jit/tangent_matrix.hip): the values of
the sparse matrix compared ON THE BITS with the ordered NumPy oracle of matrix_util.py, in both formats, under chunking, over
submeshes, with constraints; against the device's own tangent action; and in the Newton loop of
examples/cube_tension_assembled.py."""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_assembled import AssembledLoop, tension_test_assembled  # noqa: E402
from cube_tension_matrix_free import cube_operators  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import gradient, jit  # noqa: E402
from fenics_constitutive_amd import matrix as matrix_module  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402
from fenics_constitutive_amd.resident import ResidentState  # noqa: E402
from fe_gpu_util import CANARY, MARGIN, bits, guarded, assert_margins_intact, assert_same_bits  # noqa: E402
from fe_gpu_util import one_cu  # noqa: E402, F401 (the fixture: pytest finds it in this namespace)
from force_util import chain_length, random_inputs  # noqa: E402
from gradient_util import EPS, SHAPES, cube_operator_tables  # noqa: E402
from matrix_util import (csr_values, diagonal_blocks, matrix_oracle, max_contributions, oracle_matrix_loop, to_bsr)  # noqa: E402

#: gradient_util's shapes, the odd ones of the force operator's tests and one with more than 64 columns (66: two passes)
ALL_SHAPES = dict({k: v[:3] for k, v in SHAPES.items()}, q3=(3, 4, 3), odd33_1d=(1, 2, 33), odd33_3d=(3, 4, 33), wide=(3, 22, 2))
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}


def inputs(shape, n_cells, seed, integer, affine):
    t = random_inputs(ALL_SHAPES[shape] + (affine,), n_cells, seed, integer, affine)
    assert t["dofmap"].min() == 0 and t["dofmap"].max() == t["n_nodes"] - 1 and not (t["dofmap"] == t["lonely"]).any()
    return t


def build(t, **kwargs):
    op = fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"])
    f = fc.InternalForce(op, t["weights"])
    return fc.TangentMatrix(f, **kwargs), f, op


def tables(t):
    return t["dofmap"], t["ref"], t["jinv"], t["weights"], t["n_nodes"]


def random_mask(t, d_, fraction, seed):
    """a random set of constrained dofs on the nodes some cell touches (the others have no diagonal block to carry the 1.0)"""
    used = np.bincount(t["dofmap"].reshape(-1), minlength=t["n_nodes"]) > 0
    assert not used[t["lonely"]]
    mask = (np.random.default_rng(seed).random(d_ * t["n_nodes"]) < fraction) & np.repeat(used, d_)
    assert mask.any() and not mask.all()
    return mask


def in_format(fmt, indptr, indices, values):
    """the oracle's [nnzb][D][D] in the order of the format"""
    return values.reshape(-1) if fmt == "bsr" else csr_values(indptr, indices, values)


def to_blocks(fmt, indptr, indices, flat, d_):
    """the inverse of in_format"""
    if fmt == "bsr":
        return flat.reshape(-1, d_, d_)
    perm = csr_values(indptr, indices, np.arange(flat.size, dtype=np.float64).reshape(-1, d_, d_)).astype(np.int64)
    out = np.empty(flat.size)
    out[perm] = flat
    return out.reshape(-1, d_, d_)


def assemble(k, t, fill=None, accumulate=False):
    """values on the host, out of a buffer with canary margins that are checked"""
    buf, out = guarded(k.nnz, fill=fill)
    got = k(to_device(t["tangent"], "cuda"), out=out, accumulate=accumulate)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert_margins_intact(buf, k.nnz)
    return to_host(out)


def run_and_compare(shape, n_cells, affine, integer, seed, formats=matrix_module.FORMATS, **kwargs):
    t = inputs(shape, n_cells, seed, integer, affine)
    d_ = ALL_SHAPES[shape][0]
    indptr, indices, want = matrix_oracle(t["tangent"], *tables(t))
    start = np.random.default_rng(seed).integers(-5, 6, size=want.shape).astype(np.float64)
    _, _, want_on_top = matrix_oracle(t["tangent"], *tables(t), start=start)
    for fmt in formats:
        k, _, _ = build(t, format=fmt, **kwargs)
        what = f"{shape} cells={n_cells} {fmt} affine={affine} integer={integer} {kwargs}"
        assert np.array_equal(k.indptr, indptr) and np.array_equal(k.indices, indices)
        assert k.indptr[t["lonely"]] == k.indptr[t["lonely"] + 1], f"{what}: the row of the node no cell touches is not empty"
        assert_same_bits(assemble(k, t), in_format(fmt, indptr, indices, want), what)
        have = assemble(k, t, fill=in_format(fmt, indptr, indices, start), accumulate=True)
        assert_same_bits(have, in_format(fmt, indptr, indices, want_on_top), what + " accumulate")
        assert_same_bits(to_blocks(fmt, indptr, indices, have, d_), want_on_top, what + " accumulate, as blocks")
    return k


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. every shape, both formats, per-cell and per-point inverse Jacobians, the sizes around a tile of the element kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["per_cell", "per_point"])
@pytest.mark.parametrize("shape", list(ALL_SHAPES))
def test_bits_of_the_ordered_oracle(shape, affine):
    d_, a_, q = ALL_SHAPES[shape]
    cw = matrix_module.cells_per_tile(d_, a_)
    assert cw == max(1, 64 // (a_ * d_)) and (shape != "wide" or (cw == 1 and a_ * d_ > 64))
    for n_cells in sorted({1, max(cw - 1, 1), cw, cw + 1, 2 * cw + 1, -(-257 // q)}):
        for integer in (True, False):
            k = run_and_compare(shape, n_cells, affine, integer, seed=n_cells + 7 * integer)
    assert k.cells_per_tile == cw and len(k.chunks()) == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the grid-stride loops of both kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,affine", [("hex8", False), ("q5", True), ("tet_p2", True), ("tri_p2", False)])
def test_grid_stride_loops(shape, affine, one_cu):
    d_, a_, q = ALL_SHAPES[shape]
    cw = matrix_module.cells_per_tile(d_, a_)
    waves = gradient.BLOCKS_PER_CU * 4  # tiles all waves of the capped grid cover in one trip
    # two whole trips, five more whole tiles and a short one
    n_cells = (2 * waves + 5) * cw + cw // 2
    assert cw // 2 >= 1 and n_cells // cw == 2 * waves + 5 and n_cells % cw
    for integer in (True, False):
        k = run_and_compare(shape, n_cells, affine, integer, seed=3, formats=("csr",) if integer else ("bsr",))
    assert k.nnz > 2 * gradient.BLOCKS_PER_CU * 256  # the gather kernel: more entries than two trips of the capped grid cover
    assert {name for name, _ in one_cu} == {matrix_module.ELEMENT_KERNEL, matrix_module.GATHER_KERNEL}
    assert all(b == gradient.BLOCKS_PER_CU for _, b in one_cu), one_cu  # the launches really were capped


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the scratch between the kernels is bounded: the same bits for every chunk size
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,affine", [("hex8", False), ("tet_p2", True)])
def test_chunk_invariance(shape, affine):
    d_, a_, q = ALL_SHAPES[shape]
    cw, m = matrix_module.cells_per_tile(d_, a_), a_ * d_
    n_cells = 2 * 5 * cw + 3  # chunks of five tiles: two whole ones and a short one
    t = inputs(shape, n_cells, 17, False, affine)
    mask = random_mask(t, d_, 0.15, 2)
    for fmt in matrix_module.FORMATS:
        whole, _, _ = build(t, format=fmt)
        assert len(whole.chunks()) == 1
        want = assemble(whole, t)
        indptr, indices, oracle_values = matrix_oracle(t["tangent"], *tables(t))
        assert_same_bits(want, in_format(fmt, indptr, indices, oracle_values), f"{shape} {fmt} unchunked")
        start = np.random.default_rng(3).normal(size=whole.nnz)
        whole.set_constrained(mask)
        want_constrained = assemble(whole, t, fill=start, accumulate=True)
        for scratch, chunks in ((5 * cw * m * m * 8 + 8, 3), (cw * m * m * 8, -(-n_cells // cw))):
            k, _, _ = build(t, format=fmt, scratch_bytes=scratch)
            assert len(k.chunks()) == chunks and k.chunks()[-1][1] == n_cells and k.chunks()[-1][1] - k.chunks()[-1][0] < k.chunk_cells
            assert_same_bits(assemble(k, t), want, f"{shape} {fmt} in {chunks} chunks")
            k.set_constrained(mask)
            assert_same_bits(assemble(k, t, fill=start, accumulate=True), want_constrained, f"{shape} {fmt} in {chunks} chunks, constrained, on top")
            assert k._scratch[k.device].numel() == k.chunk_cells * m * m  # the scratch is what was asked for


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. two operators on the two halves of one mesh, into one global pattern
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,affine", [("hex8", False), ("tet_p2", True)])
def test_submeshes_into_one_pattern(shape, affine):
    d_, a_, q = ALL_SHAPES[shape]
    s2 = {1: 1, 2: 4, 3: 6}[d_] ** 2
    n_cells, cut = 31, 13
    t = inputs(shape, n_cells, 23, False, affine)
    for fmt in matrix_module.FORMATS:
        whole, _, _ = build(t, format=fmt)
        want = assemble(whole, t)
        buf, out = guarded(whole.nnz)
        for part, cells in enumerate((slice(0, cut), slice(cut, n_cells))):
            sub = dict(t, dofmap=np.ascontiguousarray(t["dofmap"][cells]), jinv=np.ascontiguousarray(t["jinv"][cells]),
                       weights=np.ascontiguousarray(t["weights"][cells]),
                       tangent=np.ascontiguousarray(t["tangent"].reshape(n_cells, q * s2)[cells]).reshape(-1))
            k, _, _ = build(sub, format=fmt, pattern_dofmap=t["dofmap"])
            assert np.array_equal(k.indptr, whole.indptr) and np.array_equal(k.indices, whole.indices)
            k(to_device(sub["tangent"], "cuda"), out=out, accumulate=part > 0)
            torch.cuda.synchronize()
            if part == 0:
                untouched = np.flatnonzero(np.diff(k.blk_ptr) == 0)
                assert untouched.size, "the second half must own some blocks alone"
                first = to_blocks(fmt, k.indptr, k.indices, to_host(out), d_)
                assert (bits(first[untouched]) == 0).all(), "a block the first operator does not touch is not +0.0"
        assert_same_bits(to_host(out), want, f"{shape} {fmt}: two submeshes")
        assert_margins_intact(buf, whole.nnz)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. Dirichlet rows and columns in the same pass
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", matrix_module.FORMATS)
def test_constraints_on_the_device(fmt):
    t = inputs("hex8", 29, 31, False, False)
    k, _, _ = build(t, format=fmt)
    n_dofs = 3 * t["n_nodes"]
    free_values = assemble(k, t)
    mask = random_mask(t, 3, 0.25, 6)
    k.set_constrained(mask)
    have = assemble(k, t)
    indptr, indices, want = matrix_oracle(t["tangent"], *tables(t), constrained=mask)
    assert_same_bits(have, in_format(fmt, indptr, indices, want), f"{fmt}: constrained")
    a, b = k.to_scipy(free_values).toarray(), k.to_scipy(have).toarray()
    assert np.array_equal(b[mask][:, mask], np.eye(mask.sum())) and not b[mask][:, ~mask].any() and not b[~mask][:, mask].any()
    assert np.array_equal(bits(b[~mask][:, ~mask] + 0.0), bits(a[~mask][:, ~mask] + 0.0))  # (+ 0.0: outside the pattern there is no sign)
    # twice on top of itself: the constrained entries are constants, the free ones have been added to
    again = assemble(k, t, fill=have, accumulate=True)
    _, _, want2 = matrix_oracle(t["tangent"], *tables(t), constrained=mask, start=want)
    assert_same_bits(again, in_format(fmt, indptr, indices, want2), f"{fmt}: constrained, on top of itself")
    hit = bits(again) != bits(have)
    assert hit.any() and (bits(again)[~hit] == bits(have)[~hit]).all()
    b2 = k.to_scipy(again).toarray()
    assert np.array_equal(b2[mask][:, mask], np.eye(mask.sum())) and (bits(b2[mask][:, ~mask]) == 0).all() and (bits(b2[~mask][:, mask]) == 0).all()
    # without the mask again
    k.set_constrained(None)
    assert_same_bits(assemble(k, t), free_values, f"{fmt}: the mask taken off")
    with pytest.raises(ValueError, match="diagonal block"):
        k.set_constrained(np.arange(n_dofs) == 3 * t["lonely"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the node's own blocks
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,affine", [("hex8", False), ("tri_p2", True), ("interval", True)])
def test_diagonal_blocks(shape, affine):
    d_ = ALL_SHAPES[shape][0]
    t = inputs(shape, 19, 41, False, affine)
    indptr, indices, want = matrix_oracle(t["tangent"], *tables(t))
    for fmt in matrix_module.FORMATS:
        k, _, _ = build(t, format=fmt)
        values = k(to_device(t["tangent"], "cuda"))
        blocks = k.diagonal_blocks(values)
        assert blocks.is_cuda and tuple(blocks.shape) == (t["n_nodes"], d_, d_)
        have = to_host(blocks)
        assert_same_bits(have, diagonal_blocks(indptr, indices, want), f"{shape} {fmt}: diagonal blocks")
        assert (bits(have[t["lonely"]]) == 0).all() and np.abs(have).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. against the device's own tangent action
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,affine", [("hex8", False), ("tet_p2", True), ("tri_p2", True), ("interval", True)])
def test_against_the_tangent_action(shape, affine):
    d_, a_, q = ALL_SHAPES[shape]
    t = inputs(shape, 40, 43, False, affine)
    indptr, indices, _ = matrix_oracle(t["tangent"], *tables(t))
    _, _, k_abs = matrix_oracle(t["tangent"], *tables(t), absolute=True)
    v = np.random.default_rng(8).normal(scale=1e-3, size=d_ * t["n_nodes"])
    chain = chain_length(d_, q, max_contributions(t["dofmap"], t["n_nodes"], indptr, indices), True) + d_ * int(np.diff(indptr).max()) + a_
    bound = chain * EPS * (to_bsr(indptr, indices, k_abs, t["n_nodes"]) @ np.abs(v))
    for fmt in matrix_module.FORMATS:
        k, f, op = build(t, format=fmt)
        tangent = to_device(t["tangent"], "cuda")
        got = k.to_scipy(k(tangent)) @ v
        want = to_host(f.tangent_action(tangent, op(v)))
        err = np.abs(got - want)
        print(f"{shape} {fmt}: K v against tangent_action at most {(err[bound > 0] / bound[bound > 0]).max():.3f} of the bound")
        assert (err <= bound).all() and np.abs(want).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the Newton loop with the assembled matrix
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear_elasticity", "von_mises_3d"])
def test_in_the_loop_behind_a_resident_state(kind):
    """The example's loop reproduces the Newton iteration counts of fe_mini.tension_test.  The reaction tolerance: the host direct
    solve and the assembled loop differ on the CPU (same law -- the NumPy oracle --, the oracle matrix) by ``delta`` relative to
    the largest reaction, from the other order of the sums in the matrix and in the factorisation; the GPU run is allowed ten times
    that against the host direct solve: the factor covers the device law's rounding, not another algorithm.  The block-Jacobi
    preconditioner of diagonal_blocks must lower the conjugate-gradient iterations of every solve.
    Measured on the CPU: delta = 3.6e-16 (von_mises_3d)."""
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    n = mesh.n_points
    if kind == "von_mises_3d":
        oracle_law, hist, law = O.von_mises_3d, {"eps_n": 6, "alpha": 1}, fc.VonMises3D(VM_P)
        params = VM_P
    else:
        params = {"E": 42.0, "nu": 0.3}
        oracle_law, hist, law = O.linear_elasticity, None, fc.LinearElasticityModel(params, fc.StressStrainConstraint.FULL)

    def cpu_state():
        return FE.CopyProtocolState(FE.OracleLaw(oracle_law, params, hist), n)

    r_direct, norms_direct, _ = FE.tension_test(mesh, cpu_state(), steps=8)
    op, f = cube_operators(mesh)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    r_cpu, norms_cpu, _, _ = tension_test_assembled(mesh, oracle_matrix_loop(cpu_state(), dofmap, ref, jinv, f._weights, mesh.n_nodes), steps=8,
                                                    compare_cg=False)
    scale = np.max(np.abs(r_direct))
    delta = np.max(np.abs(r_cpu - r_direct)) / scale
    loop = AssembledLoop(ResidentState(law, n, placement="torch"), op, f, fc.TangentMatrix(f, format="csr"))
    r_gpu, norms_gpu, u, solves = tension_test_assembled(mesh, loop, steps=8)  # (raises where a load step does not converge)
    difference = np.max(np.abs(r_gpu - r_direct)) / scale
    counts = [len(h) for h in norms_gpu]
    print(f"assembled tension test, {kind}: delta (CPU, oracle matrix against direct) {delta:.3e}, GPU against direct {difference:.3e}, "
          f"Newton iterations {counts}, conjugate-gradient iterations (plain, block-Jacobi) {solves}")
    assert counts == [len(h) for h in norms_direct] == [len(h) for h in norms_cpu]
    if kind == "von_mises_3d":
        assert counts == [2, 2, 2, 3, 3, 4, 5, 5]
    assert loop.assemblies == len(solves) == sum(counts) - 8
    assert all(jacobi < plain for plain, jacobi in solves), solves
    assert difference <= 10 * delta, (difference, delta)


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. refusals come before any launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    t = inputs("hex8", 21, 11, False, False)
    k, f, op = build(t)
    n, nnz = k.n_points, k.nnz
    tangent = to_device(t["tangent"], "cuda")
    k.diagonal_blocks(k(tangent))  # tables uploaded, kernels loaded: what follows can only add launches
    buf, out = guarded(nnz)
    spare = torch.zeros(max(2 * 36 * n + 2, 2 * nnz), dtype=torch.float64, device="cuda")
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        with pytest.raises(ValueError, match="aligned"):
            k(tangent, out=buf[MARGIN + 1: MARGIN + 1 + nnz])
        with pytest.raises(ValueError, match="entries"):
            k(tangent, out=buf[MARGIN: MARGIN + nnz - 9])
        with pytest.raises(ValueError, match="contiguous"):
            k(tangent, out=spare[: 2 * nnz: 2])
        with pytest.raises(ValueError, match="cuda"):
            k(tangent, out=torch.empty(nnz, dtype=torch.float64))  # on the host
        with pytest.raises(TypeError):
            k(tangent, out=out.float())
        with pytest.raises(ValueError, match="accumulate"):
            k(tangent, accumulate=True)
        with pytest.raises(ValueError, match="entries"):
            k(tangent[:-36], out=out)
        with pytest.raises(ValueError, match="aligned"):
            k(spare[1: 1 + 36 * n], out=out)
        with pytest.raises(ValueError, match="contiguous"):
            k(spare[: 72 * n: 2], out=out)
        with pytest.raises(ValueError, match="cuda"):
            k(tangent.cpu(), out=out)
        with pytest.raises(TypeError):
            k(t["tangent"], out=out)
        with pytest.raises(TypeError):
            k(tangent.float(), out=out)
        with pytest.raises(ValueError, match="entries"):
            k.diagonal_blocks(buf[MARGIN: MARGIN + nnz - 9])
        with pytest.raises(ValueError, match="format"):
            fc.TangentMatrix(f, format="ell")
        with pytest.raises(ValueError, match="one tile"):
            fc.TangentMatrix(f, scratch_bytes=8)
        with pytest.raises(ValueError, match="diagonal block"):
            k.set_constrained(np.arange(3 * t["n_nodes"]) == 3 * t["lonely"] + 2)
        if torch.cuda.device_count() > 1:
            with pytest.raises(ValueError, match="cuda"):
                k(tangent.to("cuda:1"), out=out)
    finally:
        jit.launch = real
    torch.cuda.synchronize()
    assert not launches
    assert (bits(to_host(buf)) == CANARY).all()
    # an empty mesh under a global pattern: zeros, or out as it is under accumulate, the constrained constants in both
    t0 = inputs("hex8", 1, 2, False, False)
    empty_f = fc.InternalForce(fc.DisplacementGradient(t0["dofmap"][:0], t0["ref"], t0["jinv"][:0], t0["n_nodes"]), t0["weights"][:0])
    empty = fc.TangentMatrix(empty_f, pattern_dofmap=t0["dofmap"])
    none = torch.zeros(0, dtype=torch.float64, device="cuda")
    assert empty.nnzb == np.unique(t0["dofmap"]).size ** 2 and (bits(to_host(empty(none))) == 0).all()
    start = np.arange(float(empty.nnz))
    keep = to_device(start, "cuda")
    assert empty(none, out=keep, accumulate=True) is keep and np.array_equal(to_host(keep), start)
    mask = np.zeros(3 * t0["n_nodes"], dtype=bool)
    mask[3 * int(t0["dofmap"][0, 0])] = True
    empty.set_constrained(mask)
    have = empty.to_scipy(empty(none, out=keep, accumulate=True)).toarray()
    assert have[mask][:, mask] == 1.0 and not have[mask][:, ~mask].any() and not have[~mask][:, mask].any()
    # and with no pattern at all
    nothing = fc.TangentMatrix(empty_f)
    assert nothing.nnz == 0 and nothing(none).numel() == 0 and to_host(nothing.diagonal_blocks(nothing(none))).shape == (t0["n_nodes"], 3, 3)
