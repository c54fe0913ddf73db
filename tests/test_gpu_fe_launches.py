"""The launches of the finite-element operators, pinned: for every kernel ``DisplacementGradient``, ``InternalForce``,
``TangentMatrix``, ``TangentOperator`` and the first Galerkin step of ``MultilevelPreconditioner`` on an operator enqueue, the
kernel's name, the number of blocks and the fields of its argument structure -- the integers as they are, the pointers into
``tangent``, ``jinv``, ``weights``, the scratch and the output as the address the formula gives.  The bit tests of the other
files cannot see a chunk that starts at the wrong cell when the kernel is handed the matching pointer, a launch of one block
where none is due, or a grid that is not capped.  What is expected is computed HERE from the formulas of the module docstrings:

* the cap of every grid: ``BLOCKS_PER_CU * num_cu``; "a wave per tile, 4 waves per block": ``min((tiles + 3) // 4, cap)``; "a lane
  per entry": ``min((n + 255) // 256, cap)``, with ``max(1, .)`` around it where the module has it (the operator's diagonal node
  kernel and its node kernel, every launch of the multilevel preconditioner; not the matrix's gather, not the force's node kernel);
* the chunks: ascending ranges of ``chunk_cells = scratch_bytes // bytes_per_cell // cells_per_tile * cells_per_tile`` cells; of chunk
  ``(c0, c1)`` the element kernel gets ``tangent + 8 S*S Q c0``, ``jinv + 8 D*D (1 | Q) c0``, ``weights + 8 Q c0``, the scratch's
  base and ``c1 - c0`` cells; the consumer ``key_lo, key_hi = c0 A*A, c1 A*A`` (the operator's diagonal kernel: ``c0 A, c1 A``),
  ``cell0 = c0``, ``first`` in the first chunk alone, and in a later chunk the range of blocks its cells touch (``entry0 / n_entries``
  in entries of ``D*D`` per block, ``block0 / block1`` in blocks for the rigid-body gather).

Meshes: no cell, one cell, and ``2 * 5 * CW + 3`` cells with a scratch of five tiles (three chunks, the last one short) and of
exactly one tile; trilinear hexahedra with per-point inverse Jacobians and quadratic tetrahedra with per-cell ones.  Everything
runs once as the device is and once with ``jit.num_cu`` patched to one compute unit."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import force, gradient, jit, matrix, multilevel, solver  # noqa: E402
from fenics_constitutive_amd import tangent_operator as to  # noqa: E402
from fenics_constitutive_amd.hostio import to_device  # noqa: E402
from tangent_operator_util import distinct_inputs, random_mask  # noqa: E402

#: name -> (D, A, Q, affine)
SHAPES = {"hex8": (3, 8, 8, False), "tet_p2": (3, 10, 4, True)}
MANDEL = {1: 1, 2: 4, 3: 6}


@pytest.fixture(params=[False, True], ids=["device", "one_cu"])
def recorded(request, monkeypatch):
    """``(launches, cap)``: every launch as (kernel, blocks, {field: value}) -- the fields copied at the launch, the structures are
    written again between launches --, and the cap of a grid"""
    launches = []
    real = jit.launch

    def launch(code, device, nblocks, args, what, kernel=None):
        launches.append((kernel or code.kernel, nblocks, {name: getattr(args, name) or 0 for name, _ in args._fields_}))
        return real(code, device, nblocks, args, what, kernel=kernel)

    if request.param:
        monkeypatch.setattr(jit, "num_cu", lambda dev: 1)
    monkeypatch.setattr(jit, "launch", launch)
    return launches, gradient.BLOCKS_PER_CU * jit.num_cu(0)


def trace(launches, call):
    del launches[:]
    result = call()
    torch.cuda.synchronize()
    return list(launches), result


def assert_launches(have, want, what):
    """``want``: (kernel, blocks, {field: value}) with the fields the formulas give; the others are not looked at"""
    assert [x[0] for x in have] == [x[0] for x in want], what
    for i, ((kernel, blocks, fields), (_, want_blocks, want_fields)) in enumerate(zip(have, want)):
        assert blocks == want_blocks, f"{what}: launch {i} ({kernel}) has {blocks} blocks, the formula {want_blocks}"
        got = {name: fields[name] for name in want_fields}
        assert got == want_fields, f"{what}: launch {i} ({kernel})"


def tables(shape, n_cells, seed, every_node=False):
    """distinct_inputs, or for no cell at all the empty tables of a mesh of A + 2 nodes"""
    d_, a_, q_, affine = SHAPES[shape]
    if n_cells:
        return distinct_inputs(SHAPES[shape], n_cells, seed, False, affine, every_node=every_node)
    rng = np.random.default_rng(seed)
    s_ = MANDEL[d_]
    return dict(dofmap=np.zeros((0, a_), dtype=np.int32), ref=rng.normal(size=(q_, a_, d_)), jinv=np.zeros((0, d_, d_) if affine else (0, q_, d_, d_)),
                n_nodes=a_ + 2, weights=np.zeros((0, q_)), stress=np.zeros(0), tangent=np.zeros(0), grad_v=np.zeros(0), du=rng.normal(size=d_ * (a_ + 2)))


def chunks_of(n_cells, chunk_cells):
    return [(c, min(c + chunk_cells, n_cells)) for c in range(0, n_cells, chunk_cells)]


def tile_blocks(cells, cells_per_tile, cap):
    """a wave per tile, 4 waves per block"""
    return min((-(-cells // cells_per_tile) + 3) // 4, cap)


def lane_blocks(n, cap):
    """a lane per entry"""
    return min((n + 255) // 256, cap)


def touched(nodes, n, indptr, indices, c0, c1):
    """the range of blocks of the pattern the node pairs of the cells ``c0 .. c1`` fall into"""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr.astype(np.int64)))
    pattern = rows * n + indices.astype(np.int64)
    d64 = nodes[c0:c1].astype(np.int64)
    block = np.searchsorted(pattern, (d64[:, :, None] * n + d64[:, None, :]).reshape(-1))
    return int(block.min()), int(block.max()) + 1


class Mesh:
    """the operators of one mesh on the device and the addresses the element kernels' pointers start from"""

    def __init__(self, shape, n_cells, seed, every_node=False):
        self.shape = shape
        self.t = t = tables(shape, n_cells, seed, every_node)
        self.d, self.a, self.q, self.affine = SHAPES[shape]
        self.n_cells, self.n_nodes = n_cells, t["n_nodes"]
        self.op = fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"])
        self.f = fc.InternalForce(self.op, t["weights"])
        self.tangent = to_device(t["tangent"], "cuda")
        self.dev = self.op.device

    def element(self, kernel, c0, c1, cells_per_tile, cap, scratch_name, scratch):
        """the element launch of the chunk ``(c0, c1)``"""
        s2, dd = MANDEL[self.d]**2, self.d * self.d
        jinv, weights = self.op._tables(self.dev)[2], self.f._tables(self.dev)[0]
        return (kernel, tile_blocks(c1 - c0, cells_per_tile, cap),
                {"tangent": self.tangent.data_ptr() + 8 * s2 * self.q * c0, "jinv": jinv.data_ptr() + 8 * dd * (1 if self.affine else self.q) * c0,
                 "weights": weights.data_ptr() + 8 * self.q * c0, "ref": self.op._tables(self.dev)[1].data_ptr(), scratch_name: scratch.data_ptr(),
                 "n_cells": c1 - c0})


# ---------------------------------------------------------------------------------------------------------------------------------
# what the formulas give
# ---------------------------------------------------------------------------------------------------------------------------------
def matrix_launches(m, k, out, cap, accumulate):
    d_, a_ = m.d, m.a
    cols = a_ * d_
    cw = max(1, 64 // cols)
    chunk_cells = k.scratch_bytes // (cols * cols * 8) // cw * cw
    mask = k._mask_table(m.dev)
    common = {"values": out.data_ptr(), "mask": 0 if mask is None else mask.data_ptr(), "accumulate": accumulate}
    if k.nnz == 0:
        return []
    if m.n_cells == 0:
        return [(matrix.GATHER_KERNEL, lane_blocks(k.nnz, cap), dict(common, ke=0, entry0=0, n_entries=k.nnz, key_lo=0, key_hi=0, cell0=0, first=1))]
    ke = k._scratch[m.dev]
    assert ke.numel() == min(chunk_cells, m.n_cells) * cols * cols
    want = []
    for i, (c0, c1) in enumerate(chunks_of(m.n_cells, chunk_cells)):
        want.append(m.element(matrix.ELEMENT_KERNEL, c0, c1, cw, cap, "ke", ke))
        lo, hi = (0, k.nnzb) if i == 0 else touched(m.t["dofmap"], m.n_nodes, k.indptr, k.indices, c0, c1)
        want.append((matrix.GATHER_KERNEL, lane_blocks(d_ * d_ * (hi - lo), cap),
                     dict(common, ke=ke.data_ptr(), entry0=d_ * d_ * lo, n_entries=d_ * d_ * hi, key_lo=c0 * a_ * a_, key_hi=c1 * a_ * a_, cell0=c0,
                          first=1 if i == 0 else 0)))
    return want


def diagonal_launches(m, a, out_ptr, cap):
    d_, a_ = m.d, m.a
    dd = d_ * d_
    cw = max(1, 64 // a_)
    chunk_cells = a.scratch_bytes // (a_ * dd * 8) // cw * cw
    mask = a._mask_table(m.dev)
    common = {"out": out_ptr, "mask": 0 if mask is None else mask.data_ptr(), "n_entries": dd * m.n_nodes}
    node_blocks = max(1, lane_blocks(dd * m.n_nodes, cap))
    if m.n_cells == 0:
        return [(to.DIAGONAL_NODE_KERNEL, node_blocks, dict(common, de=0, key_lo=0, key_hi=0, first=1))]
    de = a._scratch[m.dev]
    assert de.numel() == min(chunk_cells, m.n_cells) * a_ * dd
    want = []
    for i, (c0, c1) in enumerate(chunks_of(m.n_cells, chunk_cells)):
        want.append(m.element(to.DIAGONAL_ELEMENT_KERNEL, c0, c1, cw, cap, "de", de))
        want.append((to.DIAGONAL_NODE_KERNEL, node_blocks, dict(common, de=de.data_ptr(), key_lo=c0 * a_, key_hi=c1 * a_, first=1 if i == 0 else 0)))
    return want


def product_launches(m, a, v, out, cap):
    nd = m.d * m.n_nodes
    w = 64 // m.q
    w = w - 1 if w > 1 and (w * m.q * m.d * m.d) % 2 else w
    want = []
    fe = 0
    if m.n_cells:
        fe = m.f._fe[m.dev].data_ptr()
        want.append((to.ELEMENT_KERNEL, tile_blocks(m.n_cells, w, cap), {"tangent": m.tangent.data_ptr(), "v": v.data_ptr(), "fe": fe, "n_cells": m.n_cells,
                                                                         "mode": to.MODE_QUIET}))
    nseg = -(-nd // to.SEG)
    want.append((to.NODE_KERNEL, max(1, min(nseg, cap)), {"fe": fe, "v": v.data_ptr(), "out": out.data_ptr(), "n_dofs": nd, "nseg": nseg, "mode": to.MODE_QUIET}))
    return want


def force_launches(m, src, grad, out, cap):
    nd = m.d * m.n_nodes
    w = 64 // m.q
    w = w - 1 if w > 1 and (w * m.q * m.d * m.d) % 2 else w
    if m.n_cells == 0:
        return []
    jinv, weights, fe = m.op._tables(m.dev)[2], m.f._tables(m.dev)[0], m.f._fe[m.dev]
    assert fe.numel() == m.n_cells * m.a * m.d
    return [(force.ELEMENT_KERNEL, tile_blocks(m.n_cells, w, cap), {"src": src.data_ptr(), "grad": 0 if grad is None else grad.data_ptr(), "jinv": jinv.data_ptr(),
                                                                    "weights": weights.data_ptr(), "fe": fe.data_ptr(), "n_cells": m.n_cells}),
            (force.NODE_KERNEL, lane_blocks(nd, cap), {"fe": fe.data_ptr(), "out": out.data_ptr(), "n_dofs": nd})]


def gradient_launches(m, du, out, cap):
    n_points = m.n_cells * m.q
    if n_points == 0:
        return []
    dofmap, ref, jinv, _ = m.op._tables(m.dev)
    return [(gradient.KERNEL, tile_blocks(n_points, 64, cap), {"du": du.data_ptr(), "dofmap": dofmap.data_ptr(), "ref": ref.data_ptr(), "jinv": jinv.data_ptr(),
                                                               "out": out.data_ptr(), "n": n_points})]


def setup_launches(m, a, pc, cap, rigid):
    """the first Galerkin step from the element matrices, the Galerkin steps of the coarser levels, then per level the inverses of
    the nodes' own blocks -- on level 0 behind the operator's diagonal-block launches"""
    d_, a_ = m.d, m.a
    dd, cols = d_ * d_, a_ * d_
    on = pc._on[m.dev]
    levels = pc.levels
    dofs = [d_] + [{2: 3, 3: 6}[d_] if rigid else d_] * (len(levels) - 1)
    want = []
    if len(levels) > 1:
        cw = max(1, 64 // cols)
        chunk_cells = a.scratch_bytes // (cols * cols * 8) // cw * cw
        agg = pc.aggregates(0)
        indptr, indices = pc.pattern(1)
        mask = a._mask_table(m.dev)
        for i, (c0, c1) in enumerate(chunks_of(m.n_cells, chunk_cells)):
            want.append(m.element(matrix.ELEMENT_KERNEL, c0, c1, cw, cap, "ke", on.ke))
            lo, hi = (0, levels[1]["blocks"]) if i == 0 else touched(agg[m.t["dofmap"]], levels[1]["nodes"], indptr, indices, c0, c1)
            fields = {"ke": on.ke.data_ptr(), "values": on.values[1].data_ptr(), "mask": 0 if mask is None else mask.data_ptr(), "key_lo": c0 * a_ * a_,
                      "key_hi": c1 * a_ * a_, "cell0": c0, "first": 1 if i == 0 else 0}
            if rigid:  # a group of 64 lanes (3-D) per coarse block
                want.append((multilevel.FREE_RIGID_GALERKIN_KERNEL, max(1, lane_blocks({2: 16, 3: 64}[d_] * (hi - lo), cap)), dict(fields, block0=lo, block1=hi)))
            else:  # a lane per entry
                want.append((multilevel.FREE_GALERKIN_KERNEL, max(1, lane_blocks(dd * (hi - lo), cap)), dict(fields, entry0=dd * lo, n_entries=dd * hi)))
    for l in range(1, len(levels) - 1):
        n_coarse = dofs[l + 1]**2 * levels[l + 1]["blocks"]
        want.append((multilevel.RIGID_GALERKIN_KERNEL if rigid else multilevel.GALERKIN_KERNEL, max(1, lane_blocks(n_coarse, cap)), {"n_coarse": n_coarse}))
    for l, lv in enumerate(levels):
        if l == 0:
            want += diagonal_launches(m, a, on.blocks.data_ptr(), cap)
        want.append((solver.INVERSE_KERNEL, max(1, lane_blocks(lv["nodes"], cap)), {"n_nodes": lv["nodes"], "inv": on.inv[l].data_ptr()}))
    return want


# ---------------------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gradient_force_and_product(shape, recorded):
    launches, cap = recorded
    d_, a_, q_, _ = SHAPES[shape]
    w = force.cells_per_tile(d_, q_)
    for n_cells in (0, 1, (gradient.BLOCKS_PER_CU * 4 + 5) * w + 1):  # the last: more tiles than the waves of one compute unit's grid
        m = Mesh(shape, n_cells, 5 + n_cells)
        what = f"{shape} cells={n_cells} cap={cap}"
        du = to_device(m.t["du"], "cuda")
        have, grad = trace(launches, lambda: m.op(du))
        assert_launches(have, gradient_launches(m, du, grad, cap), what + " gradient")
        stress = to_device(m.t["stress"], "cuda")
        have, out = trace(launches, lambda: m.f(stress))
        assert_launches(have, force_launches(m, stress, None, out, cap), what + " force")
        have, out = trace(launches, lambda: m.f.tangent_action(m.tangent, grad, out=out, accumulate=True))
        assert_launches(have, force_launches(m, m.tangent, grad, out, cap), what + " tangent action")
        a = fc.TangentOperator(m.f)
        have, y = trace(launches, lambda: a(m.tangent, du))
        assert_launches(have, product_launches(m, a, du, y, cap), what + " product")
        if n_cells > 1:
            assert have[0][1] == min(gradient.BLOCKS_PER_CU + 2, cap)  # (the one compute unit's cap is what held)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_tangent_matrix(shape, recorded):
    launches, cap = recorded
    d_, a_, q_, _ = SHAPES[shape]
    cols = a_ * d_
    cw = matrix.cells_per_tile(d_, a_)
    tile = cw * cols * cols * 8
    for n_cells, scratches in ((0, (None,)), (1, (None, tile)), (2 * 5 * cw + 3, (5 * tile + 8, tile, None))):
        m = Mesh(shape, n_cells, 11 + n_cells)
        pattern = None if n_cells else np.arange(a_, dtype=np.int32)[None, :]  # (no cell: the pattern of one cell nobody fills)
        for scratch in scratches:
            for fmt in matrix.FORMATS:
                what = f"{shape} cells={n_cells} scratch={scratch} {fmt} cap={cap}"
                k = fc.TangentMatrix(m.f, format=fmt, scratch_bytes=scratch, pattern_dofmap=pattern)
                if n_cells > 1:
                    assert len(k.chunks()) == {5 * tile + 8: 3, tile: -(-n_cells // cw), None: 1}[scratch], what
                    k.set_constrained(random_mask(m.t, d_, 3))
                have, values = trace(launches, lambda: k(m.tangent))
                assert_launches(have, matrix_launches(m, k, values, cap, 0), what)
                have, _ = trace(launches, lambda: k(m.tangent, out=values, accumulate=True))
                assert_launches(have, matrix_launches(m, k, values, cap, 1), what + " accumulate")
        assert have, what


@pytest.mark.parametrize("shape", list(SHAPES))
def test_diagonal_blocks_of_the_operator(shape, recorded):
    launches, cap = recorded
    d_, a_, q_, _ = SHAPES[shape]
    cw = to.diagonal_cells_per_tile(a_)
    tile = cw * a_ * d_ * d_ * 8
    for n_cells, scratches in ((0, (None,)), (1, (None, tile)), (2 * 5 * cw + 3, (5 * tile + 8, tile, None))):
        m = Mesh(shape, n_cells, 17 + n_cells)
        for scratch in scratches:
            what = f"{shape} cells={n_cells} scratch={scratch} cap={cap}"
            a = fc.TangentOperator(m.f, scratch_bytes=scratch)
            if n_cells > 1:
                assert len(a.chunks()) == {5 * tile + 8: 3, tile: -(-n_cells // cw), None: 1}[scratch], what
                a.set_constrained(random_mask(m.t, d_, 4))
            have, blocks = trace(launches, lambda: a.diagonal_blocks(m.tangent))
            assert_launches(have, diagonal_launches(m, a, blocks.data_ptr(), cap), what)
            have, _ = trace(launches, lambda: a.diagonal_blocks(m.tangent, out=blocks.reshape(-1)))
            assert_launches(have, diagonal_launches(m, a, blocks.data_ptr(), cap), what + " into out")


@pytest.mark.parametrize("coarse_space", multilevel.COARSE_SPACES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_multilevel_setup_on_the_operator(shape, coarse_space, recorded):
    launches, cap = recorded
    d_, a_, q_, _ = SHAPES[shape]
    cols = a_ * d_
    cw = matrix.cells_per_tile(d_, a_)
    tile = cw * cols * cols * 8
    rigid = coarse_space == "rigid_body"
    # (no cell: every node is an aggregate of its own, the hierarchy does not shrink and stays at one level -- no Galerkin step, the
    # diagonal node kernel alone before the inverses, and a cycle of the coarsest sweeps on the operator itself)
    for n_cells, scratches in ((0, (None,)), (1, (None, tile)), (2 * 5 * cw + 3, (5 * tile + 8, tile, None))):
        m = Mesh(shape, n_cells, 23 + n_cells, every_node=True)
        x = np.random.default_rng(n_cells).normal(size=(m.n_nodes, d_)) if rigid else None
        for scratch in scratches:
            what = f"{shape} cells={n_cells} scratch={scratch} {coarse_space} cap={cap}"
            a = fc.TangentOperator(m.f, scratch_bytes=scratch)
            if n_cells > 1:
                a.set_constrained(random_mask(m.t, d_, 6))
            pc = fc.MultilevelPreconditioner(a, coarsest_nodes=4, coarse_space=coarse_space, coordinates=x)
            assert len(pc.levels) > 1 if n_cells else len(pc.levels) == 1, what
            if n_cells > 1:
                assert len(pc._seam.chunks()) == {5 * tile + 8: 3, tile: -(-n_cells // cw), None: 1}[scratch], what
            have, _ = trace(launches, lambda: pc.setup(m.tangent))
            assert_launches(have, setup_launches(m, a, pc, cap, rigid), what)
            # one application behind it: the setup again, then the cycle, every grid of it a lane per entry and at least one block
            applied, _ = trace(launches, lambda: pc.apply(m.tangent, to_device(m.t["du"], "cuda")))
            assert_launches(applied[:len(have)], setup_launches(m, a, pc, cap, rigid), what + " apply")
            sized = {multilevel.SMOOTH_KERNEL: "n", multilevel.PROLONG_KERNEL: "n", multilevel.RIGID_PROLONG_KERNEL: "n", multilevel.RESTRICT_KERNEL: "n_coarse",
                     multilevel.RIGID_RESTRICT_KERNEL: "n_coarse"}
            cycle = applied[len(have):]
            transfers = {multilevel.RIGID_RESTRICT_KERNEL if rigid else multilevel.RESTRICT_KERNEL} if n_cells else set()
            assert {kernel for kernel, _, _ in cycle} >= {multilevel.SMOOTH_KERNEL} | transfers, what
            for kernel, blocks, fields in cycle:
                if kernel in sized:
                    assert blocks == max(1, lane_blocks(fields[sized[kernel]], cap)), (what, kernel)
                elif kernel in (solver.MATVEC_KERNEL, to.NODE_KERNEL):
                    assert blocks == max(1, min(fields["nseg"], cap)), (what, kernel)
                else:
                    assert kernel == to.ELEMENT_KERNEL and blocks == tile_blocks(n_cells, force.cells_per_tile(d_, q_), cap), (what, kernel)
