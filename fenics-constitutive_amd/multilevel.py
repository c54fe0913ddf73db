"""An aggregation multilevel preconditioner for the device solver: ``z = M^-1 r`` over a hierarchy of node aggregates with Galerkin
coarse matrices, applied on the GPU inside ``ConjugateGradient`` (``preconditioner="multilevel"`` or an instance).

*The hierarchy* is built once per pattern on the host (NumPy, no values involved, deterministic).  Aggregation works on the node
graph of a level's block pattern; a row's neighbours are its column nodes, itself included.  Pass 1, nodes ascending: a node whose
neighbours are all unaggregated becomes a root and its whole neighbourhood the next aggregate.  Pass 2: every node still free
joins the aggregate of its lowest-numbered neighbour that pass 1 aggregated (the state after pass 1, not one updated on the way).
Pass 3: what is left -- a node with no neighbour but itself -- is an aggregate of its own.  Aggregates are numbered in order of
creation.  The coarse pattern is ``{(agg[i], agg[j])}`` over the fine blocks, block CSR with sorted columns whatever the format of
``K``; coarse blocks stay ``D x D`` (piecewise-constant translation aggregates), so every level is multiplied by the solver's
matrix-vector kernel and its nodes' own blocks are inverted by the solver's inverse kernel.  Levels are added until one has at
most ``coarsest_nodes`` nodes, ``max_levels`` is reached or a level does not shrink.

*The arithmetic* is fixed as in ``solver.py`` (no floating-point atomics, no MFMA, ``-ffp-contract=off``, ``/`` is a division), so
a NumPy oracle gives the bits:

*Galerkin values*, every call, level ``l + 1`` from level ``l``: for coarse block ``(I, J)`` and entry ``(r, s)``: ``f = 0.0; f = f +
value_l(k, r, s)`` over the fine blocks ``k`` that fold into it, ascending; level 0's value sits where ``dest_base`` / ``dest_stride``
of the ``TangentMatrix`` say (both formats: the same bits).  Constrained dofs are not special: their identity rows add ``1.0`` per
constrained member to a coarse diagonal, which keeps a fully constrained aggregate non-singular and ``M`` symmetric positive
definite.  *Block inverses* of every level: the solver's formulas; a zero or non-finite determinant on any level: status
``singular_block``.  *Restriction*: ``rc[D I + c] = 0.0; rc = rc + d[D i + c]`` over the members ``i`` of ``I``, ascending; ``d`` is the
level's right-hand side (additive) or ``b[e] - q[e]`` formed in the same kernel (multiplicative).  *Prolongation*: ``x[D i + c] =
x[D i + c] + xc[D agg[i] + c]``, on level 0 skipped at the dofs of ``K.set_constrained`` (the mask the matrix carries at the call).
*Smoothing sweep*: from zero ``x = omega * t``, later ``x = x + omega * t``, ``t = 0.0; t = t + inv[v][c][s] * d[D v + s]``, ``s``
ascending, ``d = b`` or ``b - q``, ``q = K x`` by the matrix-vector kernel.

*Additive cycle*: going down ``z_l = D_l^-1 r_l`` (no ``omega``: ``x = t``), ``r_{l+1} = R r_l``; on the coarsest level
``coarsest_sweeps`` damped sweeps from zero; going up ``z_l = z_l + P z_{l+1}``.  *Multiplicative cycle*, per level: ``smoothing``
sweeps from zero, ``q = K_l x``, restrict ``b - q``, recurse, prolong, ``smoothing`` sweeps; the coarsest level as in the additive
cycle.  With one level both cycles are the coarsest sweeps on ``K`` itself.

*In the conjugate gradients* the update kernel (``FCAMD_CG_PRECOND = 2``) forms neither ``z`` nor ``rz``; the cycle's launches and
the closing kernel follow it: ``rz' = r . z`` by the solver's ordered dot, ``rz_old = rz``, ``rz = rz'`` (in the start: ``p = z``), and
not ``rz > 0``: status ``indefinite`` (the iteration has been counted).  Every kernel returns at once when the status is not
"running", so iterations enqueued behind the end are no-ops and ``check_every`` changes no bit.

THE MULTIPLICATIVE CYCLE AND THE COARSEST SWEEPS NEED ``omega * lambda_max(D^-1 K) < 2``; nothing is refused for it and nothing
estimates ``lambda_max``.  On the trilinear hexahedron cube it is 2.87, hence the default ``omega = 0.5``.

*The rigid-body coarse space* (``coarse_space="rigid_body"``, ``coordinates``; csrc/jit/multilevel_rigid.hip).  Aggregation, coarse
patterns, ``fold`` and ``members`` are the ones above; a coarse node carries ``Dc = D + R`` dofs, ``D`` translations and ``R``
rotations (``R = 3`` in 3-D, ``1`` in 2-D; in 1-D there is no rotation and the translation hierarchy is built), so the blocks of the
levels ``l >= 1`` are ``Dc x Dc``.  *Positions*: level 0 has ``coordinates``; a node of level ``l + 1`` has ``s = 0.0; s = s + x_i`` over the
members ``i`` of its aggregate, ascending, then ``s / count`` (per coordinate).  *Offsets*: ``o_i = x_i - x_agg(i)``.  ``B(o)`` is the
``D x R`` matrix of ``theta -> theta x o``: 3-D ``[[0, oz, -oy], [-oz, 0, ox], [oy, -ox, 0]]``, 2-D ``[-oy, ox]^T`` (a minus negates the
offset's entry, the zeros are ``+0.0``).  The prolongation block of node ``i`` is ``P_i = [I_D  B(o_i)]`` (``D x Dc``) from level 0 and
``P_i = [[I_D, B(o_i)], [0, I_R]]`` (``Dc x Dc``) from a level ``l >= 1``, formed in registers; all its entries take part in the sums,
the zeros and ones too.  With ``Df`` the dofs per node of the fine level of a pair (``D`` or ``Dc``):
*Galerkin values*, coarse block ``(I, J)``, entry ``(r, s)``: ``f = 0.0``; over the fine blocks ``k = (i, j)`` that fold into it, ascending:
``t = 0.0``; for ``a`` ascending: ``u = 0.0; u = u + value_l(k, a, b) * P_j[b][s]``, ``b`` ascending; ``t = t + P_i[a][r] * u``; then
``f = f + t``.  *Restriction*: ``rc[Dc I + c] = 0.0``; over the members ``i``, ascending: ``t = 0.0; t = t + P_i[a][c] * d[Df i + a]``, ``a``
ascending; ``rc = rc + t``.  *Prolongation*: ``t = 0.0; t = t + P_i[r][c] * xc[Dc agg[i] + c]``, ``c`` ascending; ``x[Df i + r] = x[Df i + r] +
t``, on level 0 skipped at the constrained dofs.  *Block inverses* of ``6 x 6`` blocks: Gauss-Jordan in place, pivots in the order
0 .. 5 without a search: ``p = m[k][k]; m[k][k] = 1.0; m[k][j] = m[k][j] / p``, ``j`` ascending; for the rows ``i != k`` ascending:
``f = m[i][k]; m[i][k] = 0.0; m[i][j] = m[i][j] - f * m[k][j]``, ``j`` ascending; a zero or non-finite pivot: ``singular_block``
(``3 x 3`` blocks, 2-D: the solver's cofactor formulas).  Smoothing, products and cycles are the ones above on the levels' own block
sizes.  Two programs per object: the fine one (``FCAMD_CG_D = D``, the object's ``_code``, with the ``(D, Dc)`` transfer kernels) and the
coarse one (``FCAMD_CG_D = Dc``: every level ``l >= 1`` and the ``(Dc, Dc)`` transfer kernels).  A level-0 aggregate whose columns of ``P``
are linearly dependent -- a lone node, all members at one point, in 3-D all members on one line -- is refused at construction.

*On a matrix-free operator* (``MultilevelPreconditioner(A)`` with a ``TangentOperator``; csrc/jit/multilevel_free.hip for the
translations, csrc/jit/multilevel_free_rigid.hip for the rigid-body modes, below).  The hierarchy is that of ``matrix.block_pattern(dofmap, n_nodes)``: every table is the one of a ``TangentMatrix`` of the same
force (a node of no cell, which that matrix would refuse, has a row of its own block).  Nothing reads fine values: the first argument of ``setup``, ``apply`` and the solve is the tangent of the quadrature points.
*Level-1 values*, coarse block ``(I, J)``, entry ``(r, s)``: ``f`` = the number of constrained dofs ``D i + r`` among the members ``i`` of
``I``, as a double, if ``I == J`` and ``r == s``, else ``0.0``; over the contributions ``(c, a, b)`` with ``agg[dofmap[c][a]] == I`` and
``agg[dofmap[c][b]] == J``, ascending in ``c A A + a A + b``: nothing where dof ``D dofmap[c][a] + r`` or dof ``D dofmap[c][b] + s`` is
constrained, else ``f = f + ke[c][a][r][b][s]`` (``ke``: the element matrix of ``matrix.py``'s docstring, on the bits, from its element
kernel).  This is ``P^T (M K M + I - M) P``, the Galerkin step of the assembled route in another order of summation: equal to it
within rounding, not on the bits.  The remark on the constrained dofs carries over: each adds ``1.0`` to its aggregate's coarse
diagonal, a fully constrained aggregate stays non-singular and ``M`` symmetric positive definite.  The element matrices pass through
a scratch of at most ``A.scratch_bytes`` in ascending whole-tile chunks of cells, ``(A D)^2 * 8`` bytes per cell; a later chunk goes
on from the value that is there, so the bits do not depend on the chunk size.  *Level 0 of the cycle*: the block array is
``A.diagonal_blocks(tangent)``, inverted by the solver's inverse kernel through the diagonal table ``0 .. n`` (what block-Jacobi on
an operator does); a product of the multiplicative cycle is the operator's two launches in quiet mode, which does not look at
the status: behind the end of a solve such a product still writes the preconditioner's own ``q``, which no kernel reads then.
Restriction, prolongation (skipped at the operator's constrained dofs), smoothing, the closing kernel and the levels ``l >= 2`` are
the kernels above, unchanged.

*The rigid-body coarse space on an operator* (``MultilevelPreconditioner(A, coarse_space="rigid_body", coordinates=X)``).  Positions,
offsets, ``P_i = [I_D  B(o_i)]``, the ``(D, Dc)`` transfer kernels of level 0, the ``(Dc, Dc)`` Galerkin kernel of the levels ``l >= 2``,
the inverses and the cycles are those of the rigid-body coarse space above; level 0 is the operator's as in the last paragraph (its
own blocks, its products); the contribution lists, their chunks and the element matrices are those of the translations.  Only the
first Galerkin step is new.  *Level-1 values*, coarse block ``(I, J)``, entry ``(r, s)``, ``0 <= r, s < Dc``: ``f = 0.0``; with a mask and
``I == J``, over the members ``i`` of ``I``, ascending: ``t = 0.0``; for ``a = 0 .. D - 1`` ascending, where dof ``D i + a`` is constrained:
``t = t + P_i[a][r] * P_i[a][s]``; then ``f = f + t`` (every member takes part, one with no constrained dof adds ``0.0``; without a mask
the loop is skipped: the same bits).  Then over the contributions ``(c, a, b)`` of the block, ascending in ``c A A + a A + b``, with ``i =
dofmap[c][a]`` and ``j = dofmap[c][b]``: ``t = 0.0``; for ``a' = 0 .. D - 1`` ascending, skipped where dof ``D i + a'`` is constrained: ``u =
0.0``; for ``b' = 0 .. D - 1`` ascending, skipped where dof ``D j + b'`` is constrained: ``u = u + ke[c][a][a'][b][b'] * P_j[b'][s]``; ``t = t +
P_i[a'][r] * u``; then ``f = f + t``.  A later chunk of cells goes on from the value that is there, so the bits do not depend on
``A.scratch_bytes``.  This is ``P^T (M K M + I - M) P``, the rigid-body Galerkin step of the assembled route in another order of
summation: equal to it within rounding, not on the bits; a constrained dof adds its translation's ``1.0`` and its couplings to the
rotations.  The level-0 offsets go to the device, no level-0 fold list does.  Coordinates that put all nodes of a mesh of more than
one node at one point are refused on an operator whatever the number of levels (every offset is zero, the rotations vanish).

LDS of a block: ``lds_bytes(kernel)`` (``lds_bytes(FREE_RIGID_GALERKIN_KERNEL, gdim)`` for the gather above).
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import jit, solver
from . import matrix as _matrix
from ._fe_common import ChunkedPass, blocks_for
from .force import compile_without_scratch, kernel_resources
from .gradient import BLOCKS_PER_CU
from .matrix import TangentMatrix
from .tangent_operator import TangentOperator

GALERKIN_KERNEL = "fcamd_ml_galerkin_kernel"
RESTRICT_KERNEL = "fcamd_ml_restrict_kernel"
PROLONG_KERNEL = "fcamd_ml_prolong_kernel"
SMOOTH_KERNEL = "fcamd_ml_smooth_kernel"
CLOSE_KERNEL = "fcamd_ml_close_kernel"
KERNELS = (GALERKIN_KERNEL, RESTRICT_KERNEL, PROLONG_KERNEL, SMOOTH_KERNEL, CLOSE_KERNEL)
RIGID_GALERKIN_KERNEL = "fcamd_mr_galerkin_kernel"
RIGID_RESTRICT_KERNEL = "fcamd_mr_restrict_kernel"
RIGID_PROLONG_KERNEL = "fcamd_mr_prolong_kernel"
RIGID_KERNELS = (RIGID_GALERKIN_KERNEL, RIGID_RESTRICT_KERNEL, RIGID_PROLONG_KERNEL)
FREE_GALERKIN_KERNEL = "fcamd_mf_galerkin_kernel"
FREE_RIGID_GALERKIN_KERNEL = "fcamd_mfr_galerkin_kernel"
CYCLES = ("multiplicative", "additive")
COARSE_SPACES = ("translations", "rigid_body")
_MODE_QUIET = 3
#: launch plans kept per device: one per (source, destination) pair of the applications in flight -- one in the conjugate
#: gradients, two in BiCGStab (p -> y, s -> z), and the standalone ``apply`` beside them
PLANS = 4

__all__ = ["MultilevelPreconditioner", "aggregate", "coarse_dofs", "coarsen", "compile_free_kernels", "compile_free_rigid_kernels", "compile_kernels",
           "compile_rigid_kernels", "free_program", "free_rigid_program", "hierarchy", "lds_bytes", "place", "program", "rigid_program"]


def lds_bytes(kernel: str = CLOSE_KERNEL, gdim: int = 3) -> int:
    """LDS of one block of ``kernel``: the tree of the dot and the last-block flag in the closing kernel, nothing in the other four
    nor in the three of the rigid-body coarse space; the solver's kernels of the same program: ``solver.lds_bytes(kernel, False)``.
    The first Galerkin step of an operator with the rigid-body space, in ``gdim`` dimensions: per lane a double of an element
    matrix, a double of an offset and the int of a constrained byte, and four ints per group of 64 (3-D) or 16 (2-D) lanes"""
    if kernel in solver.KERNELS:
        return solver.lds_bytes(kernel, False)
    if kernel == FREE_RIGID_GALERKIN_KERNEL:
        return 256 * (8 + 8 + 4) + 256 // {2: 16, 3: 64}[int(gdim)] * 4 * 4
    if kernel in RIGID_KERNELS or kernel == FREE_GALERKIN_KERNEL:
        return 0
    return {CLOSE_KERNEL: 8 * (256 + 2), GALERKIN_KERNEL: 0, RESTRICT_KERNEL: 0, PROLONG_KERNEL: 0, SMOOTH_KERNEL: 0}[kernel]


def program(gdim: int, slab: int = solver.SLAB) -> str:
    """the program text of one block size: the solver's kernels without their own preconditioner and the multilevel kernels"""
    return "\n".join([f"#define FCAMD_CG_D {int(gdim)}", "#define FCAMD_CG_PRECOND 2", f"#define FCAMD_CG_SLAB {int(slab)}", '#include "multilevel.hip"']) + "\n"


def compile_kernels(gdim: int):
    """The code object of one block size, all ten kernels in it (no GPU needed).  A kernel with scratch is a ``ValueError``."""
    if gdim not in (1, 2, 3):
        raise ValueError(f"the dofs per node must be 1, 2 or 3, got {gdim}")
    return compile_without_scratch(program(gdim), f"multilevel_{gdim}d", solver.MATVEC_KERNEL, solver.KERNELS + KERNELS)


def coarse_dofs(gdim: int) -> int:
    """``Dc``: the dofs of a coarse node of the rigid-body coarse space, translations and rotations (1-D: no rotation)"""
    return {1: 1, 2: 3, 3: 6}[int(gdim)]


def rigid_program(gdim: int, block: int, slab: int = solver.SLAB) -> str:
    """the program text of the rigid-body coarse space in ``gdim`` dimensions with blocks of ``block`` dofs per node: ``gdim`` (the
    fine program) or ``coarse_dofs(gdim)`` (the coarse program)"""
    return "\n".join([f"#define FCAMD_CG_D {int(block)}", "#define FCAMD_CG_PRECOND 2", f"#define FCAMD_CG_SLAB {int(slab)}",
                      f"#define FCAMD_ML_GDIM {int(gdim)}", '#include "multilevel_rigid.hip"']) + "\n"


def compile_rigid_kernels(gdim: int):
    """``(fine, coarse)``: the two code objects of the rigid-body coarse space in 2 or 3 dimensions, thirteen kernels in each (no GPU
    needed).  A kernel with scratch is a ``ValueError``."""
    if gdim not in (2, 3):
        raise ValueError(f"the rigid-body coarse space is for 2 or 3 dofs per node, got {gdim}")
    return tuple(compile_without_scratch(rigid_program(gdim, block), f"multilevel_rigid_{gdim}d_{block}", solver.MATVEC_KERNEL,
                                         solver.KERNELS + KERNELS + RIGID_KERNELS) for block in (gdim, coarse_dofs(gdim)))


def free_program(gdim: int, nodes_per_cell: int) -> str:
    """the program text of the first Galerkin step of a ``TangentOperator``: level 1 from the element matrices"""
    return "\n".join([f"#define FCAMD_MF_D {int(gdim)}", f"#define FCAMD_MF_A {int(nodes_per_cell)}", '#include "multilevel_free.hip"']) + "\n"


def compile_free_kernels(gdim: int, nodes_per_cell: int):
    """The code object of the first Galerkin step of a ``TangentOperator`` of one cell shape (no GPU needed).  Scratch is a
    ``ValueError``."""
    if gdim not in (1, 2, 3):
        raise ValueError(f"the dofs per node must be 1, 2 or 3, got {gdim}")
    if nodes_per_cell < 1:
        raise ValueError("a cell needs at least one node")
    return compile_without_scratch(free_program(gdim, nodes_per_cell), f"multilevel_free_{gdim}d_{nodes_per_cell}n", FREE_GALERKIN_KERNEL,
                                   (FREE_GALERKIN_KERNEL,))


def free_rigid_program(gdim: int, nodes_per_cell: int) -> str:
    """the program text of the first Galerkin step of a ``TangentOperator`` with the rigid-body coarse space"""
    return "\n".join([f"#define FCAMD_MF_D {int(gdim)}", f"#define FCAMD_MF_A {int(nodes_per_cell)}", '#include "multilevel_free_rigid.hip"']) + "\n"


def compile_free_rigid_kernels(gdim: int, nodes_per_cell: int):
    """The code object of the first Galerkin step of a ``TangentOperator`` of one cell shape with the rigid-body coarse space (no GPU
    needed).  Scratch is a ``ValueError``."""
    if gdim not in (2, 3):
        raise ValueError(f"the rigid-body coarse space is for 2 or 3 dofs per node, got {gdim}")
    if nodes_per_cell < 1:
        raise ValueError("a cell needs at least one node")
    return compile_without_scratch(free_rigid_program(gdim, nodes_per_cell), f"multilevel_free_rigid_{gdim}d_{nodes_per_cell}n",
                                   FREE_RIGID_GALERKIN_KERNEL, (FREE_RIGID_GALERKIN_KERNEL,))


# ---- the hierarchy (host) --------------------------------------------------------------------------------------------------------
def aggregate(indptr: np.ndarray, indices: np.ndarray):
    """``(agg[n_nodes], roots)``: the aggregate of every node of the block pattern and the root of every aggregate (int32), by the
    three passes of the module docstring"""
    n = int(indptr.size - 1)
    ptr, cols = indptr.tolist(), indices.tolist()
    agg = [-1] * n
    roots = []
    for v in range(n):  # pass 1
        nb = cols[ptr[v]: ptr[v + 1]]
        if agg[v] >= 0 or any(agg[u] >= 0 for u in nb):
            continue
        for u in nb:
            agg[u] = len(roots)
        agg[v] = len(roots)
        roots.append(v)
    agg1 = np.array(agg, dtype=np.int64).reshape(n)
    out = agg1.copy()
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr.astype(np.int64)))
    cols = indices.astype(np.int64)
    sel = np.flatnonzero((agg1[rows] < 0) & (agg1[cols] >= 0))  # pass 2 (the columns of a row ascend: the first is the lowest)
    joiners, first = np.unique(rows[sel], return_index=True)
    out[joiners] = agg1[cols[sel[first]]]
    alone = np.flatnonzero(out < 0)  # pass 3
    out[alone] = len(roots) + np.arange(alone.size)
    return out.astype(np.int32), np.concatenate([np.array(roots, dtype=np.int64), alone]).astype(np.int32)


def coarsen(indptr: np.ndarray, indices: np.ndarray, agg: np.ndarray, n_agg: int):
    """``(indptr, indices, fold_ptr, fold)`` (int32): the coarse block CSR pattern ``{(agg[i], agg[j])}`` with sorted columns, and for
    coarse block ``K`` the fine blocks ``fold[fold_ptr[K]: fold_ptr[K + 1]]`` that fold into it, ascending"""
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr.astype(np.int64)))
    key = agg.astype(np.int64)[rows] * n_agg + agg.astype(np.int64)[indices]
    order = np.argsort(key, kind="stable")  # stable: ascending fine block within a coarse block
    pattern, counts = np.unique(key, return_counts=True)
    c_indptr = np.zeros(n_agg + 1, dtype=np.int64)
    np.cumsum(np.bincount(pattern // n_agg, minlength=n_agg), out=c_indptr[1:])
    fold_ptr = np.zeros(pattern.size + 1, dtype=np.int64)
    np.cumsum(counts, out=fold_ptr[1:])
    return c_indptr.astype(np.int32), (pattern % n_agg).astype(np.int32), fold_ptr.astype(np.int32), order.astype(np.int32)


class Level:
    """one level's pattern and, unless it is the coarsest, the tables that lead to the next"""

    def __init__(self, indptr, indices):
        self.indptr, self.indices = indptr, indices
        self.n_nodes, self.nnzb = int(indptr.size - 1), int(indices.size)
        rows = np.repeat(np.arange(self.n_nodes, dtype=np.int32), np.diff(indptr.astype(np.int64)))
        self.diag_block = np.full(self.n_nodes, -1, dtype=np.int64)
        on = np.flatnonzero(indices == rows)
        self.diag_block[rows[on]] = on
        self.block_row = rows  # the row node of every block
        self.agg = self.roots = self.mem_ptr = self.members = self.fold_ptr = self.fold = None
        self.position = self.offset = None  # place(): [n_nodes][gdim] each; the coarsest level has no offset


def hierarchy(indptr: np.ndarray, indices: np.ndarray, coarsest_nodes: int = 64, max_levels: int = 10) -> list:
    """the levels of a block pattern, finest first"""
    levels = [Level(np.ascontiguousarray(indptr, dtype=np.int32), np.ascontiguousarray(indices, dtype=np.int32))]
    while levels[-1].n_nodes > coarsest_nodes and len(levels) < max_levels:
        fine = levels[-1]
        agg, roots = aggregate(fine.indptr, fine.indices)
        if roots.size >= fine.n_nodes:
            break  # it does not shrink
        c_indptr, c_indices, fold_ptr, fold = coarsen(fine.indptr, fine.indices, agg, int(roots.size))
        fine.agg, fine.roots, fine.fold_ptr, fine.fold = agg, roots, fold_ptr, fold
        fine.members = np.argsort(agg, kind="stable").astype(np.int32)  # ascending within an aggregate
        mem_ptr = np.zeros(roots.size + 1, dtype=np.int64)
        np.cumsum(np.bincount(agg, minlength=roots.size), out=mem_ptr[1:])
        fine.mem_ptr = mem_ptr.astype(np.int32)
        levels.append(Level(c_indptr, c_indices))
    return levels


def place(levels: list, coordinates: np.ndarray) -> None:
    """the position of every node of every level and its offset from its aggregate's position (module docstring): level 0 has
    ``coordinates``, a coarse node the sum of its members' positions, ascending, divided by their count"""
    levels[0].position = np.ascontiguousarray(coordinates, dtype=np.float64)
    for fine, coarse in zip(levels[:-1], levels[1:]):
        total = np.zeros((coarse.n_nodes, fine.position.shape[1]))
        np.add.at(total, fine.agg, fine.position)  # unbuffered, in the order of the nodes: ascending within an aggregate
        coarse.position = total / np.diff(fine.mem_ptr).astype(np.float64)[:, None]
        fine.offset = fine.position - coarse.position[fine.agg]


def _refuse_degenerate(lv) -> None:
    """a level-0 aggregate whose columns of ``P`` are linearly dependent: a ``ValueError`` that names it"""
    g = lv.offset.shape[1]
    for a in range(lv.roots.size):
        mine = lv.members[lv.mem_ptr[a]: lv.mem_ptr[a + 1]]
        sv = np.linalg.svd(lv.offset[mine], compute_uv=False)
        rank = int((sv > 1e-10 * sv[0]).sum()) if sv[0] > 0.0 else 0
        if rank >= g - 1:
            continue
        what = "is a lone node" if mine.size == 1 else "has all its members at one point" if rank == 0 else "has all its members on one line"
        raise ValueError(f"aggregate {a} of level 0 (root {int(lv.roots[a])}, {mine.size} members) {what}: its rigid-body modes are linearly dependent")


class RigidArgs(C.Structure):
    """ctypes mirror of fcamd_mr::Args (multilevel_rigid.hip)"""

    _fields_ = [(name, C.c_void_p) for name in ("fine_values", "coarse_values", "fold_ptr", "fold", "dest_base", "dest_stride", "block_row", "indices",
                                                "offsets", "mem_ptr", "members", "agg", "mask", "b", "q", "x", "xc", "rc", "sc")] + \
               [("n", C.c_int64), ("n_coarse", C.c_int64), ("use_q", C.c_int32), ("pad", C.c_int32)]


class Args(C.Structure):
    """ctypes mirror of fcamd_ml::Args (multilevel.hip)"""

    _fields_ = [(name, C.c_void_p) for name in ("fine_values", "coarse_values", "fold_ptr", "fold", "dest_base", "dest_stride", "mem_ptr", "members", "agg",
                                                "mask", "b", "q", "x", "xc", "rc", "inv", "r", "z", "p", "partials", "sc")] + \
               [("omega", C.c_double), ("n", C.c_int64), ("n_coarse", C.c_int64), ("nseg", C.c_int64),
                ("first", C.c_int32), ("plain", C.c_int32), ("use_q", C.c_int32), ("start", C.c_int32)]


class FreeArgs(C.Structure):
    """ctypes mirror of fcamd_mf::Args (multilevel_free.hip)"""

    _fields_ = [(name, C.c_void_p) for name in ("ke", "blk_ptr", "contrib", "dofmap", "mask", "block_row", "block_col", "mem_ptr", "members", "values")] + \
               [("entry0", C.c_int64), ("n_entries", C.c_int64), ("key_lo", C.c_int64), ("key_hi", C.c_int64), ("cell0", C.c_int64),
                ("first", C.c_int32), ("pad", C.c_int32)]


class FreeRigidArgs(C.Structure):
    """ctypes mirror of fcamd_mfr::Args (multilevel_free_rigid.hip)"""

    _fields_ = [(name, C.c_void_p) for name in ("ke", "blk_ptr", "contrib", "dofmap", "mask", "block_row", "block_col", "mem_ptr", "members", "offsets",
                                                "values")] + \
               [("block0", C.c_int64), ("block1", C.c_int64), ("key_lo", C.c_int64), ("key_hi", C.c_int64), ("cell0", C.c_int64),
                ("first", C.c_int32), ("pad", C.c_int32)]


# ---- the seam of level 0 -----------------------------------------------------------------------------------------------------------
# What the preconditioner alone asks of its fine level: the pattern the hierarchy is built from, the launches of a product, the first
# Galerkin step, and the device pointers of all that a cached launch plan holds.  The check of the first argument of a call, the node
# without a diagonal block and the array the inverse kernel reads the nodes' own blocks from are the solver's seam's (``solver._Seam``).
class _AssembledFine:
    """level 0 is a ``TangentMatrix``: its values array is read where ``dest_base`` / ``dest_stride`` say"""

    free = False

    def __init__(self, K: TangentMatrix):
        self.K = K
        self.indptr, self.indices = K.indptr, K.indices

    def product(self, pc, dev: int, values, control, x_ptr: int, q_ptr: int, cap: int) -> list:
        a = pc._level_args(dev, 0, values, control)
        a.va, a.q, a.mode = x_ptr, q_ptr, _MODE_QUIET
        return [(pc._code, solver.MATVEC_KERNEL, max(1, min(int(a.nseg), cap)), a, "MultilevelPreconditioner matrix-vector launch")]

    def key(self, pc, dev: int) -> tuple:
        return tuple(t.data_ptr() for t in pc._op.tables(dev))


class _FreeFine:
    """Level 0 is a ``TangentOperator``: there is no values array.  The nodes' own blocks are ``A.diagonal_blocks(tangent)`` in a block
    array of the preconditioner's, a product is the operator's two launches in quiet mode, and the values of level 1 are gathered
    from the element matrices of ``fcamd_tangent_matrix_element_kernel`` -- compiled here through ``matrix.compile_kernels``, no
    ``TangentMatrix`` is constructed -- which pass in ascending whole-tile chunks through a scratch of at most ``A.scratch_bytes``."""

    free = True

    def __init__(self, A: TangentOperator):
        self.K = A
        d_, a_ = A.gdim, A.nodes_per_cell
        m = a_ * d_
        self.cells_per_tile = cw = _matrix.cells_per_tile(d_, a_)
        # (the scratch itself is the preconditioner's: ``_OnDevice.ke``, with its other tensors)
        self._pass = ChunkedPass(A.force, A.scratch_bytes, m * m * 8, cw, lambda have, tile: f"the operator's scratch_bytes = {have} does not hold one tile of "
                                 f"{cw} element matrices of {m} x {m} doubles ({tile} bytes): the multilevel preconditioner forms its first coarse level from them")
        self.chunk_cells = self._pass.chunk_cells
        # the pattern of the TangentMatrix of the same force; a node of no cell (that matrix would lack its diagonal block) gets a row of
        # its own block, as a pattern_dofmap with a cell of its own would give it: the block is zero, the status of a setup singular_block
        unused = np.flatnonzero(A.valence == 0).astype(np.int32)
        cells = A.op._dofmap if not unused.size else np.concatenate([A.op._dofmap, np.repeat(unused[:, None], a_, axis=1)])
        self.indptr, self.indices = _matrix.block_pattern(cells, A.n_nodes)
        self.element_code = self.gather_code = None
        self.blk_ptr = self.contributions = self.block_row = None
        self.chunk_blocks = []

    def chunks(self):
        """the ascending cell ranges ``(first, end)`` whose element matrices pass through the scratch one after the other"""
        return self._pass.chunks()

    def build(self, levels: list, rigid: bool = False) -> None:
        """the programs and, with a coarse level, its contribution lists (host); ``rigid``: the gather of multilevel_free_rigid.hip"""
        A = self.K
        d_, a_ = A.gdim, A.nodes_per_cell
        self.element_code = _matrix.compile_kernels(d_, a_, A.points_per_cell, A.op.affine)  # (no kernel of it has scratch, or this raises)
        self.gather_code = compile_free_rigid_kernels(d_, a_) if rigid else compile_free_kernels(d_, a_)
        if len(levels) < 2:
            return
        fine, coarse = levels[0], levels[1]
        self.blk_ptr, self.contributions = _matrix.contribution_lists(fine.agg[A.op._dofmap], coarse.n_nodes, coarse.indptr, coarse.indices)
        self.block_row = coarse.block_row
        # the range of coarse blocks every chunk's cells touch: a later chunk's gather runs over it alone
        self.chunk_blocks = self._pass.block_ranges(self.contributions, self.blk_ptr, coarse.nnzb, a_ * a_)

    def product(self, pc, dev: int, tangent, control, x_ptr: int, q_ptr: int, cap: int) -> list:
        # (quiet mode neither reads nor writes the control block: a product enqueued behind the end of a solve writes the
        # preconditioner's own q and nothing else, and every kernel that would read q returns at once)
        return self.K._launches(dev, tangent.data_ptr(), x_ptr, q_ptr, _MODE_QUIET)

    def key(self, pc, dev: int) -> tuple:
        # (the element forces between the product's two kernels are ``force``'s own buffer: made once, kept as long as the operator)
        A = self.K
        held = [*pc._op.tables(dev), *A.force._tables(dev)] + ([*A.op._tables(dev)[:3]] if A.n_cells else [])
        return tuple(t.data_ptr() for t in held)

    def galerkin(self, pc, dev: int, tangent, cap: int) -> None:
        """the values of level 1 from the tangent: per chunk the element kernel, then the gather of multilevel_free.hip or, with the
        rigid-body coarse space, of multilevel_free_rigid.hip"""
        import torch

        A, on = self.K, pc._device(dev)
        d_, a_ = A.gdim, A.nodes_per_cell
        dd = d_ * d_
        dofmap, ref, _, _ = A.op._tables(dev)
        mask = A._mask_table(dev)
        t0, t1 = on.tables[0], on.tables[1]
        common = (on.ke.data_ptr(), t1["blk_ptr"].data_ptr(), t1["contrib"].data_ptr(), dofmap.data_ptr(), 0 if mask is None else mask.data_ptr(),
                  t1["block_row"].data_ptr(), t1["indices"].data_ptr(), t0["mem_ptr"].data_ptr(), t0["members"].data_ptr())
        if pc._rigid:  # multilevel_free_rigid.hip: a group of lanes per coarse block
            lanes, what = {2: 16, 3: 64}[d_], "MultilevelPreconditioner first rigid-body Galerkin launch"
            ga = FreeRigidArgs(*common, t0["offset"].data_ptr(), on.values[1].data_ptr(), 0, 0, 0, 0, 0, 1, 0)
        else:  # multilevel_free.hip: a lane per entry
            lanes, what = dd, "MultilevelPreconditioner first Galerkin launch"
            ga = FreeArgs(*common, on.values[1].data_ptr(), 0, 0, 0, 0, 0, 1, 0)

        def cover(lo, hi):
            """the launch covers the coarse blocks ``lo .. hi``: its thread blocks"""
            if pc._rigid:
                ga.block0, ga.block1 = lo, hi
            else:
                ga.entry0, ga.n_entries = dd * lo, dd * hi
            return pc._blocks(lanes * (hi - lo), cap)

        gather_blocks = cover(0, pc._levels[1].nnzb)
        with torch.cuda.device(dev):
            for k, c0, c1, tangent_ptr, jinv_ptr, weights_ptr, element_blocks in self._pass.walk(dev, tangent, cap):
                ea = _matrix.ElementArgs(tangent_ptr, ref.data_ptr(), jinv_ptr, weights_ptr, on.ke.data_ptr(), c1 - c0)
                jit.launch(self.element_code, dev, element_blocks, ea, "MultilevelPreconditioner element launch")
                ga.key_lo, ga.key_hi, ga.cell0, ga.first = c0 * a_ * a_, c1 * a_ * a_, c0, 1 if k == 0 else 0
                if k:  # the first chunk starts every entry; a later one visits the coarse blocks its cells touch
                    gather_blocks = cover(*self.chunk_blocks[k])
                jit.launch(self.gather_code, dev, gather_blocks, ga, what)


class _OnDevice:
    """the hierarchy's tables, values and vectors on one device"""

    def __init__(self, pc, dev: int):
        import torch

        from .hostio import to_device

        d = torch.device("cuda", dev)
        dofs = pc._dofs  # per node, by level

        def zeros(n):
            return torch.zeros(max(int(n), 2), dtype=torch.float64, device=d)

        self.dummy = to_device(np.zeros(1, dtype=np.int32), d)
        self.tables, self.values, self.inv, self.b, self.x, self.q = [], [None], [], [None], [None], []
        for l, lv in enumerate(pc._levels):
            t = {}
            if l > 0:
                t["indptr"], t["indices"] = to_device(lv.indptr, d), to_device(lv.indices, d)
                t["diag"] = to_device(np.maximum(lv.diag_block, 0).astype(np.int32), d)
                self.values.append(zeros(dofs[l]**2 * lv.nnzb))
                self.b.append(zeros(dofs[l] * lv.n_nodes))
                self.x.append(zeros(dofs[l] * lv.n_nodes))
            if lv.agg is not None:
                # (an operator's level 0 has no blocks to fold: its fold lists, as long as the fine pattern, stay on the host)
                folds = () if l == 0 and pc._seam.free else ("fold_ptr", "fold")
                # (the rigid-body transfers read the offsets; the (Df, Dc) Galerkin kernel of a level with values the nodes of its blocks too)
                rigid = () if not pc._rigid else ("offset",) if l == 0 and pc._seam.free else ("block_row", "indices", "offset")
                for name in ("agg", "mem_ptr", "members") + folds + rigid:
                    if name not in t:  # (a coarse level's column nodes are there already)
                        t[name] = to_device(getattr(lv, name), d)
            if l == 1 and pc._seam.free:  # the lists of the first Galerkin step
                t["blk_ptr"], t["contrib"] = (to_device(x, d) for x in (pc._seam.blk_ptr, pc._seam.contributions))
                if "block_row" not in t:  # (with the rigid-body space and a level 2 it is there already)
                    t["block_row"] = to_device(pc._seam.block_row, d)
            self.tables.append(t)
            self.inv.append(zeros(dofs[l]**2 * lv.n_nodes))
            self.q.append(zeros(dofs[l] * lv.n_nodes))
        self.blocks = None  # (a matrix has its nodes' own blocks in its values)
        if pc._seam.free:  # the nodes' own blocks of level 0 and, with a coarse level, the element matrices of a chunk of cells
            A, seam = pc.K, pc._seam
            self.blocks = zeros(A.gdim**2 * A.n_nodes)[: A.gdim**2 * A.n_nodes]
            if len(pc._levels) > 1:
                self.ke = zeros(min(seam.chunk_cells, A.n_cells) * (A.nodes_per_cell * A.gdim)**2)
        self.control = None  # of setup() and apply()
        self.plans = {}  # key -> (launch plan, what it keeps alive), the last PLANS used


class MultilevelPreconditioner:
    """``MultilevelPreconditioner(K, cycle, smoothing, omega, coarsest_nodes, coarsest_sweeps, max_levels)``: the aggregation
    multilevel preconditioner of ``K`` (a ``TangentMatrix`` in either format), for ``ConjugateGradient(K, preconditioner=...)``.

    ``cycle``: "multiplicative" -- a V cycle with ``smoothing`` damped block-Jacobi sweeps before and after the coarse correction,
    ``2 smoothing`` fine products per application (the first sweep starts from zero and needs none; one for the residual, one in
    every later sweep) and the same on every coarse level -- or "additive" -- block-Jacobi on every level, no fine product.  ``omega``: the
    damping of the sweeps (``omega * lambda_max(D^-1 K) < 2`` IS NEEDED AND NOT CHECKED, see the module docstring).  The hierarchy
    stops at a level of at most ``coarsest_nodes`` nodes or at ``max_levels``; there ``coarsest_sweeps`` sweeps from zero stand for a
    solve.  Built on the host at construction from the pattern alone, with the kernels compiled there (no GPU needed); a level
    with a node without a diagonal block is refused.  ``levels``, ``aggregates(l)``, ``pattern(l)``, ``members(l)``, ``folds(l)`` and
    ``roots(l)`` show the tables.  All value and vector tensors of the hierarchy belong to the object, one set per device,
    allocated at the first call; use an object from one stream at a time.

    ``coarse_space``: "translations" (the default: ``D x D`` coarse blocks, an aggregate moves as a whole) or "rigid_body" with
    ``coordinates``, the float64 array ``[K.n_nodes][K.gdim]`` of the positions of the pattern's nodes: an aggregate rotates too, the
    nodes of the levels ``l >= 1`` carry ``coarse_dofs`` = 6 (3-D) or 3 (2-D) dofs (module docstring; 1-D: the translation
    hierarchy).  A level-0 aggregate whose rigid-body modes are linearly dependent -- a lone node, all members at one point, in 3-D
    all on one line -- is a ``ValueError`` that names it, raised before anything is compiled.  ``positions(l)`` and ``offsets(l)``
    show where the nodes were placed.

    ``K`` may be a ``TangentOperator`` instead (module docstring, "On a matrix-free operator"): the hierarchy is that of the
    ``TangentMatrix`` of the same force, ``setup(tangent)``, ``apply(tangent, r, out=None)`` and ``ConjugateGradient(A, preconditioner=pc)(tangent,
    b)`` take the ``S*S n_points`` tangent where the values stood, and no matrix is formed: level 1 is gathered from the element matrices,
    which pass through a scratch of ``A.scratch_bytes`` (less than one tile of ``matrix.cells_per_tile`` element matrices: a
    ``ValueError``).  ``coarse_space="rigid_body"`` with ``coordinates`` works on an operator as on a matrix (level 1 is gathered as
    ``P_i^T ke P_j`` with the offsets of level 0); there, coordinates that put all nodes at one point are a ``ValueError`` whatever the
    number of levels: the rotations vanish.  A node in no cell has a zero
    block of its own on every level it reaches: ``setup`` and ``apply`` end with the status ``singular_block`` (nothing is applied), and
    ``ConjugateGradient`` refuses such an operator at construction."""

    def __init__(self, K: TangentMatrix, cycle: str = "multiplicative", smoothing: int = 1, omega: float = 0.5, coarsest_nodes: int = 64,
                 coarsest_sweeps: int = 8, max_levels: int = 10, coarse_space: str = "translations", coordinates=None):
        if not isinstance(K, (TangentMatrix, TangentOperator)):
            raise TypeError(f"K must be a TangentMatrix or a TangentOperator, got {type(K).__name__}")
        if cycle not in CYCLES:
            raise ValueError(f"cycle must be one of {CYCLES}, got {cycle!r}")
        if not (isinstance(coarse_space, str) and coarse_space in COARSE_SPACES):
            raise ValueError(f"coarse_space must be one of {COARSE_SPACES}, got {coarse_space!r}")
        if coarse_space == "translations":
            if coordinates is not None:
                raise ValueError('coordinates belong to coarse_space="rigid_body"; the translations need none')
        else:
            if coordinates is None:
                raise ValueError('coarse_space="rigid_body" needs coordinates, the positions [n_nodes][gdim] of the nodes of the pattern')
            if not isinstance(coordinates, np.ndarray):
                raise TypeError(f"coordinates must be a NumPy array, got {type(coordinates).__name__}")
            if coordinates.dtype != np.float64:
                raise TypeError(f"coordinates must be float64, got {coordinates.dtype}")
            if coordinates.shape != (K.n_nodes, K.gdim):
                raise ValueError(f"coordinates must have the shape {(K.n_nodes, K.gdim)}, got {coordinates.shape}")
            if not np.isfinite(coordinates).all():
                raise ValueError("coordinates must be finite")
            if isinstance(K, TangentOperator) and K.gdim > 1 and K.n_nodes > 1 and (coordinates == coordinates[0]).all():
                raise ValueError(f'coordinates put all {K.n_nodes} nodes at one point: every offset is zero and the rotations vanish, so coarse_space="rigid_body" '
                                 'has a singular coarse level; pass the positions of the nodes or use coarse_space="translations"')
        if isinstance(omega, bool) or not isinstance(omega, (int, float, np.integer, np.floating)):
            raise TypeError(f"omega must be a number, got {type(omega).__name__}")
        if not (omega > 0.0 and np.isfinite(omega)):
            raise ValueError(f"omega must be finite and positive, got {omega}")
        for name, v in (("smoothing", smoothing), ("coarsest_nodes", coarsest_nodes), ("coarsest_sweeps", coarsest_sweeps), ("max_levels", max_levels)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{name} must be an integer, got {type(v).__name__}")
            if v < 1 or v >= 2**31:
                raise ValueError(f"{name} must lie in [1, 2^31), got {v}")
        seam = _FreeFine(K) if isinstance(K, TangentOperator) else _AssembledFine(K)  # (an operator: raises the ValueError of its scratch)
        self._op = solver._operator(K)
        if not seam.free:  # (an operator's node of no cell has a row of its own block in the pattern, and a zero block at setup)
            self._op.refuse_missing()
        self.K = K
        self._seam = seam
        # fixed for the life of the object (read-only properties below): the launch plan of a cycle is built from them
        self._cycle_name, self._smoothing, self._omega = cycle, int(smoothing), float(omega)
        self._coarsest_nodes, self._coarsest_sweeps, self._max_levels = int(coarsest_nodes), int(coarsest_sweeps), int(max_levels)
        self._levels = hierarchy(seam.indptr, seam.indices, self.coarsest_nodes, self.max_levels)
        for l, lv in enumerate(self._levels):
            missing = np.flatnonzero(lv.diag_block < 0)
            if missing.size:
                raise ValueError(f"node {int(missing[0])} of level {l} has no diagonal block in the pattern")
        self._coarse_space = coarse_space
        #: the coarse nodes carry rotations (in 1-D there is none: the translation hierarchy, its program and its bits)
        self._rigid = coarse_space == "rigid_body" and K.gdim > 1
        if coordinates is not None:
            place(self._levels, coordinates)
            if self._rigid and len(self._levels) > 1:
                _refuse_degenerate(self._levels[0])
        #: dofs per node, by level
        self._dofs = [K.gdim] + [coarse_dofs(K.gdim) if self._rigid else K.gdim] * (len(self._levels) - 1)
        if self._rigid:
            self._code, self._coarse_code = compile_rigid_kernels(K.gdim)
        else:
            self._code = self._coarse_code = compile_kernels(K.gdim)
        if seam.free:
            seam.build(self._levels, self._rigid)
        self._on = {}  # device index -> _OnDevice

    # ---- what was asked for (read-only) ----------------------------------------------------------------------------------------
    cycle = property(lambda self: self._cycle_name)
    smoothing = property(lambda self: self._smoothing)
    omega = property(lambda self: self._omega)
    coarsest_nodes = property(lambda self: self._coarsest_nodes)
    coarsest_sweeps = property(lambda self: self._coarsest_sweeps)
    max_levels = property(lambda self: self._max_levels)
    coarse_space = property(lambda self: self._coarse_space)

    # ---- what was built --------------------------------------------------------------------------------------------------------
    @property
    def levels(self) -> list:
        """``[{"nodes", "blocks"}]``, finest first"""
        return [{"nodes": lv.n_nodes, "blocks": lv.nnzb} for lv in self._levels]

    def _fine(self, l: int) -> Level:
        if not 0 <= l < len(self._levels) - 1:
            raise ValueError(f"level {l} has no coarser level (the hierarchy has {len(self._levels)})")
        return self._levels[l]

    def aggregates(self, l: int) -> np.ndarray:
        """the aggregate (the node of level ``l + 1``) of every node of level ``l``"""
        return self._fine(l).agg

    def roots(self, l: int) -> np.ndarray:
        """the root of every aggregate of level ``l`` (a lone node is its own)"""
        return self._fine(l).roots

    def members(self, l: int):
        """``(mem_ptr, members)``: the members of every aggregate of level ``l``, ascending"""
        return self._fine(l).mem_ptr, self._fine(l).members

    def folds(self, l: int):
        """``(fold_ptr, fold)``: for every block of level ``l + 1`` the blocks of level ``l`` that fold into it, ascending"""
        return self._fine(l).fold_ptr, self._fine(l).fold

    def pattern(self, l: int):
        """``(indptr, indices)`` of level ``l``, block CSR"""
        if not 0 <= l < len(self._levels):
            raise ValueError(f"there is no level {l} (the hierarchy has {len(self._levels)})")
        return self._levels[l].indptr, self._levels[l].indices

    def diag_block(self, l: int) -> np.ndarray:
        self.pattern(l)
        return self._levels[l].diag_block

    @property
    def coarse_dofs(self) -> int:
        """``Dc``: the dofs of a node of the levels ``l >= 1`` (``D`` with the translations)"""
        return coarse_dofs(self.K.gdim) if self._rigid else self.K.gdim

    def positions(self, l: int) -> np.ndarray:
        """``[nodes][D]``: the position of every node of level ``l`` (``coarse_space="rigid_body"``)"""
        self.pattern(l)
        if self._levels[l].position is None:
            raise ValueError('only coarse_space="rigid_body" places the nodes')
        return self._levels[l].position

    def offsets(self, l: int) -> np.ndarray:
        """``[nodes][D]``: the offset of every node of level ``l`` from the position of its aggregate (``coarse_space="rigid_body"``)"""
        if self._fine(l).offset is None:
            raise ValueError('only coarse_space="rigid_body" places the nodes')
        return self._fine(l).offset

    @property
    def resources(self) -> dict:
        """the compiler's remarks of the five multilevel kernels, by "galerkin", "restrict", "prolong", "smooth" and "close" """
        r = {kernel[len("fcamd_ml_"): -len("_kernel")]: kernel_resources(self._code.log, kernel) for kernel in KERNELS}
        if self._rigid:  # the three transfer kernels of the pair (D, Dc), and under "coarse" every kernel of the coarse program by its name
            r.update({"rigid_" + kernel[len("fcamd_mr_"): -len("_kernel")]: kernel_resources(self._code.log, kernel) for kernel in RIGID_KERNELS})
            r["coarse"] = {kernel: kernel_resources(self._coarse_code.log, kernel) for kernel in solver.KERNELS + KERNELS + RIGID_KERNELS}
        if self._seam.free:  # the two kernels of the first Galerkin step of an operator: its gather (of either coarse space) and the element kernel
            if self._rigid:
                r["free_rigid_galerkin"] = kernel_resources(self._seam.gather_code.log, FREE_RIGID_GALERKIN_KERNEL)
            else:
                r["free_galerkin"] = kernel_resources(self._seam.gather_code.log, FREE_GALERKIN_KERNEL)
            r["free_element"] = kernel_resources(self._seam.element_code.log, _matrix.ELEMENT_KERNEL)
        return r

    @property
    def compile_log(self) -> str:
        return self._code.log

    @property
    def coarse_compile_log(self) -> str:
        """the log of the program of the levels ``l >= 1`` (with the translations: the one program there is)"""
        return self._coarse_code.log

    @staticmethod
    def lds_bytes(kernel: str = CLOSE_KERNEL, gdim: int = 3) -> int:
        return lds_bytes(kernel, gdim)

    @property
    def device(self) -> int:
        return self.K.device

    # ---- launches --------------------------------------------------------------------------------------------------------------
    def _device(self, dev: int) -> _OnDevice:
        on = self._on.get(dev)
        if on is None:
            import torch

            with torch.cuda.device(dev):
                on = self._on[dev] = _OnDevice(self, dev)
        return on

    def _level_args(self, dev: int, l: int, values, control) -> solver.Args:
        """the solver's arguments of level ``l``: its matrix for the product and the inverse kernel"""
        if l == 0:
            a = self._op.args(dev, values, control)
        else:
            on, lv, t = self._device(dev), self._levels[l], self._device(dev).tables[l]
            d_ = self._dofs[l]
            a = solver.Args()
            a.values, a.indptr, a.indices, a.diag, a.groups = (on.values[l].data_ptr(), t["indptr"].data_ptr(), t["indices"].data_ptr(), t["diag"].data_ptr(),
                                                               on.dummy.data_ptr())
            a.partials, a.sc = control.partials.data_ptr(), control.device_block.data_ptr()
            a.n, a.nnz, a.nseg, a.n_nodes, a.csr = d_ * lv.n_nodes, d_ * d_ * lv.nnzb, solver._segments(d_ * lv.n_nodes), lv.n_nodes, 0
        a.inv = self._device(dev).inv[l].data_ptr()
        return a

    def _program(self, l: int):
        """the code object of level ``l``'s own kernels and of the transfers between it and level ``l + 1``"""
        return self._code if l == 0 else self._coarse_code

    @staticmethod
    def _blocks(n: int, cap: int) -> int:
        return max(1, blocks_for(n, cap))  # a lane per entry, never an empty grid

    def _setup(self, dev: int, values, control) -> None:
        """the Galerkin values of every coarse level, then the inverses of every level's own blocks (asynchronous)"""
        on, cap, dd = self._device(dev), BLOCKS_PER_CU * jit.num_cu(dev), self.K.gdim**2
        tables = None if self._seam.free else self.K._tables(dev)
        for l, lv in enumerate(self._levels[:-1]):
            if l == 0 and self._seam.free:  # no values to fold: level 1 straight from the element matrices
                self._seam.galerkin(self, dev, values, cap)
                continue
            if self._rigid:
                a, t = RigidArgs(), on.tables[l]
                a.fine_values = (values if l == 0 else on.values[l]).data_ptr()
                a.coarse_values = on.values[l + 1].data_ptr()
                a.fold_ptr, a.fold, a.block_row, a.indices, a.offsets = (t[name].data_ptr() for name in ("fold_ptr", "fold", "block_row", "indices", "offset"))
                if l == 0:
                    a.dest_base, a.dest_stride = tables[2].data_ptr(), tables[3].data_ptr()
                a.sc = control.device_block.data_ptr()
                a.n_coarse = self._dofs[l + 1]**2 * self._levels[l + 1].nnzb
                jit.launch(self._program(l), dev, self._blocks(a.n_coarse, cap), a, "MultilevelPreconditioner rigid-body Galerkin launch", kernel=RIGID_GALERKIN_KERNEL)
                continue
            a = Args()
            a.fine_values = (values if l == 0 else on.values[l]).data_ptr()
            a.coarse_values = on.values[l + 1].data_ptr()
            a.fold_ptr, a.fold = on.tables[l]["fold_ptr"].data_ptr(), on.tables[l]["fold"].data_ptr()
            if l == 0:
                a.dest_base, a.dest_stride = tables[2].data_ptr(), tables[3].data_ptr()
            a.sc = control.device_block.data_ptr()
            a.n_coarse = dd * self._levels[l + 1].nnzb
            jit.launch(self._code, dev, self._blocks(a.n_coarse, cap), a, "MultilevelPreconditioner Galerkin launch", kernel=GALERKIN_KERNEL)
        for l, lv in enumerate(self._levels):
            a = self._level_args(dev, l, values, control)
            if l == 0:  # (a matrix: its values; an operator: the block array its diagonal kernels fill here)
                a.values = self._op.own_blocks(dev, values, on.blocks)
            jit.launch(self._program(l), dev, self._blocks(lv.n_nodes, cap), a, "MultilevelPreconditioner inverse launch", kernel=solver.INVERSE_KERNEL)

    def _plan(self, dev: int, values, control, r_ptr: int, z_ptr: int) -> list:
        """the launches of one application ``z = M^-1 r``: ``[(code, kernel, blocks, args, what)]``"""
        on, cap = self._device(dev), BLOCKS_PER_CU * jit.num_cu(dev)
        mask = self.K._mask_table(dev)
        sc = control.device_block.data_ptr()
        n_of = [d_ * lv.n_nodes for d_, lv in zip(self._dofs, self._levels)]
        b_of = [r_ptr] + [t.data_ptr() for t in on.b[1:]]
        x_of = [z_ptr] + [t.data_ptr() for t in on.x[1:]]
        q_of = [t.data_ptr() for t in on.q]
        last = len(self._levels) - 1
        ops = []

        def product(l):
            if l == 0:  # one launch of the matrix-vector kernel, or the operator's two
                ops.extend(self._seam.product(self, dev, values, control, x_of[0], q_of[0], cap))
                return
            a = self._level_args(dev, l, values, control)
            a.va, a.q, a.mode = x_of[l], q_of[l], _MODE_QUIET
            ops.append((self._program(l), solver.MATVEC_KERNEL, max(1, min(int(a.nseg), cap)), a, "MultilevelPreconditioner matrix-vector launch"))

        def smooth(l, first=0, plain=0, use_q=0):
            a = Args()
            a.b, a.q, a.x, a.inv, a.sc, a.omega, a.n = b_of[l], q_of[l], x_of[l], on.inv[l].data_ptr(), sc, self.omega, n_of[l]
            a.first, a.plain, a.use_q = first, plain, use_q
            ops.append((self._program(l), SMOOTH_KERNEL, self._blocks(n_of[l], cap), a, "MultilevelPreconditioner smoothing launch"))

        def sweeps(l, count, from_zero):
            for i in range(count):
                if from_zero and i == 0:
                    smooth(l, first=1)
                else:
                    product(l)
                    smooth(l, use_q=1)

        def restrict(l, use_q):
            a, t = (RigidArgs() if self._rigid else Args()), on.tables[l]
            if self._rigid:
                a.offsets = t["offset"].data_ptr()
            a.mem_ptr, a.members, a.b, a.q, a.rc, a.sc, a.n_coarse, a.use_q = t["mem_ptr"].data_ptr(), t["members"].data_ptr(), b_of[l], q_of[l], b_of[l + 1], sc, n_of[l + 1], use_q
            ops.append((self._program(l), RIGID_RESTRICT_KERNEL if self._rigid else RESTRICT_KERNEL, self._blocks(n_of[l + 1], cap), a,
                        "MultilevelPreconditioner restriction launch"))

        def prolong(l):
            a = RigidArgs() if self._rigid else Args()
            if self._rigid:
                a.offsets = on.tables[l]["offset"].data_ptr()
            a.agg, a.x, a.xc, a.sc, a.n = on.tables[l]["agg"].data_ptr(), x_of[l], x_of[l + 1], sc, n_of[l]
            if l == 0 and mask is not None:
                a.mask = mask.data_ptr()
            ops.append((self._program(l), RIGID_PROLONG_KERNEL if self._rigid else PROLONG_KERNEL, self._blocks(n_of[l], cap), a,
                        "MultilevelPreconditioner prolongation launch"))

        if self.cycle == "additive":
            for l in range(last):
                smooth(l, plain=1)
                restrict(l, 0)
            sweeps(last, self.coarsest_sweeps, True)
            for l in range(last - 1, -1, -1):
                prolong(l)
        else:
            for l in range(last):
                sweeps(l, self.smoothing, True)
                product(l)
                restrict(l, 1)
            sweeps(last, self.coarsest_sweeps, True)
            for l in range(last - 1, -1, -1):
                prolong(l)
                sweeps(l, self.smoothing, False)
        return ops

    def _cycle(self, dev: int, values, control, r_ptr: int, z_ptr: int) -> None:
        """``z = M^-1 r`` with the values ``_setup`` left (asynchronous)"""
        on = self._device(dev)
        mask = self.K._mask_table(dev)
        # every device pointer the plan's arguments hold that is not the object's own: the values, the control block and its
        # partial sums, the vectors, the mask and the level-0 tables.  The control and the mask are kept alive with the plan, so
        # that their addresses cannot be handed to other tensors while it is cached.
        key = (values.data_ptr(), control.device_block.data_ptr(), control.partials.data_ptr(), r_ptr, z_ptr, None if mask is None else mask.data_ptr(),
               self._seam.key(self, dev), jit.num_cu(dev), self._coarse_space)
        have = on.plans.pop(key, None)  # (taken out and put back: the dict keeps the order of the last use)
        if have is None:
            have = (self._plan(dev, values, control, r_ptr, z_ptr), (control, mask))
            while len(on.plans) >= PLANS:
                del on.plans[next(iter(on.plans))]
        on.plans[key] = have
        for code, kernel, blocks, a, what in have[0]:
            jit.launch(code, dev, blocks, a, what, kernel=kernel)

    def _close(self, dev: int, control, r, z, p, start: bool) -> None:
        """the closing kernel behind a cycle: ``rz``, ``rz_old``, in the start ``p = z``"""
        a = Args()
        a.r, a.z, a.p, a.partials, a.sc = r.data_ptr(), z.data_ptr(), p.data_ptr(), control.partials.data_ptr(), control.device_block.data_ptr()
        a.n, a.nseg, a.start = self._op.n, self._op.nseg, 1 if start else 0
        jit.launch(self._code, dev, self._op.blocks(dev), a, "MultilevelPreconditioner closing launch", kernel=CLOSE_KERNEL)

    def _own_control(self, dev: int):
        on = self._device(dev)
        if on.control is None:
            on.control = solver._Control(dev, self._op.nseg)
        on.control.upload()
        return on.control

    # ---- standalone --------------------------------------------------------------------------------------------------------------
    def setup(self, values) -> list:
        """The value tensors of the coarse levels (block CSR, ``[blocks][D][D]`` flat; ``[blocks][Dc][Dc]`` with the rigid-body modes), finest first, formed from ``values`` with the
        inverses of every level (asynchronous, on torch's current stream).  The tensors are the object's own: the next call writes
        them again."""
        import torch

        dev = self.device
        self._op.check(values, dev)
        with torch.cuda.device(dev):
            if self.K.shape[0]:
                self._setup(dev, values, self._own_control(dev))
            on = self._device(dev)
            return [on.values[l][: self._dofs[l]**2 * lv.nnzb] for l, lv in enumerate(self._levels) if l > 0]

    def apply(self, values, r, out=None):
        """``out = M^-1 r`` for the matrix ``values`` (asynchronous, on torch's current stream); ``out`` must not alias ``r``.  With a
        singular block on any level nothing is applied and ``out`` is left as it was."""
        import torch

        dev, n = self.device, self.K.shape[0]
        self._op.check(values, dev)
        self.K._check("r", r, n, dev)
        if out is not None:
            self.K._check("out", out, n, dev)
            if solver._overlap(out, r):
                raise ValueError("out must not alias r")
        with torch.cuda.device(dev):
            if out is None:
                out = torch.zeros(n, dtype=torch.float64, device=torch.device("cuda", dev))
            if n:
                control = self._own_control(dev)
                self._setup(dev, values, control)
                self._cycle(dev, values, control, r.data_ptr(), out.data_ptr())
        return out
