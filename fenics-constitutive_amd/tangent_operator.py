"""The matrix-free tangent operator: ``y = K v`` and the nodes' own blocks of ``K`` from the tangent of the quadrature points.

``TangentMatrix`` writes ``K = sum_p B_p^T C_p B_p w_p`` out as a sparse matrix -- 72 bytes per block next to a tangent array that
sits in HBM anyway.  ``TangentOperator(force)`` applies the same matrix without forming it, constraints included, and is what
``ConjugateGradient`` accepts in a ``TangentMatrix``'s place: the product with the ordered ``p . q`` behind it, and the diagonal
blocks for block-Jacobi.  It covers ONE operator per mesh: the sums over the laws of several submeshes (``accumulate``,
``pattern_dofmap``) are out of scope.

Four run-time compiled kernels (``csrc/jit/tangent_operator.hip``, through ``jit.compile_program`` / ``jit.launch``), no
floating-point atomics, ``-ffp-contract=off``.

*The product.*  With ``M`` the 0/1 diagonal of the free dofs, ``y = M K M v + (I - M) v``: what the assembled matrix does with
identity rows and columns at the constrained dofs.  The element kernel reads ``v`` through the dofmap (``+0.0`` at a constrained
dof), forms the gradient of the point in registers by the producer's arithmetic (``gradient.py``: ``R`` over ``a`` ascending, then
``G`` over ``k`` ascending) and goes on as the tangent form of ``internal_force.hip`` does (``force.py``: ``e``, ``s = C e``, ``T``,
``fe``); no gradient array exists, and no gradient layout.  The node kernel adds every node's entries in ascending ``c*A + a``, gives
a constrained dof ``v``'s own value, and forms the solver's ordered ``v . y`` as the rows complete.  The result is the bits of
``force.tangent_action(tangent, op(where(mask, 0, v)))`` with ``v`` put back at the constrained dofs, for either layout of ``op``.

*The diagonal blocks.*  For every cell and local node ``a`` the element kernel forms ``ke[c][a][.][a][.]`` by the arithmetic of
``matrix.py``'s docstring (the zero entries of ``G`` and their products included), summed over ``q`` ascending, into a bounded
scratch; the node kernel adds each node's entries in ascending ``c*A + a`` and writes the constrained rows and columns as the
constants ``0.0`` and ``1.0``.  The cells go in ascending chunks of at most ``scratch_bytes``; the result is the bits of
``K.diagonal_blocks(K(tangent))`` of a ``TangentMatrix`` of the same force and mask for every chunk size.  That equality needs the
nodes of a cell to be distinct (a repeated node would add off-diagonal element entries to the block): a cell that names a node
twice is refused.

LDS of a block of either element kernel (``lds_bytes``): that of the force operator -- the reference table and four regions of
``64 * D*D`` doubles; the same ``LDS_CAP``.  ``Q`` may be at most 64.

For a tangent that is not symmetric the operator goes under ``bicgstab_free.MatrixFreeBiCGStab``: the element kernel as it stands and a
node kernel of that module's own program (``csrc/jit/bicgstab_free.hip``) that leaves BiCGStab's dots behind the product.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import jit
from ._fe_common import (ChunkedPass, ConstraintMask, blocks_for, check_tensor, compile_ladder, even, kernel_resources, launch_cap, overlap, tile_blocks,
                         vector_registers)
from .force import MANDEL_DIM, MAX_POINTS_PER_CELL, VGPRS_PER_SIMD, InternalForce, cells_per_tile
from .gradient import LDS_CAP, lds_bytes

ELEMENT_KERNEL = "fcamd_tangent_operator_element_kernel"
NODE_KERNEL = "fcamd_tangent_operator_node_kernel"
DIAGONAL_ELEMENT_KERNEL = "fcamd_tangent_operator_diagonal_element_kernel"
DIAGONAL_NODE_KERNEL = "fcamd_tangent_operator_diagonal_node_kernel"
KERNELS = (ELEMENT_KERNEL, NODE_KERNEL, DIAGONAL_ELEMENT_KERNEL, DIAGONAL_NODE_KERNEL)
#: entries of a segment of the solver's ordered dot (solver.SEG)
SEG = 3072
#: the node kernel's modes: those of conjugate_gradient.hip
MODE_ITERATE, MODE_PLAIN, MODE_QUIET = 1, 2, 3
#: the most points of a slab of the diagonal-block kernel
MAX_SLAB = 16

__all__ = ["TangentOperator", "compile_kernels", "diagonal_cells_per_tile", "diagonal_slab", "lds_bytes", "program"]


def diagonal_cells_per_tile(nodes_per_cell: int) -> int:
    """the whole cells one wave of the diagonal-block kernel takes: ``64 // A`` (a lane per local node), at least one"""
    return max(1, 64 // nodes_per_cell)


def diagonal_slab(gdim: int, nodes_per_cell: int, affine: bool) -> int:
    """points of a slab of the diagonal-block kernel: the most (up to ``MAX_SLAB``) whose tangent rows, per-point inverse Jacobians,
    basis gradients and weights fit a wave's region of ``64 * D*D`` doubles, every part padded to 16 bytes (``ValueError`` where not
    even one point does)"""
    s = MANDEL_DIM[gdim]
    for slab in range(MAX_SLAB, 0, -1):
        need = even(slab * s * s) + (0 if affine else even(slab * gdim * gdim)) + even(slab * gdim * nodes_per_cell) + even(slab)
        if need <= 64 * gdim * gdim:
            return slab
    raise ValueError(f"the basis gradients of {nodes_per_cell} nodes x {gdim} at one point do not fit the wave's region of {64 * gdim * gdim} doubles "
                     "of LDS")


def program(gdim: int, nodes_per_cell: int, points_per_cell: int, affine: bool, slab: int, waves: int) -> str:
    """the program text of one shape (the compile cache is keyed by it)"""
    lines = [f"#define FCAMD_TO_D {int(gdim)}", f"#define FCAMD_TO_A {int(nodes_per_cell)}", f"#define FCAMD_TO_Q {int(points_per_cell)}",
             f"#define FCAMD_TO_AFFINE {1 if affine else 0}", f"#define FCAMD_TO_SLAB {int(slab)}", f"#define FCAMD_TO_WAVES {int(waves)}",
             '#include "tangent_operator.hip"']
    return "\n".join(lines) + "\n"


def compile_kernels(gdim: int, nodes_per_cell: int, points_per_cell: int, affine: bool, waves: int | None = None):
    """The code object of one shape, all four kernels in it (no GPU needed).  ``waves``: that register budget of the element
    kernels; ``None``: the first of ``WAVES_LADDER`` at which no kernel has scratch and the product's element kernel keeps to the
    registers of that many waves.  A shape that spills at every budget, ``Q > 64`` or tables that do not fit the LDS: ``ValueError``.
    ``code.waves`` is the budget kept, ``code.slab`` the slab of the diagonal blocks."""
    if gdim not in (1, 2, 3):
        raise ValueError(f"the geometric dimension must be 1, 2 or 3, got {gdim}")
    if nodes_per_cell < 1 or points_per_cell < 1:
        raise ValueError("a cell needs at least one node and one quadrature point")
    if points_per_cell > MAX_POINTS_PER_CELL:
        raise ValueError(f"a cell may have at most {MAX_POINTS_PER_CELL} quadrature points (a wave takes whole cells), got {points_per_cell}")
    need = lds_bytes(gdim, nodes_per_cell, points_per_cell)
    if need > LDS_CAP:
        raise ValueError(f"the reference table of {points_per_cell} x {nodes_per_cell} x {gdim} doubles needs {need} bytes of LDS per block "
                         f"with the wave regions; at most {LDS_CAP} fit")
    slab = diagonal_slab(gdim, nodes_per_cell, affine)
    name = f"tangent_operator_{gdim}d_{nodes_per_cell}n_{points_per_cell}q"
    # __launch_bounds__ is a hint: a budget the compiler overran is not the one the kernel runs at
    return compile_ladder(lambda w: program(gdim, nodes_per_cell, points_per_cell, affine, slab, w), name, ELEMENT_KERNEL, waves, KERNELS, slab=slab,
                          accept=lambda log, w: vector_registers(log, ELEMENT_KERNEL) <= VGPRS_PER_SIMD // w,
                          exhausted=lambda s: ValueError(f"{name}: the kernels do not compile without scratch at any register budget (last: {s} bytes per lane)"))


class ElementArgs(C.Structure):
    """ctypes mirror of ElementArgs (tangent_operator.hip)"""

    _fields_ = [(name, C.c_void_p) for name in ("tangent", "v", "dofmap", "mask", "ref", "jinv", "weights", "fe", "sc")] + \
               [("n_cells", C.c_int64), ("mode", C.c_int32), ("pad", C.c_int32)]


class NodeArgs(C.Structure):
    """ctypes mirror of NodeArgs (tangent_operator.hip)"""

    _fields_ = [(name, C.c_void_p) for name in ("fe", "node_ptr", "adj", "v", "mask", "out", "partials", "sc")] + \
               [("n_dofs", C.c_int64), ("nseg", C.c_int64), ("mode", C.c_int32), ("pad", C.c_int32)]


class DiagElementArgs(C.Structure):
    """ctypes mirror of DiagElementArgs (tangent_operator.hip)"""

    _fields_ = [(name, C.c_void_p) for name in ("tangent", "ref", "jinv", "weights", "de")] + [("n_cells", C.c_int64)]


class DiagNodeArgs(C.Structure):
    """ctypes mirror of DiagNodeArgs (tangent_operator.hip)"""

    _fields_ = [(name, C.c_void_p) for name in ("de", "node_ptr", "adj", "mask", "out")] + \
               [("n_entries", C.c_int64), ("key_lo", C.c_int64), ("key_hi", C.c_int64), ("first", C.c_int32), ("pad", C.c_int32)]


class TangentOperator(ConstraintMask):
    """``A(tangent, v) -> y`` and ``A.diagonal_blocks(tangent)``: the tangent stiffness of the mesh of an ``InternalForce`` applied
    without a matrix, on the GPU.

    ``force``: the ``InternalForce`` whose operator (dofmap, reference gradients, inverse Jacobians, device), weights and node
    adjacency are used; their device tables are shared, nothing they hold is uploaded again, and the element forces between the
    product's two kernels live in ``force``'s own buffer.  One operator covers the whole mesh: sums over the laws of several
    submeshes (``accumulate``, ``pattern_dofmap``) are out of scope.  ``scratch_bytes``: the most the cells' diagonal blocks may take
    between the two kernels of ``diagonal_blocks`` (default ``matrix.SCRATCH_BYTES``; at least one tile of
    ``diagonal_cells_per_tile`` cells); the result does not depend on it.

    ``tangent`` is a float64 device tensor of ``S*S * n_points``, ``v`` one of ``D * n_nodes``; ``y`` is ``out`` or a new tensor
    (``out`` must not alias ``v``).  ``set_constrained(mask)`` (bool ``[D n_nodes]``) makes the rows and columns of the constrained
    dofs the identity's: ``y = v`` there, ``v`` counts as ``+0.0`` there elsewhere; the diagonal blocks get the constants ``1.0`` and
    ``0.0``.

    Everything is validated on the host before anything is uploaded or launched (``TypeError`` / ``ValueError`` as for
    ``InternalForce`` and ``TangentMatrix``); a cell that names a node twice, ``Q > 64`` and the LDS cap are refused at construction.
    The kernels are compiled at construction (no GPU needed).  All launches go to torch's current stream and are asynchronous; the
    buffers between the kernels belong to the objects: use one from one stream at a time."""

    def __init__(self, force: InternalForce, scratch_bytes: int | None = None):
        if not isinstance(force, InternalForce):
            raise TypeError(f"force must be an InternalForce, got {type(force).__name__}")
        op = force.op
        d_, a_, q_ = op.gdim, op.nodes_per_cell, op.points_per_cell
        cw = diagonal_cells_per_tile(a_)
        self._pass = ChunkedPass(force, scratch_bytes, a_ * d_ * d_ * 8, cw, lambda have, tile: f"scratch_bytes = {have} does not hold one tile of {cw} cells' "
                                 f"diagonal blocks of {a_} x {d_} x {d_} doubles ({tile} bytes)")
        rows = np.sort(op._dofmap, axis=1)
        twice = np.flatnonzero((rows[:, 1:] == rows[:, :-1]).any(axis=1))
        if twice.size:
            raise ValueError(f"cell {int(twice[0])} names a node twice: its off-diagonal element entries would belong to the node's own block")
        self._code = compile_kernels(d_, a_, q_, op.affine)  # (raises the ValueError of Q > 64, of the LDS cap and of the registers)
        self.force, self.op = force, op
        self.gdim, self.nodes_per_cell, self.points_per_cell = d_, a_, q_
        self.n_cells, self.n_points, self.n_nodes = op.n_cells, op.n_points, op.n_nodes
        self.tangent_dim = MANDEL_DIM[d_] ** 2
        self.shape = (d_ * op.n_nodes, d_ * op.n_nodes)
        self.scratch_bytes, self.chunk_cells = self._pass.scratch_bytes, self._pass.chunk_cells
        self.diagonal_cells_per_tile = cw
        #: cells of every node: a node of none has an empty row
        self.valence = np.diff(force.node_ptr.astype(np.int64))
        self._mask_on = {}  # device index -> (version, mask tensor)
        self._scratch = {}  # device index -> the diagonal blocks of a chunk's cells

    # ---- what the compiler made ------------------------------------------------------------------------------------------------
    @property
    def resources(self) -> dict:
        """``{"vgprs", "sgprs", "scratch_bytes", "lds_bytes", "waves_per_simd", ...}`` of the product's element kernel, under "node",
        "diagonal_element" and "diagonal_node" those of the other kernels (compiler remarks), under "waves" the register budget
        kept and under "slab" the points per slab of the diagonal blocks"""
        r = kernel_resources(self._code.log, ELEMENT_KERNEL)
        for name, kernel in (("node", NODE_KERNEL), ("diagonal_element", DIAGONAL_ELEMENT_KERNEL), ("diagonal_node", DIAGONAL_NODE_KERNEL)):
            r[name] = kernel_resources(self._code.log, kernel)
        r["waves"], r["slab"] = self._code.waves, self._code.slab
        return r

    @property
    def compile_log(self) -> str:
        return self._code.log

    def lds_bytes(self) -> int:
        """LDS of one block of either element kernel"""
        return lds_bytes(self.gdim, self.nodes_per_cell, self.points_per_cell)

    @property
    def device(self) -> int:
        return self.op.device

    # ---- constraints (set_constrained, _mask_table: ConstraintMask; the refusal is the one of ``TangentMatrix``) ------------------
    _no_own_block = "belongs to no cell: it has no diagonal block to make the identity's"

    def _without_own_block(self, nodes):
        return self.valence[nodes] == 0

    _check = staticmethod(check_tensor)  # (name, a, numel, dev): the solvers call K._check

    # ---- the product -----------------------------------------------------------------------------------------------------------
    def _apply(self, dev: int, tangent_ptr: int, v_ptr: int, out_ptr: int, mode: int, partials_ptr: int = 0, control_ptr: int = 0) -> None:
        """both launches of ``out = A v`` on pointers that have been validated (the solver's seam); ``mode``: ``MODE_QUIET`` -- the
        product alone --, ``MODE_PLAIN`` -- the ordered ``v . out`` into the control block's ``dot`` --, ``MODE_ITERATE`` -- into ``pq``, under
        the status"""
        for code, kernel, blocks, args, what in self._launches(dev, tangent_ptr, v_ptr, out_ptr, mode, partials_ptr, control_ptr):
            jit.launch(code, dev, blocks, args, what, kernel=kernel)

    def _launches(self, dev: int, tangent_ptr: int, v_ptr: int, out_ptr: int, mode: int, partials_ptr: int = 0, control_ptr: int = 0) -> list:
        """the launches of ``_apply`` as ``[(code, kernel, blocks, args, what)]``, for a caller that keeps them (the launch plan of the
        multilevel preconditioner): they hold the pointers given here, those of ``force``'s tables and element forces and the mask's"""
        force, op = self.force, self.op
        nd = self.shape[0]
        _, node_ptr, adj = force._tables(dev)
        mask = self._mask_table(dev)
        mask_ptr = 0 if mask is None else mask.data_ptr()
        cap = launch_cap(dev)
        fe_ptr = 0
        ops = []
        if self.n_cells:
            dofmap, ref, jinv, _ = op._tables(dev)
            weights = force._tables(dev)[0]
            fe = force._fe.get(dev)
            fe_ptr = (fe if fe is not None else force._element_forces(dev)).data_ptr()
            tiles = -(-self.n_cells // cells_per_tile(self.gdim, self.points_per_cell))
            ea = ElementArgs(tangent_ptr, v_ptr, dofmap.data_ptr(), mask_ptr, ref.data_ptr(), jinv.data_ptr(), weights.data_ptr(), fe_ptr,
                             control_ptr, self.n_cells, mode, 0)
            ops.append((self._code, None, tile_blocks(tiles, cap), ea, "TangentOperator element launch"))
        nseg = -(-nd // SEG)
        na = NodeArgs(fe_ptr, node_ptr.data_ptr(), adj.data_ptr(), v_ptr, mask_ptr, out_ptr, partials_ptr, control_ptr, nd, nseg, mode, 0)
        ops.append((self._code, NODE_KERNEL, max(1, min(nseg, cap)), na, "TangentOperator node launch"))  # a block per segment
        return ops

    def __call__(self, tangent, v, out=None):
        """``y = M K M v + (I - M) v`` for this tangent (asynchronous, on torch's current stream)"""
        import torch

        dev = self.device
        nd = self.shape[0]
        self._check("tangent", tangent, self.tangent_dim * self.n_points, dev)
        self._check("v", v, nd, dev)
        if out is not None:
            self._check("out", out, nd, dev)
            if overlap(out, v):
                raise ValueError("out must not alias v")
        with torch.cuda.device(dev):
            if out is None:
                out = torch.empty(nd, dtype=torch.float64, device=torch.device("cuda", dev))
            self._apply(dev, tangent.data_ptr(), v.data_ptr(), out.data_ptr(), MODE_QUIET)
        return out

    # ---- the diagonal blocks ---------------------------------------------------------------------------------------------------
    def chunks(self):
        """the ascending cell ranges ``(first, end)`` ``diagonal_blocks`` runs one after the other"""
        return self._pass.chunks()

    def diagonal_blocks(self, tangent, out=None):
        """device tensor ``[n_nodes][D][D]``: every node's own block of the constrained ``K`` (zeros at a node of no cell) --
        ``out`` or a new one (asynchronous, on torch's current stream)"""
        import torch

        dev = self.device
        d_, a_ = self.gdim, self.nodes_per_cell
        dd = d_ * d_
        self._check("tangent", tangent, self.tangent_dim * self.n_points, dev)
        if out is not None:
            self._check("out", out, dd * self.n_nodes, dev)
        with torch.cuda.device(dev):
            if out is None:
                out = torch.empty((self.n_nodes, d_, d_), dtype=torch.float64, device=torch.device("cuda", dev))
            _, node_ptr, adj = self.force._tables(dev)
            mask = self._mask_table(dev)
            cap = launch_cap(dev)
            na = DiagNodeArgs(0, node_ptr.data_ptr(), adj.data_ptr(), 0 if mask is None else mask.data_ptr(), out.data_ptr(), dd * self.n_nodes,
                              0, 0, 1, 0)
            node_blocks = max(1, blocks_for(dd * self.n_nodes, cap))  # a lane per entry
            if self.n_cells == 0:  # no contributions: the entries are started and left
                jit.launch(self._code, dev, node_blocks, na, "TangentOperator diagonal node launch", kernel=DIAGONAL_NODE_KERNEL)
                return out
            ref = self.op._tables(dev)[1].data_ptr()
            de = na.de = self._pass.buffer(self._scratch, dev).data_ptr()
            for k, c0, c1, tangent_ptr, jinv_ptr, weights_ptr, element_blocks in self._pass.walk(dev, tangent, cap):
                ea = DiagElementArgs(tangent_ptr, ref, jinv_ptr, weights_ptr, de, c1 - c0)
                jit.launch(self._code, dev, element_blocks, ea, "TangentOperator diagonal element launch", kernel=DIAGONAL_ELEMENT_KERNEL)
                na.key_lo, na.key_hi, na.first = c0 * a_, c1 * a_, 1 if k == 0 else 0
                jit.launch(self._code, dev, node_blocks, na, "TangentOperator diagonal node launch", kernel=DIAGONAL_NODE_KERNEL)
        return out
