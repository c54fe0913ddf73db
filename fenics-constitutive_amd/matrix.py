"""The assembled tangent stiffness on the GPU: ``K = sum_p B_p^T C_p B_p w_p`` as the values of a sparse matrix.

``InternalForce.tangent_action`` applies the tangent stiffness without forming it; a direct solver, an algebraic-multigrid or
incomplete-factorisation preconditioner and block-Jacobi need the matrix itself.  ``TangentMatrix(force)`` builds the sparsity
pattern of the mesh once on the host (block CSR over the nodes, ``D x D`` blocks) and fills its values on the device from the
tangent that already sits in HBM; only the values array (or nothing, with a solver on the device) leaves it.

Two run-time compiled kernels (``csrc/jit/tangent_matrix.hip``, through ``jit.compile_program`` / ``jit.launch``): the element
kernel writes the dense ``(A D) x (A D)`` matrix of every cell into a scratch buffer, the gather kernel adds, for every entry of
the pattern, the contributions of its block in a fixed order -- no floating-point atomics, the same bits in every run.  Column
``(b, s)`` of a cell's matrix is the element force of the unit displacement of local node ``b`` in direction ``s``; with
``-ffp-contract=off`` the arithmetic is exactly (``H`` the double of ``sqrt(0.5)``; the functions of ``force.py``'s docstring)::

    g[c][q][a][x] = 0.0;  g = g + ref[q][a][k] * jinv[c(,q)][k][x], k ascending
    for every (b, s):  G[r][x] = g[c][q][b][x] if r == s else 0.0
      e = (G00, G11, G22, H*(G01+G10), H*(G02+G20), H*(G12+G21));  sv[i] = 0.0;  sv[i] = sv[i] + C[c][q][i][j] * e[j]
      T[i][i] = sv[i];  T[i][j] = T[j][i] = sv[3 + m] * H
      ke[c][a][r][b][s] = 0.0;  for q ascending:  t = 0.0;  t = t + T[r][x] * g[c][q][a][x];  ke = ke + t * weights[c][q]
    values[(v, u)][r][s] = 0.0 (or out's value);  + ke[c][a][r][b][s] over the block's contributions, ascending c*A*A + a*A + b

The scratch is bounded (``scratch_bytes``): the cells are cut into ascending chunks, each runs the element kernel and a gather
that adds only its own contributions.  The contribution lists are ascending in ``c``, so the result is the same bits for every
chunk size.  LDS of a block of the element kernel: ``lds_bytes``; the same ``LDS_CAP`` as the other operators.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import jit
from ._fe_common import SCRATCH_BYTES  # noqa: F401  (the default of scratch_bytes: read from here)
from ._fe_common import (ChunkedPass, ConstraintMask, blocks_for, check_tensor, compile_ladder, even, kernel_resources, launch_cap, per_device, upload,
                         vector_registers)
from .device import _is_torch
from .force import MANDEL_DIM, VGPRS_PER_SIMD, InternalForce
from .gradient import LDS_CAP

ELEMENT_KERNEL = "fcamd_tangent_matrix_element_kernel"
GATHER_KERNEL = "fcamd_tangent_matrix_gather_kernel"
FORMATS = ("bsr", "csr")
#: points of a tile whose inputs sit in a wave's LDS region at a time: the first that fits ``LDS_CAP``
SLABS = (16, 8, 4, 2, 1)

__all__ = ["TangentMatrix", "block_pattern", "cells_per_tile", "compile_kernels", "contribution_lists", "lds_bytes", "program", "slab_points"]


def cells_per_tile(gdim: int, nodes_per_cell: int) -> int:
    """CW: the whole cells one wave of the element kernel takes, ``64 // (A*D)`` (a lane per column), at least one"""
    return max(1, 64 // (gdim * nodes_per_cell))


def lds_bytes(gdim: int, nodes_per_cell: int, points_per_cell: int, affine: bool, slab: int) -> int:
    """LDS of one block of the element kernel: the reference table and four wave regions, each the tangent rows, the per-point
    inverse Jacobians, the basis gradients and the weights of ``slab`` points (every part padded to 16 bytes)"""
    s = MANDEL_DIM[gdim]
    region = even(slab * s * s) + (0 if affine else even(slab * gdim * gdim)) + even(slab * gdim * nodes_per_cell) + even(slab)
    return 8 * (even(gdim * nodes_per_cell * points_per_cell) + 4 * region)


def slab_points(gdim: int, nodes_per_cell: int, points_per_cell: int, affine: bool) -> int:
    """the first of ``SLABS`` whose block fits ``LDS_CAP`` (``ValueError`` where none does)"""
    for slab in SLABS:
        if lds_bytes(gdim, nodes_per_cell, points_per_cell, affine, slab) <= LDS_CAP:
            return slab
    need = lds_bytes(gdim, nodes_per_cell, points_per_cell, affine, SLABS[-1])
    raise ValueError(f"the tables of {points_per_cell} points x {nodes_per_cell} nodes x {gdim} need {need} bytes of LDS per block; at most {LDS_CAP} fit")


def program(gdim: int, nodes_per_cell: int, points_per_cell: int, affine: bool, slab: int, waves: int) -> str:
    """the program text of one shape (the compile cache is keyed by it)"""
    lines = [f"#define FCAMD_TM_D {int(gdim)}", f"#define FCAMD_TM_A {int(nodes_per_cell)}", f"#define FCAMD_TM_Q {int(points_per_cell)}",
             f"#define FCAMD_TM_AFFINE {1 if affine else 0}", f"#define FCAMD_TM_SLAB {int(slab)}", f"#define FCAMD_TM_WAVES {int(waves)}",
             '#include "tangent_matrix.hip"']
    return "\n".join(lines) + "\n"


def compile_kernels(gdim: int, nodes_per_cell: int, points_per_cell: int, affine: bool, waves: int | None = None):
    """The code object of one shape, both kernels in it (no GPU needed).  ``waves``: that register budget of the element kernel;
    ``None``: the first of ``WAVES_LADDER`` without scratch whose registers allow that many waves.  A shape that spills at every
    budget, or whose tables do not fit the LDS, is a ``ValueError``.  ``code.waves`` is the budget kept, ``code.slab`` the slab."""
    if gdim not in (1, 2, 3):
        raise ValueError(f"the geometric dimension must be 1, 2 or 3, got {gdim}")
    if nodes_per_cell < 1 or points_per_cell < 1:
        raise ValueError("a cell needs at least one node and one quadrature point")
    slab = slab_points(gdim, nodes_per_cell, points_per_cell, affine)
    name = f"tangent_matrix_{gdim}d_{nodes_per_cell}n_{points_per_cell}q"
    # __launch_bounds__ is a hint: a budget the compiler overran is not the one the kernel runs at
    return compile_ladder(lambda w: program(gdim, nodes_per_cell, points_per_cell, affine, slab, w), name, ELEMENT_KERNEL, waves,
                          (ELEMENT_KERNEL, GATHER_KERNEL), slab=slab,
                          accept=lambda log, w: vector_registers(log, ELEMENT_KERNEL) <= VGPRS_PER_SIMD // w,
                          exhausted=lambda s: ValueError(f"{name}: the element matrix of {gdim * nodes_per_cell} columns does not compile without scratch at "
                                                         f"any register budget (last: {s} bytes per lane)"))


def block_pattern(dofmap: np.ndarray, n_nodes: int):
    """Block CSR of the node pairs that share a cell: ``(indptr[n_nodes + 1], indices[nnzb])`` (int32), block row ``v`` the
    ascending, unique nodes ``u`` with ``v`` and ``u`` in one cell"""
    dofmap = np.ascontiguousarray(dofmap)
    a_ = dofmap.shape[1] if dofmap.ndim == 2 else 0
    if dofmap.size * a_ >= 2**31 or int(n_nodes) >= 2**31:
        raise ValueError(f"{dofmap.shape[0]} cells x {a_} x {a_} node pairs do not fit the 32-bit pattern")
    d64 = dofmap.astype(np.int64)
    key = np.unique((d64[:, :, None] * n_nodes + d64[:, None, :]).reshape(-1))
    indptr = np.zeros(n_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n_nodes, minlength=n_nodes), out=indptr[1:])
    return indptr.astype(np.int32), (key % n_nodes).astype(np.int32)


def contribution_lists(dofmap: np.ndarray, n_nodes: int, indptr: np.ndarray, indices: np.ndarray):
    """``(blk_ptr[nnzb + 1], contrib)`` (int32): the contributions ``c*A*A + a*A + b`` with ``dofmap[c][a] == v`` and
    ``dofmap[c][b] == u`` of block ``k = (v, u)`` at ``contrib[blk_ptr[k]: blk_ptr[k + 1]]``, ascending.  A cell pair that is not
    in the pattern is a ``ValueError``"""
    dofmap = np.ascontiguousarray(dofmap)
    n_cells, a_ = dofmap.shape
    if n_cells * a_ * a_ >= 2**31:
        raise ValueError(f"{n_cells} cells x {a_} x {a_} contributions do not fit the 32-bit lists")
    nnzb = indices.size
    d64 = dofmap.astype(np.int64)
    key = (d64[:, :, None] * n_nodes + d64[:, None, :]).reshape(-1)
    order = np.argsort(key, kind="stable")  # stable: ascending c*A*A + a*A + b within a block
    rows = np.repeat(np.arange(n_nodes, dtype=np.int64), np.diff(indptr.astype(np.int64)))
    pattern = rows * n_nodes + indices.astype(np.int64)  # ascending
    block = np.searchsorted(pattern, key[order])
    if key.size and (nnzb == 0 or (pattern[np.minimum(block, nnzb - 1)] != key[order]).any()):
        raise ValueError("a node pair of the operator's cells is missing from the pattern of pattern_dofmap")
    blk_ptr = np.zeros(nnzb + 1, dtype=np.int64)
    np.cumsum(np.bincount(block, minlength=nnzb), out=blk_ptr[1:])
    return blk_ptr.astype(np.int32), order.astype(np.int32)


class ElementArgs(C.Structure):
    """ctypes mirror of ElementArgs (tangent_matrix.hip)"""

    _fields_ = [("tangent", C.c_void_p), ("ref", C.c_void_p), ("jinv", C.c_void_p), ("weights", C.c_void_p), ("ke", C.c_void_p),
                ("n_cells", C.c_int64)]


class GatherArgs(C.Structure):
    """ctypes mirror of GatherArgs (tangent_matrix.hip)"""

    _fields_ = [("ke", C.c_void_p), ("blk_ptr", C.c_void_p), ("contrib", C.c_void_p), ("dest_base", C.c_void_p), ("dest_stride", C.c_void_p),
                ("block_row", C.c_void_p), ("block_col", C.c_void_p), ("mask", C.c_void_p), ("values", C.c_void_p), ("entry0", C.c_int64), ("n_entries", C.c_int64),
                ("key_lo", C.c_int64), ("key_hi", C.c_int64), ("cell0", C.c_int64), ("first", C.c_int32), ("accumulate", C.c_int32)]


class TangentMatrix(ConstraintMask):
    """``K(tangent) -> values``: the tangent stiffness of the mesh of an ``InternalForce`` as a sparse matrix on the GPU.

    ``force``: the ``InternalForce`` whose operator (dofmap, reference gradients, inverse Jacobians, device) and weights are
    used; their device tables are shared, nothing is uploaded twice.  ``format``: "bsr" -- ``values[nnzb][D][D]``, block ``k`` of
    the pattern ``indptr`` / ``indices`` (int32, nodes), ``values[k][r][s] = K[D v + r][D u + s]`` -- or "csr", the scalar CSR of
    the same matrix (``csr_indptr`` / ``csr_indices``, columns ascending in every row; both formats have them).
    ``pattern_dofmap`` (int32 ``[cells][A']``): the pattern is that of this (global) dofmap, the contributions still those of
    ``force``'s cells; blocks the operator does not touch become ``+0.0`` or keep ``out``'s value under ``accumulate=True``, so
    the laws of several submeshes add into one matrix in a fixed order.  ``scratch_bytes``: the most element matrices may take
    between the kernels (default ``SCRATCH_BYTES``; at least one tile of ``cells_per_tile`` cells); the result does not depend
    on it.

    ``tangent`` is a float64 device tensor of ``S*S * n_points``; the result is ``out`` or a new float64 device tensor of ``nnz``
    = ``D*D * nnzb`` entries.  ``accumulate=True`` (needs ``out``) starts every entry from ``out``'s value.
    ``set_constrained(mask)`` (bool ``[D n_nodes]``) makes every entry whose row or column dof is constrained the constant ``1.0``
    on the diagonal and ``+0.0`` elsewhere, never read from the element matrices and never added to.

    Everything is validated on the host before anything is uploaded or launched (``TypeError`` / ``ValueError`` as for
    ``InternalForce``).  The kernels are compiled at construction (no GPU needed).  The scratch buffer belongs to the object, one
    per device, and all launches go to torch's current stream: use an object from one stream at a time."""

    def __init__(self, force: InternalForce, format: str = "bsr", pattern_dofmap=None, scratch_bytes: int | None = None):
        if not isinstance(force, InternalForce):
            raise TypeError(f"force must be an InternalForce, got {type(force).__name__}")
        if format not in FORMATS:
            raise ValueError(f"format must be one of {FORMATS}, got {format!r}")
        op = force.op
        d_, a_, q_ = op.gdim, op.nodes_per_cell, op.points_per_cell
        n_nodes = op.n_nodes
        if pattern_dofmap is not None:
            if not isinstance(pattern_dofmap, np.ndarray):
                raise TypeError(f"pattern_dofmap must be a numpy.ndarray, got {type(pattern_dofmap).__name__}")
            if pattern_dofmap.dtype != np.int32:
                raise TypeError(f"pattern_dofmap must be int32, got {pattern_dofmap.dtype}")
            if pattern_dofmap.ndim != 2:
                raise ValueError(f"pattern_dofmap must be [cells][nodes per cell], got shape {pattern_dofmap.shape}")
            if pattern_dofmap.size and (int(pattern_dofmap.min()) < 0 or int(pattern_dofmap.max()) >= n_nodes):
                raise ValueError(f"pattern_dofmap entries must lie in [0, {n_nodes})")
        m = a_ * d_
        cw = cells_per_tile(d_, a_)
        self._pass = ChunkedPass(force, scratch_bytes, m * m * 8, cw, lambda have, tile: f"scratch_bytes = {have} does not hold one tile of {cw} element "
                                 f"matrices of {m} x {m} doubles ({tile} bytes)")
        self.force, self.op, self.format = force, op, format
        self.gdim, self.nodes_per_cell, self.points_per_cell = d_, a_, q_
        self.n_cells, self.n_points, self.n_nodes = op.n_cells, op.n_points, n_nodes
        self.tangent_dim = MANDEL_DIM[d_] ** 2
        self._code = compile_kernels(d_, a_, q_, op.affine)  # (raises the ValueError of the LDS cap and of the registers)
        self.cells_per_tile = cw
        self.scratch_bytes, self.chunk_cells = self._pass.scratch_bytes, self._pass.chunk_cells
        # the symbolic phase
        self.indptr, self.indices = block_pattern(op._dofmap if pattern_dofmap is None else pattern_dofmap, n_nodes)
        self.nnzb = int(self.indices.size)
        dd = d_ * d_
        if self.nnzb * dd >= 2**31:
            raise ValueError(f"{self.nnzb} blocks of {d_} x {d_} do not fit the 32-bit scalar pattern")
        self.nnz = self.nnzb * dd
        self.shape = (d_ * n_nodes, d_ * n_nodes)
        self.blk_ptr, self.contributions = contribution_lists(op._dofmap, n_nodes, self.indptr, self.indices)
        per_row = np.diff(self.indptr.astype(np.int64))  # blocks of a block row
        self.block_row = np.repeat(np.arange(n_nodes, dtype=np.int32), per_row)
        self.csr_indptr = np.zeros(d_ * n_nodes + 1, dtype=np.int64)
        np.cumsum(np.repeat(d_ * per_row, d_), out=self.csr_indptr[1:])
        rank = np.arange(self.nnzb, dtype=np.int64) - self.indptr[:-1].astype(np.int64)[self.block_row]
        csr_base = self.csr_indptr[d_ * self.block_row.astype(np.int64)] + d_ * rank
        csr_stride = (d_ * per_row)[self.block_row]
        pos = csr_base[:, None, None] + csr_stride[:, None, None] * np.arange(d_)[None, :, None] + np.arange(d_)[None, None, :]
        self.csr_indices = np.empty(self.nnz, dtype=np.int32)
        self.csr_indices[pos.reshape(-1)] = np.broadcast_to((d_ * self.indices.astype(np.int64))[:, None, None] + np.arange(d_)[None, None, :],
                                                            pos.shape).reshape(-1)
        self.csr_indptr = self.csr_indptr.astype(np.int32)
        if format == "bsr":
            self.dest_base = dd * np.arange(self.nnzb, dtype=np.int64)
            self.dest_stride = np.full(self.nnzb, d_, dtype=np.int32)
        else:
            self.dest_base, self.dest_stride = csr_base, csr_stride.astype(np.int32)
        # the range of blocks every chunk's cells touch: a later chunk's gather runs over it alone
        self.chunk_blocks = self._pass.block_ranges(self.contributions, self.blk_ptr, self.nnzb, a_ * a_)
        # the node's own block (-1: none)
        self.diag_block = np.full(n_nodes, -1, dtype=np.int64)
        on_diagonal = np.flatnonzero(self.indices == self.block_row)
        self.diag_block[self.block_row[on_diagonal]] = on_diagonal
        self._on = {}  # device index -> the pattern tables
        self._scratch = {}  # device index -> element matrices of a chunk
        self._mask_on = {}  # device index -> (version, mask tensor)
        self._diag_on = {}  # device index -> (positions, present)

    # ---- what the compiler made ------------------------------------------------------------------------------------------------
    @property
    def resources(self) -> dict:
        """``{"vgprs", "sgprs", "scratch_bytes", "lds_bytes", "waves_per_simd", ...}`` of the element kernel, under "gather" those
        of the gather kernel (compiler remarks), under "waves" the register budget kept and under "slab" the points per slab"""
        r = kernel_resources(self._code.log, ELEMENT_KERNEL)
        r["gather"] = kernel_resources(self._code.log, GATHER_KERNEL)
        r["waves"], r["slab"] = self._code.waves, self._code.slab
        return r

    @property
    def compile_log(self) -> str:
        return self._code.log

    def lds_bytes(self) -> int:
        """LDS of one block of the element kernel"""
        return lds_bytes(self.gdim, self.nodes_per_cell, self.points_per_cell, self.op.affine, self._code.slab)

    @property
    def device(self) -> int:
        return self.op.device

    # ---- constraints (set_constrained, _mask_table: ConstraintMask) ---------------------------------------------------------------
    _no_own_block = "no diagonal block in the pattern: its row cannot be made the identity's"

    def _without_own_block(self, nodes):
        return self.diag_block[nodes] < 0

    # ---- device tables ---------------------------------------------------------------------------------------------------------
    def _tables(self, dev: int):
        t = self._on.get(dev)  # (the hit stays inline: this is on the path of every call)
        return t if t is not None else per_device(self._on, dev, lambda d: upload(d, self.blk_ptr, self.contributions, self.dest_base, self.dest_stride, self.block_row,
                                                          self.indices))

    _check = staticmethod(check_tensor)  # (name, a, numel, dev): the solvers call K._check

    def chunks(self):
        """the ascending cell ranges ``(first, end)`` a call runs one after the other"""
        return self._pass.chunks()

    def __call__(self, tangent, out=None, accumulate: bool = False):
        """the values of ``K`` for this tangent (asynchronous, on torch's current stream)"""
        import torch

        if accumulate and out is None:
            raise ValueError("accumulate=True needs out: the values the sums start from")
        dev = self.device
        self._check("tangent", tangent, self.tangent_dim * self.n_points, dev)
        if out is not None:
            self._check("out", out, self.nnz, dev)
        d_, a_ = self.gdim, self.nodes_per_cell
        with torch.cuda.device(dev):
            if out is None:
                out = torch.empty((self.nnzb, d_, d_) if self.format == "bsr" else (self.nnz,), dtype=torch.float64, device=torch.device("cuda", dev))
            if self.nnz == 0:
                return out
            blk_ptr, contrib, dest_base, dest_stride, block_row, block_col = self._tables(dev)
            mask = self._mask_table(dev)
            cap = launch_cap(dev)
            gather_blocks = blocks_for(self.nnz, cap)  # a lane per entry
            ga = GatherArgs(0, blk_ptr.data_ptr(), contrib.data_ptr(), dest_base.data_ptr(), dest_stride.data_ptr(), block_row.data_ptr(),
                            block_col.data_ptr(), 0 if mask is None else mask.data_ptr(), out.data_ptr(), 0, self.nnz, 0, 0, 0, 1,
                            1 if accumulate else 0)
            if self.n_cells == 0:  # no contributions: the entries are started (zeros, out's values, the constrained constants) and left
                jit.launch(self._code, dev, gather_blocks, ga, "TangentMatrix gather launch", kernel=GATHER_KERNEL)
                return out
            ref = self.op._tables(dev)[1].data_ptr()
            ke = ga.ke = self._pass.buffer(self._scratch, dev).data_ptr()
            for k, c0, c1, tangent_ptr, jinv_ptr, weights_ptr, element_blocks in self._pass.walk(dev, tangent, cap):
                ea = ElementArgs(tangent_ptr, ref, jinv_ptr, weights_ptr, ke, c1 - c0)
                jit.launch(self._code, dev, element_blocks, ea, "TangentMatrix element launch")
                ga.key_lo, ga.key_hi, ga.cell0, ga.first = c0 * a_ * a_, c1 * a_ * a_, c0, 1 if k == 0 else 0
                if k:  # the first chunk starts every entry; a later one visits the blocks its cells touch
                    ga.entry0, ga.n_entries = d_ * d_ * self.chunk_blocks[k][0], d_ * d_ * self.chunk_blocks[k][1]
                    gather_blocks = blocks_for(ga.n_entries - ga.entry0, cap)
                jit.launch(self._code, dev, gather_blocks, ga, "TangentMatrix gather launch", kernel=GATHER_KERNEL)
        return out

    # ---- small helpers ---------------------------------------------------------------------------------------------------------
    def to_scipy(self, values):
        """``scipy.sparse.bsr_matrix`` ("bsr") or ``csr_matrix`` ("csr") of a values array (device tensor: downloaded; ndarray)"""
        import scipy.sparse as sp

        if _is_torch(values):
            from .hostio import to_host

            values = to_host(values) if values.is_cuda else values.numpy()
        values = np.asarray(values, dtype=np.float64)
        if values.size != self.nnz:
            raise ValueError(f"values has {values.size} entries, the pattern {self.nnz}")
        if self.format == "bsr":
            return sp.bsr_matrix((values.reshape(self.nnzb, self.gdim, self.gdim), self.indices, self.indptr), shape=self.shape)
        return sp.csr_matrix((values.reshape(-1), self.csr_indices, self.csr_indptr), shape=self.shape)

    def diagonal_blocks(self, values):
        """device tensor ``[n_nodes][D][D]``: every node's own block of ``values`` (zeros where the pattern has none): the inverse
        of these is the block-Jacobi preconditioner of the matrix-free loop"""
        import torch

        dev = self.device
        self._check("values", values, self.nnz, dev)
        d_ = self.gdim

        def positions(d):
            k = np.maximum(self.diag_block, 0)
            base = self.dest_base[k] if self.nnzb else np.zeros(self.n_nodes, dtype=np.int64)
            stride = self.dest_stride[k].astype(np.int64) if self.nnzb else np.zeros(self.n_nodes, dtype=np.int64)
            pos = base[:, None, None] + stride[:, None, None] * np.arange(d_)[None, :, None] + np.arange(d_)[None, None, :]
            present = np.broadcast_to((self.diag_block >= 0)[:, None, None], pos.shape)
            return upload(d, np.where(present, pos, 0), present.copy())

        pos, present = per_device(self._diag_on, dev, positions)
        with torch.cuda.device(dev):
            if self.nnz == 0:
                return torch.zeros((self.n_nodes, d_, d_), dtype=torch.float64, device=torch.device("cuda", dev))
            picked = values.reshape(-1)[pos]
            return torch.where(present, picked, torch.zeros((), dtype=torch.float64, device=picked.device))
