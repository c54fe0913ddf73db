"""The transpose of the gradient producer: nodal internal forces and tangent actions on the GPU.

What an assembler does with the stress and the tangent of the quadrature points is the transpose of the operator
``DisplacementGradient`` already holds on the device::

    f = sum_p B_p^T sigma_p w_p                 InternalForce.__call__        (the residual)
    y = sum_p B_p^T C_p B_p v w_p               InternalForce.tangent_action  (the Jacobian action of a Newton-Krylov loop)

``InternalForce(op, weights)`` takes the dofmap, the reference gradients, the inverse Jacobians, the device and the gradient
layout from ``op`` and shares its device tables; only ``weights[C][Q] = w_q |det J|(c, q)`` (``gradient.integration_weights``)
and the node -> (cell, local node) adjacency are new.  The loop of a Newton iteration becomes ``du -> op -> law -> force`` with
nodal vectors on the link and stress and tangent staying in HBM.

Two run-time compiled kernels (``csrc/jit/internal_force.hip``, through ``jit.compile_program`` / ``jit.launch``): the element
kernel writes ``fe[C][A][D]``, the node kernel adds the entries of every node in a fixed order -- no floating-point atomics, so the
result is the same bits in every run.  With ``-ffp-contract=off`` the arithmetic is exactly (``H`` the double of ``sqrt(0.5)``,
``0x3FE6A09E667F3BCD``; stress in the Mandel order of ``interfaces.py``: 6, 4 or 1 components for D = 3, 2, 1)::

    T[i][i] = s[i];   T[i][j] = T[j][i] = s[3 + m] * H      for the m-th pair of (0,1), (0,2), (1,2)      (D = 2: (0,1) only)
    tangent_action, G[r][x] = d v_r / d x_x of the point:
      e = (G00, G11, G22, H*(G01+G10), H*(G02+G20), H*(G12+G21))      (D = 2: (G00, G11, 0.0, H*(G01+G10)); D = 1: (G00))
      s[i] = 0.0;  for j = 0..S-1:  s[i] = s[i] + tangent[p][i][j] * e[j]
    fe[c][a][r] = 0.0
    for q = 0..Q-1:            p = Q*c + q
      g[x] = 0.0;  for k = 0..D-1:  g[x] = g[x] + ref[q][a][k] * jinv[c(,q)][k][x]
      t    = 0.0;  for x = 0..D-1:  t    = t + T[r][x] * g[x]
      fe[c][a][r] = fe[c][a][r] + t * weights[c][q]
    f[D*v + r] = 0.0 (or out's value);  for the entries (c, a) of node v, ascending c*A + a:  f = f + fe[c][a][r]

LDS of a block (``lds_bytes``): that of the producer -- the reference table and four regions of ``64 * D*D`` doubles, which serve
the transpositions, the tangent slabs and the per-cell sums alike; the same ``LDS_CAP``.  ``Q`` may be at most 64: a wave takes
whole cells.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import gradient, jit
from ._fe_common import BLOCKS_PER_CU, check_tensor, compile_ladder, doubles, kernel_resources, per_device, upload
from .gradient import LDS_CAP, DisplacementGradient, lds_bytes

ELEMENT_KERNEL = "fcamd_internal_force_element_kernel"
NODE_KERNEL = "fcamd_internal_force_node_kernel"
SOURCES = ("stress", "tangent")
#: the most quadrature points a cell may have: a wave of 64 lanes takes whole cells
MAX_POINTS_PER_CELL = 64
MANDEL_DIM = {1: 1, 2: 4, 3: 6}
#: vector registers of a SIMD per lane: a kernel with v of them runs at most 512 // v waves there
VGPRS_PER_SIMD = 512

__all__ = ["InternalForce", "cells_per_tile", "compile_kernels", "kernel_resources", "lds_bytes", "node_adjacency", "program"]


def cells_per_tile(gdim: int, points_per_cell: int) -> int:
    """W: the whole cells one wave takes, ``64 // Q``, one less where ``W * Q * D*D`` would be odd (every tile base of stress,
    ``jinv`` and gradient then stays on the 16-byte grid)"""
    w = 64 // points_per_cell
    return w - 1 if w > 1 and (w * points_per_cell * gdim * gdim) % 2 else w


def program(gdim: int, nodes_per_cell: int, points_per_cell: int, affine: bool, layout: str, source: str, accumulate: bool, waves: int) -> str:
    """the program text of one shape (the compile cache is keyed by it)"""
    if layout not in gradient.LAYOUTS:
        raise ValueError(f"layout must be one of {gradient.LAYOUTS}, got {layout!r}")
    if source not in SOURCES:
        raise ValueError(f"source must be one of {SOURCES}, got {source!r}")
    lines = [f"#define FCAMD_IF_D {int(gdim)}", f"#define FCAMD_IF_A {int(nodes_per_cell)}", f"#define FCAMD_IF_Q {int(points_per_cell)}",
             f"#define FCAMD_IF_AFFINE {1 if affine else 0}", f"#define FCAMD_IF_NABLA {1 if layout == 'nabla_grad' else 0}",
             f"#define FCAMD_IF_SOURCE {SOURCES.index(source)}", f"#define FCAMD_IF_ACCUMULATE {1 if accumulate else 0}",
             f"#define FCAMD_IF_WAVES {int(waves)}", '#include "internal_force.hip"']
    return "\n".join(lines) + "\n"


def compile_without_scratch(text: str, name: str, entry: str, kernels):
    """``jit.compile_program(text, name, entry)``; one of ``kernels`` with scratch is a ``ValueError`` that names it"""
    code = jit.compile_program(text, name, entry)
    for kernel in kernels:
        scratch = kernel_resources(code.log, kernel)["scratch_bytes"]
        if scratch:
            raise ValueError(f"{name}: {kernel} compiles with {scratch} bytes of scratch per lane")
    return code


def compile_kernels(gdim: int, nodes_per_cell: int, points_per_cell: int, affine: bool, layout: str = "nabla_grad", source: str = "stress",
                    accumulate: bool = False, waves: int | None = None):
    """The code object of one shape, both kernels in it (no GPU needed).  ``waves``: that register budget of the element kernel;
    ``None``: the first of ``WAVES_LADDER`` without scratch whose registers allow that many waves (a kernel that spills at every
    budget is an error).  ``code.waves`` is the budget kept."""
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
    name = f"internal_force_{gdim}d_{nodes_per_cell}n_{points_per_cell}q_{source}"
    # __launch_bounds__ is a hint: the compiler may take more registers than the budget allows waves for (cells with many points
    # do); such a budget is not the one the kernel runs at.  Where every budget is overrun, the first without scratch is kept.
    return compile_ladder(lambda w: program(gdim, nodes_per_cell, points_per_cell, affine, layout, source, accumulate, w), name, ELEMENT_KERNEL, waves,
                          (ELEMENT_KERNEL, NODE_KERNEL), keep_overrun=True,
                          accept=lambda log, w: kernel_resources(log, ELEMENT_KERNEL)["vgprs"] <= VGPRS_PER_SIMD // w,
                          exhausted=lambda s: RuntimeError(f"{name}: the kernels use {s} bytes of scratch per lane at every register budget"))


def node_adjacency(dofmap: np.ndarray, n_nodes: int):
    """CSR node -> (cell, local node): ``(node_ptr[n_nodes + 1], entries)`` (int32), the entries ``c*A + a`` of node ``v`` at
    ``entries[node_ptr[v]: node_ptr[v + 1]]`` in ascending order"""
    flat = np.ascontiguousarray(dofmap).reshape(-1)
    if flat.size >= 2**31:
        raise ValueError(f"{dofmap.shape[0]} cells x {dofmap.shape[1]} nodes do not fit the 32-bit adjacency")
    entries = np.argsort(flat, kind="stable").astype(np.int32)  # stable: ascending c*A + a within a node
    node_ptr = np.zeros(n_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=n_nodes), out=node_ptr[1:])
    return node_ptr.astype(np.int32), entries


class ElementArgs(C.Structure):
    """ctypes mirror of ElementArgs (internal_force.hip)"""

    _fields_ = [("src", C.c_void_p), ("grad", C.c_void_p), ("ref", C.c_void_p), ("jinv", C.c_void_p), ("weights", C.c_void_p),
                ("fe", C.c_void_p), ("n_cells", C.c_int64)]


class NodeArgs(C.Structure):
    """ctypes mirror of NodeArgs (internal_force.hip)"""

    _fields_ = [("fe", C.c_void_p), ("node_ptr", C.c_void_p), ("adj", C.c_void_p), ("out", C.c_void_p), ("n_dofs", C.c_int64)]


class InternalForce:
    """``force(stress) -> f`` and ``force.tangent_action(tangent, op(v)) -> y`` on the GPU for the mesh of a gradient operator.

    ``op``: a ``DisplacementGradient``; ``weights[C][Q]`` (float64): quadrature weight times ``|det J|`` of every point
    (``gradient.integration_weights``).  ``stress`` is a float64 device tensor of ``S * n_points`` (Mandel components, ``S`` = 6,
    4, 1 for ``D`` = 3, 2, 1; the ``zz`` entry of ``D = 2`` does no work in the plane and is not read), ``tangent`` one of
    ``S*S * n_points``, ``grad_v`` the operator's own output for a nodal vector ``v``.  The result is a float64 device tensor of
    ``D * n_nodes``, component ``r`` of node ``v`` at ``D*v + r``: ``out`` or a new one.  ``accumulate=True`` (needs ``out``)
    starts every node sum from ``out``'s value: the laws of several submeshes, each with operators built from ``dofmap[cells]``,
    add into one global vector in a fixed order.

    Everything is validated on the host before anything is uploaded or launched: types and dtypes (``TypeError``); the shape of
    ``weights`` and its finiteness, ``Q <= 64``, the LDS cap, tensors on another device, not contiguous, of the wrong length or off
    the 16-byte grid, ``accumulate`` without ``out`` (``ValueError``).  The kernels are compiled on first use of a form (no GPU
    needed: ``compile_log``, ``resources``); the stress form at construction.

    The element forces ``fe[C][A][D]`` between the two kernels live in ONE buffer per device that the operator owns, and both
    launches go to torch's current stream: use an operator from one stream at a time (two calls on different streams would race
    on ``fe``); calls on one stream are ordered and need nothing."""

    def __init__(self, op: DisplacementGradient, weights):
        if not isinstance(op, DisplacementGradient):
            raise TypeError(f"op must be a DisplacementGradient, got {type(op).__name__}")
        if not isinstance(weights, np.ndarray):
            raise TypeError(f"weights must be a numpy.ndarray, got {type(weights).__name__}")
        if weights.dtype != np.float64:
            raise TypeError(f"weights must be float64, got {weights.dtype}")
        if weights.shape != (op.n_cells, op.points_per_cell):
            raise ValueError(f"weights must have shape {(op.n_cells, op.points_per_cell)} (cells x points per cell), got {weights.shape}")
        if not np.isfinite(weights).all():
            raise ValueError("weights has non-finite entries")
        self.op = op
        self.gdim, self.nodes_per_cell, self.points_per_cell = op.gdim, op.nodes_per_cell, op.points_per_cell
        self.n_cells, self.n_points, self.n_nodes = op.n_cells, op.n_points, op.n_nodes
        self.stress_dim = MANDEL_DIM[self.gdim]
        self._codes = {}
        self._code("stress", False)  # (raises the ValueError of Q > 64 and of the LDS cap)
        self._weights = np.ascontiguousarray(weights)
        self.node_ptr, self.adjacency = node_adjacency(op._dofmap, self.n_nodes)
        self._on = {}  # device index -> (weights, node_ptr, adjacency)
        self._fe = {}  # device index -> fe[C][A][D]

    def _code(self, source: str, accumulate: bool):
        code = self._codes.get((source, accumulate))
        if code is None:
            op = self.op
            code = self._codes[source, accumulate] = compile_kernels(op.gdim, op.nodes_per_cell, op.points_per_cell, op.affine, op.layout,
                                                                     source, accumulate)
        return code

    @property
    def cells_per_tile(self) -> int:
        return cells_per_tile(self.gdim, self.points_per_cell)

    @property
    def resources(self) -> dict:
        """``{"vgprs", "sgprs", "scratch_bytes", "lds_bytes", "waves_per_simd", ...}`` of the element kernel in its stress form,
        under "tangent_action" those of its tangent form and under "node" those of the node kernel (compiler remarks)"""
        r = kernel_resources(self._code("stress", False).log, ELEMENT_KERNEL)
        r["tangent_action"] = kernel_resources(self._code("tangent", False).log, ELEMENT_KERNEL)
        r["node"] = kernel_resources(self._code("stress", False).log, NODE_KERNEL)
        return r

    @property
    def compile_log(self) -> str:
        return self._code("stress", False).log

    def lds_bytes(self) -> int:
        """LDS of one block of the element kernel"""
        return lds_bytes(self.gdim, self.nodes_per_cell, self.points_per_cell)

    @property
    def device(self) -> int:
        return self.op.device

    def _tables(self, dev: int):
        t = self._on.get(dev)  # (the hit stays inline: this is on the path of every call)
        return t if t is not None else per_device(self._on, dev, lambda d: upload(d, self._weights, self.node_ptr, self.adjacency))

    def _element_forces(self, dev: int):
        """``fe[C][A][D]`` on ``dev``, made at the first use: the one buffer between the element and the node kernel (a caller on the
        path of every call looks into ``_fe`` first; the operator's product uses the buffer too)"""
        return per_device(self._fe, dev, lambda d: doubles(self.n_cells * self.nodes_per_cell * self.gdim, d))

    _check = staticmethod(check_tensor)  # (name, a, numel, dev): the solvers call K._check

    def _run(self, source: str, src, grad, out, accumulate: bool):
        import torch

        if accumulate and out is None:
            raise ValueError("accumulate=True needs out: the vector the node sums start from")
        dev = self.device
        s, dd = self.stress_dim, self.gdim * self.gdim
        if source == "stress":
            self._check("stress", src, s * self.n_points, dev)
        else:
            self._check("tangent", src, s * s * self.n_points, dev)
            self._check("grad_v", grad, dd * self.n_points, dev)
        nd = self.gdim * self.n_nodes
        if out is not None:
            self._check("out", out, nd, dev)
        code = self._code(source, bool(accumulate))
        with torch.cuda.device(dev):
            if out is None:
                out = torch.empty(nd, dtype=torch.float64, device=torch.device("cuda", dev))
            if self.n_points == 0:
                return out if accumulate else out.zero_()
            op = self.op
            _, ref, jinv, _ = op._tables(dev)
            weights, node_ptr, adj = self._tables(dev)
            fe = self._fe.get(dev)
            if fe is None:
                fe = self._element_forces(dev)
            cap = BLOCKS_PER_CU * jit.num_cu(dev)
            tiles = -(-self.n_cells // self.cells_per_tile)
            ea = ElementArgs(src.data_ptr(), 0 if grad is None else grad.data_ptr(), ref.data_ptr(), jinv.data_ptr(), weights.data_ptr(),
                             fe.data_ptr(), self.n_cells)
            jit.launch(code, dev, min((tiles + 3) // 4, cap), ea, "InternalForce element launch")  # a wave per tile, 4 waves per block
            na = NodeArgs(fe.data_ptr(), node_ptr.data_ptr(), adj.data_ptr(), out.data_ptr(), nd)
            jit.launch(code, dev, min((nd + 255) // 256, cap), na, "InternalForce node launch", kernel=NODE_KERNEL)  # a lane per dof
        return out

    def __call__(self, stress, out=None, accumulate: bool = False):
        """``f = sum_p B_p^T sigma_p w_p`` (asynchronous, on torch's current stream)"""
        return self._run("stress", stress, None, out, accumulate)

    def tangent_action(self, tangent, grad_v, out=None, accumulate: bool = False):
        """``y = sum_p B_p^T C_p B_p v w_p`` with ``grad_v = op(v)``; ``s = C e`` is formed in registers, no stress array in between"""
        return self._run("tangent", tangent, grad_v, out, accumulate)
