"""The gradient producer: quadrature-point displacement gradients on the GPU from a nodal displacement increment.

In small strain on a fixed mesh the map from the nodal increment to ``grad_del_u`` is one linear operator that never changes:
a dofmap, the reference-element basis gradients at the quadrature points and the inverse Jacobians.  ``DisplacementGradient``
holds the three tables on the device and applies them with a run-time compiled HIP kernel (``csrc/jit/displacement_gradient.hip``,
through ``jit.compile_program`` / ``jit.launch`` like the user-law templates).  Its output is the array every law -- built-in or
user-defined -- already reads, so a host assembler sends ``D * n_nodes`` doubles up the link instead of ``D * D * n_points``
(trilinear hexahedra with 2x2x2 points: about 3 B per point instead of 72) and hands the device tensor to
``ResidentState.evaluate_into``.

Arithmetic of point ``p = Q*c + q`` (the kernels are compiled with ``-ffp-contract=off``; a NumPy loop in this order gives the
same bits)::

    R[r][k] = 0.0;  for a = 0..A-1:  R[r][k] = R[r][k] + du[D*dofmap[c][a] + r] * ref[q][a][k]
    G[r][x] = 0.0;  for k = 0..D-1:  G[r][x] = G[r][x] + R[r][k] * jinv[c(,q)][k][x]
    out[D*D*p + D*r + x] = G[r][x]      layout "grad"        (d u_r / d x_x)
    out[D*D*p + D*r + x] = G[x][r]      layout "nabla_grad"  (the default: include/fcamd.h, ufl.nabla_grad)

LDS of a block (``lds_bytes``): the reference table, ``8 * roundup(Q*A*D, 2)`` bytes, and the four waves' transposition regions,
``4 * 64 * D*D * 8`` bytes.  A shape whose block needs more than ``LDS_CAP`` = 64 KiB -- the most one block may declare, and at
most two fifths of a compute unit's 160 KiB, so at least two blocks always fit a CU -- is refused with ``ValueError``: for
``D = 3`` a table of more than 5888 doubles (``Q*A > 1962``).
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi, jit
from ._fe_common import BLOCKS_PER_CU, WAVES_LADDER, doubles, per_device, upload
from .device import _check_torch, _is_torch

KERNEL = "fcamd_displacement_gradient_kernel"
LAYOUTS = ("nabla_grad", "grad")
#: the most LDS one block may use (bytes): the static limit of a block; two such blocks fit a compute unit's 160 KiB
LDS_CAP = 64 * 1024
# (WAVES_LADDER, the register budgets tried in order, and BLOCKS_PER_CU, the cap of a grid, are _fe_common's; they are read from here)


def lds_bytes(gdim: int, nodes_per_cell: int, points_per_cell: int) -> int:
    """LDS of one block: the reference table (padded to 16 bytes) and four transposition regions of 64 x D*D doubles"""
    table = gdim * nodes_per_cell * points_per_cell
    return 8 * ((table + 1) // 2 * 2) + 4 * 64 * gdim * gdim * 8


def program(gdim: int, nodes_per_cell: int, points_per_cell: int, affine: bool, layout: str, waves: int) -> str:
    """the program text of one shape (the compile cache is keyed by it)"""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {LAYOUTS}, got {layout!r}")
    lines = [f"#define FCAMD_DG_D {int(gdim)}", f"#define FCAMD_DG_A {int(nodes_per_cell)}", f"#define FCAMD_DG_Q {int(points_per_cell)}",
             f"#define FCAMD_DG_AFFINE {1 if affine else 0}", f"#define FCAMD_DG_NABLA {1 if layout == 'nabla_grad' else 0}",
             f"#define FCAMD_DG_WAVES {int(waves)}", '#include "displacement_gradient.hip"']
    return "\n".join(lines) + "\n"


def compile_kernel(gdim: int, nodes_per_cell: int, points_per_cell: int, affine: bool, layout: str = "nabla_grad", waves: int | None = None):
    """The code object of one shape (no GPU needed).  ``waves``: that register budget; ``None``: the first of ``WAVES_LADDER``
    without scratch (a kernel that spills at every budget is an error)."""
    if gdim not in (1, 2, 3):
        raise ValueError(f"the geometric dimension must be 1, 2 or 3, got {gdim}")
    if nodes_per_cell < 1 or points_per_cell < 1:
        raise ValueError("a cell needs at least one node and one quadrature point")
    need = lds_bytes(gdim, nodes_per_cell, points_per_cell)
    if need > LDS_CAP:
        raise ValueError(f"the reference table of {points_per_cell} x {nodes_per_cell} x {gdim} doubles needs {need} bytes of LDS per block "
                         f"with the transposition regions; at most {LDS_CAP} fit")
    name = f"displacement_gradient_{gdim}d_{nodes_per_cell}n_{points_per_cell}q"
    if waves is not None:
        return jit.compile_program(program(gdim, nodes_per_cell, points_per_cell, affine, layout, waves), name, KERNEL)
    # (one kernel, no register test, no budget noted on the code object: the ladder of _fe_common.compile_ladder does not fit without flags)
    for w in WAVES_LADDER:
        code = jit.compile_program(program(gdim, nodes_per_cell, points_per_cell, affine, layout, w), name, KERNEL)
        if not code.resources.get("scratch_bytes"):
            return code
    raise RuntimeError(f"{name}: the kernel uses {code.resources['scratch_bytes']} bytes of scratch per lane at every register budget")


def inverse_jacobians(cell_coordinates, geometry_reference_gradients) -> np.ndarray:
    """``jinv[c][q][k][x] = d xi_k / d x_x`` of an isoparametric mesh (any cell type), in plain NumPy.

    ``cell_coordinates[C][G][D]``: the coordinates of the G geometry nodes of every cell; ``geometry_reference_gradients[Q][G][D]``:
    the reference gradients of the coordinate element at the quadrature points.  The Jacobian is ``J[c][q][x][k] = sum_g
    X[c][g][x] * dN[q][g][k]``.  Called with the tabulation at ONE point (an affine mesh) the result is ``[C][D][D]``."""
    x = np.asarray(cell_coordinates, dtype=np.float64)
    dn = np.asarray(geometry_reference_gradients, dtype=np.float64)
    if x.ndim != 3 or dn.ndim != 3 or x.shape[1] != dn.shape[1] or x.shape[2] != dn.shape[2]:
        raise ValueError(f"cell_coordinates [C][G][D] and geometry_reference_gradients [Q][G][D] do not match: {x.shape}, {dn.shape}")
    jac = np.einsum("cgx,qgk->cqxk", x, dn)
    inv = np.ascontiguousarray(np.linalg.inv(jac))  # [c][q][k][x]
    return inv[:, 0].copy() if dn.shape[0] == 1 else inv


def integration_weights(cell_coordinates, geometry_reference_gradients, reference_weights) -> np.ndarray:
    """``weights[c][q] = reference_weights[q] * |det J[c][q]|`` of an isoparametric mesh, in plain NumPy: what ``InternalForce``
    multiplies every point's contribution with.  ``cell_coordinates`` and ``geometry_reference_gradients`` as for
    ``inverse_jacobians()`` (tabulated at all Q points, or at one for an affine mesh); ``reference_weights[Q]``: the quadrature
    weights on the reference cell."""
    x = np.asarray(cell_coordinates, dtype=np.float64)
    dn = np.asarray(geometry_reference_gradients, dtype=np.float64)
    w = np.asarray(reference_weights, dtype=np.float64)
    if x.ndim != 3 or dn.ndim != 3 or x.shape[1] != dn.shape[1] or x.shape[2] != dn.shape[2]:
        raise ValueError(f"cell_coordinates [C][G][D] and geometry_reference_gradients [Q][G][D] do not match: {x.shape}, {dn.shape}")
    if w.ndim != 1 or dn.shape[0] not in (1, w.shape[0]):
        raise ValueError(f"reference_weights must be [Q] with Q = {dn.shape[0]} (or any Q for a tabulation at one point), got {w.shape}")
    det = np.abs(np.linalg.det(np.einsum("cgx,qgk->cqxk", x, dn)))  # [c][q or 1]
    return np.ascontiguousarray(det * w[None, :])


#: corner signs of the trilinear hexahedron on [-1, 1]^3, in the node order of ``hex8_reference_gradients``
HEX8_SIGNS = ((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1))


def hex8_reference_gradients() -> np.ndarray:
    """``[8][8][3]``: ``d N_a / d xi_k`` of the trilinear hexahedron on ``[-1, 1]^3`` at the 2 x 2 x 2 Gauss points.  Nodes in
    the counter-clockwise bottom-then-top order of ``HEX8_SIGNS``; point ``q`` is node ``q``'s corner scaled by ``1/sqrt(3)``
    (the order of ``examples/fe_mini.py``).  For other elements tabulate with basix."""
    sign = np.array(HEX8_SIGNS, dtype=np.float64)
    gp = sign / np.sqrt(3.0)
    ref = np.empty((8, 8, 3))
    for q in range(8):
        for a in range(8):
            for k in range(3):
                i, j = [d for d in range(3) if d != k]
                ref[q, a, k] = 0.125 * sign[a, k] * (1.0 + sign[a, i] * gp[q, i]) * (1.0 + sign[a, j] * gp[q, j])
    return ref


class GradArgs(C.Structure):
    """ctypes mirror of GradArgs (displacement_gradient.hip)"""

    _fields_ = [("du", C.c_void_p), ("dofmap", C.c_void_p), ("ref", C.c_void_p), ("jinv", C.c_void_p), ("out", C.c_void_p), ("n", C.c_int64)]


class DisplacementGradient:
    """``op(displacement) -> grad_del_u`` on the GPU for a fixed mesh.

    ``dofmap[C][A]`` (int32): the node numbers of every cell; ``reference_gradients[Q][A][D]`` (float64): the reference-element
    basis gradients at the quadrature points; ``inverse_jacobians[C][D][D]`` (affine cells) or ``[C][Q][D][D]`` (float64),
    ``[..][k][x] = d xi_k / d x_x`` (see ``inverse_jacobians()``); ``n_nodes``: the displacement has ``D * n_nodes`` entries,
    component ``r`` of node ``v`` at ``D*v + r`` (the blocked layout of dolfinx).  Point ``p = Q*c + q`` is point ``q`` of cell
    ``c``.  ``layout``: "nabla_grad" (``out[D*D*p + D*r + x] = d u_x / d x_r``, what the laws of this package read) or "grad"
    (``d u_r / d x_x``).

    Everything is validated on the host at construction, before anything is uploaded or launched: shapes and dtypes
    (``TypeError``), ``0 <= dofmap < n_nodes``, finite tables, the LDS cap of the module docstring and ``layout``
    (``ValueError``).  The kernel is compiled at construction (no GPU needed; cached by program text); the tables are uploaded on
    first use per device.  A law on a submesh gets its operator from ``dofmap[cells]`` / ``inverse_jacobians[cells]``."""

    def __init__(self, dofmap, reference_gradients, inverse_jacobians, n_nodes: int, *, layout: str = "nabla_grad", device=None):
        for name, a, dt in (("dofmap", dofmap, np.int32), ("reference_gradients", reference_gradients, np.float64),
                            ("inverse_jacobians", inverse_jacobians, np.float64)):
            if not isinstance(a, np.ndarray):
                raise TypeError(f"{name} must be a numpy.ndarray, got {type(a).__name__}")
            if a.dtype != dt:
                raise TypeError(f"{name} must be {np.dtype(dt).name}, got {a.dtype}")
        if isinstance(n_nodes, bool) or not isinstance(n_nodes, (int, np.integer)):
            raise TypeError(f"n_nodes must be an integer, got {type(n_nodes).__name__}")
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be one of {LAYOUTS}, got {layout!r}")
        if dofmap.ndim != 2:
            raise ValueError(f"dofmap must be [cells][nodes per cell], got shape {dofmap.shape}")
        if reference_gradients.ndim != 3:
            raise ValueError(f"reference_gradients must be [points][nodes][dimension], got shape {reference_gradients.shape}")
        n_cells, a_ = dofmap.shape
        q_, a2, d_ = reference_gradients.shape
        if d_ not in (1, 2, 3):
            raise ValueError(f"the geometric dimension must be 1, 2 or 3, got {d_}")
        if a2 != a_ or a_ < 1 or q_ < 1:
            raise ValueError(f"dofmap has {a_} nodes per cell, reference_gradients {a2} (and needs at least one point)")
        if inverse_jacobians.shape == (n_cells, d_, d_):
            affine = True
        elif inverse_jacobians.shape == (n_cells, q_, d_, d_):
            affine = False
        else:
            raise ValueError(f"inverse_jacobians must have shape {(n_cells, d_, d_)} or {(n_cells, q_, d_, d_)}, got {inverse_jacobians.shape}")
        if n_nodes < 1 or d_ * int(n_nodes) >= 2**62:
            raise ValueError(f"n_nodes = {n_nodes}")
        if n_cells and (int(dofmap.min()) < 0 or int(dofmap.max()) >= n_nodes):
            raise ValueError(f"dofmap entries must lie in [0, {n_nodes}), got [{int(dofmap.min())}, {int(dofmap.max())}]")
        if not np.isfinite(reference_gradients).all():
            raise ValueError("reference_gradients has non-finite entries")
        if not np.isfinite(inverse_jacobians).all():
            raise ValueError("inverse_jacobians has non-finite entries")
        self._code = compile_kernel(d_, a_, q_, affine, layout)  # (raises the LDS cap's ValueError)
        self._dofmap = np.ascontiguousarray(dofmap)
        self._ref = np.ascontiguousarray(reference_gradients)
        self._jinv = np.ascontiguousarray(inverse_jacobians)
        self.n_cells, self.nodes_per_cell, self.points_per_cell, self.gdim = int(n_cells), int(a_), int(q_), int(d_)
        self.n_points = self.n_cells * self.points_per_cell
        self.n_nodes = int(n_nodes)
        self.affine = affine
        self.layout = layout
        self._device = None if device is None else _device_index(device)
        self._on = {}  # device index -> (dofmap, ref, jinv, displacement buffer)

    @property
    def resources(self) -> dict:
        """``{"vgprs", "sgprs", "scratch_bytes", "lds_bytes", "waves_per_simd", ...}`` of the compiled kernel (compiler remarks)"""
        return dict(self._code.resources)

    @property
    def compile_log(self) -> str:
        return self._code.log

    @property
    def device(self) -> int:
        """index of the operator's device (``device=None``: the package's default device, fixed at first use)"""
        if self._device is None:
            self._device = _capi.default_device()
        return self._device

    def _tables(self, dev: int):
        t = self._on.get(dev)  # (the hit stays inline: this is on the path of every call)
        return t if t is not None else per_device(self._on, dev, lambda d: upload(d, self._dofmap, self._ref, self._jinv) + (doubles(self.gdim * self.n_nodes, d),))

    def __call__(self, displacement, out=None):
        """``grad_del_u`` of ``displacement`` (ndarray or device tensor of ``D * n_nodes`` float64) as a float64 device tensor of
        ``D*D * n_points``: ``out`` (contiguous, on the operator's device, 16-byte aligned; ``ValueError`` otherwise, before the
        launch) or a new one.  An ndarray is uploaded synchronously into a buffer the operator owns; the launch is asynchronous
        on torch's current stream."""
        import torch

        dev = self.device
        nd = self.gdim * self.n_nodes
        if _is_torch(displacement):
            _check_torch("displacement", displacement)
            if (displacement.device.index or 0) != dev:
                raise ValueError(f"displacement is on {displacement.device}, the operator on cuda:{dev}")
            if displacement.numel() != nd:
                raise ValueError(f"displacement has {displacement.numel()} entries, the mesh {self.gdim} x {self.n_nodes}")
            host = None
        else:
            if not isinstance(displacement, np.ndarray):
                raise TypeError(f"displacement must be a numpy.ndarray or a torch CUDA tensor, got {type(displacement).__name__}")
            if displacement.dtype != np.float64:
                raise TypeError(f"displacement must be float64, got {displacement.dtype}")
            if displacement.size != nd:
                raise ValueError(f"displacement has {displacement.size} entries, the mesh {self.gdim} x {self.n_nodes}")
            host = np.ascontiguousarray(displacement).reshape(-1)
        nout = self.gdim * self.gdim * self.n_points
        if out is not None:
            if not _is_torch(out) or out.dtype != torch.float64 or not out.is_cuda:
                raise ValueError("out must be a float64 device tensor")
            if (out.device.index or 0) != dev:
                raise ValueError(f"out is on {out.device}, the operator on cuda:{dev}")
            if not out.is_contiguous() or out.numel() != nout:
                raise ValueError(f"out must be contiguous with {nout} entries, got {out.numel()}")
            if out.data_ptr() % 16:
                raise ValueError("out must be 16-byte aligned")
        dofmap, ref, jinv, buf = self._tables(dev)
        with torch.cuda.device(dev):
            if out is None:
                out = torch.empty(nout, dtype=torch.float64, device=torch.device("cuda", dev))
            if self.n_points == 0:
                return out
            if host is not None:
                from .hostio import upload

                upload(buf, host)
                displacement = buf
            a = GradArgs(displacement.data_ptr(), dofmap.data_ptr(), ref.data_ptr(), jinv.data_ptr(), out.data_ptr(), self.n_points)
            blocks = min(((self.n_points + 63) // 64 + 3) // 4, BLOCKS_PER_CU * jit.num_cu(dev))  # a wave per 64-point tile, 4 waves per block
            jit.launch(self._code, dev, blocks, a, "DisplacementGradient launch")
        return out


def _device_index(device) -> int:
    if isinstance(device, (int, np.integer)):
        return int(device)
    import torch

    return torch.device(device).index or 0
