"""The Newton step solved on the GPU: preconditioned conjugate gradients on the assembled tangent stiffness.

``ConjugateGradient(K)`` solves ``K x = b`` for the values array a ``TangentMatrix`` wrote ("bsr" or "csr"), with the inverses of
the nodes' own blocks as a block-Jacobi preconditioner (or none).  Matrix, right-hand side, solution and all work vectors stay in
HBM; per solve a handful of scalars cross the link.  The solver solves the system as given: zero ``b`` at the constrained dofs
first (``torch.where`` on a device mask), as ``TangentMatrix.set_constrained`` makes their rows and columns the identity's.

Five run-time compiled kernels (``csrc/jit/conjugate_gradient.hip``, through ``jit.compile_program`` / ``jit.launch``).  The
arithmetic is fixed -- no floating-point atomics, no MFMA, ``-ffp-contract=off``, division is ``/`` -- so that a NumPy oracle
reproduces the bits, and the bits do not depend on the grid size, the CU count, ``check_every`` or the run:

*Matrix-vector product.*  ``q[D v + r] = 0.0``; for ``k`` ascending over ``indptr[v] .. indptr[v + 1]`` and ``s`` ascending:
``q = q + value(k, r, s) * p[D indices[k] + s]``; ``value(k, r, s)`` sits where ``TangentMatrix``'s ``dest_base`` / ``dest_stride``
pair says (the kernel recomputes both from ``indptr``; in scalar CSR a table of one column node per run of ``D`` values replaces
``indices``: only the values and the column indices stream).  Both formats: the same bits.

*Ordered dot.*  The vector is cut into segments of ``SEG`` = 3072 consecutive entries.  Within a segment lane ``t`` of 256 forms
``acc = 0.0; acc = acc + a[e] * b[e]`` over ``e = seg SEG + t + 256 i``, ``i`` ascending (entries past the end are skipped); the 256
values are added by the tree ``acc[t] = acc[t] + acc[t + h]``, ``h = 128, 64, .., 1``; ``acc[0]`` is the segment's partial, stored by
segment.  The block that finishes last (an integer counter behind a ``__threadfence()``) resets the counter and reduces the
partials by the same lane-strided sum (``acc = 0.0; acc = acc + partial[t + 256 i]``, ``i`` ascending over all segments) and the same
tree, once.  ``p . q`` is formed in the matrix-vector kernel (lane ``t`` owns the rows of its dot entries), ``r . r``, ``r . z`` and
``b . b`` in the update kernel.

*Block inverse*, once per call: ``D = 1``: ``1.0 / a``; ``D = 2``: ``det = a00*a11 - a01*a10``, ``inv = (a11, -a01, -a10, a00) / det``;
``D = 3``: the cofactors ``c00 = a11*a22 - a12*a21, c01 = a12*a20 - a10*a22, c02 = a10*a21 - a11*a20, c10 = a02*a21 - a01*a22,
c11 = a00*a22 - a02*a20, c12 = a01*a20 - a00*a21, c20 = a01*a12 - a02*a11, c21 = a02*a10 - a00*a12, c22 = a00*a11 - a01*a10``,
``det = a00*c00 + a01*c01 + a02*c02`` left to right, ``inv[i][j] = c[j][i] / det``.  A zero or non-finite ``det`` anywhere: status
``singular_block``, no iteration runs, ``x`` is ``x0``.  ``z[D v + r] = 0.0; z = z + inv[v][r][s] * r_[D v + s]``, ``s`` ascending.
Without the preconditioner ``z`` is ``r`` and ``rz`` is ``rr``.

*Start.*  ``x = x0`` (or ``+0.0``), ``r = b - K x0`` (``r = b``, no product, without ``x0``), ``z``, ``p = z``, ``rz``, ``rr``, ``bb = b . b``,
``thr2 = max(rtol*rtol*bb, atol*atol)``; ``rr <= thr2``: converged with 0 iterations (so ``b = 0`` returns at once).  A non-finite
``rr`` is ``nonfinite``, ``maxiter = 0`` is ``maxiter``.
*One iteration.*  ``q = K p``; ``pq = p . q``; not ``pq > 0``: ``indefinite``, nothing written.  ``alpha = rz / pq``; ``x = x + alpha*p``;
``r = r - alpha*q``; ``z = M^-1 r``; ``rz' = r . z``; ``rr = r . r``; the iteration is counted; ``rr <= thr2``: ``converged``; a non-finite
``rr``: ``nonfinite``; the count at ``maxiter``: ``maxiter``; else ``beta = rz' / rz``; ``p = z + beta*p``.

*Control.*  ``alpha``'s and ``beta``'s operands, the dots, ``thr2``, the count and the status live in a 96-byte block in device memory.
Every kernel reads what it needs there and returns at once when the status is not "running"; the last block of the update kernel
ends the iteration.  The host uploads the block once per solve (96 bytes), looks at it after the start, then enqueues ``check_every``
iterations of three launches (product, update, direction) and looks again: a look reads the block's first 32 bytes -- ``rr``, ``bb``,
status and count -- back through a page-locked buffer, and the host stops or enqueues the next batch (``SolveResult.looks``): iterations enqueued behind the end are no-ops, and
the result is the same bits for every ``check_every``.  No cooperative launch, no grid-wide barrier, no kernel that waits on a flag.

*Multilevel.*  With ``preconditioner="multilevel"`` (or a ``MultilevelPreconditioner`` of ``K``) the program is compiled with
``FCAMD_CG_PRECOND = 2``: the update kernel forms neither ``z`` nor ``rz``; the cycle's launches and a closing kernel (``multilevel.py``)
follow it in every iteration and in the start, and the coarse levels' products run in the matrix-vector kernel's mode 3, which
honours the status and touches neither ``pq`` nor the counter.

*Without a matrix.*  ``ConjugateGradient(A)`` with a ``TangentOperator`` (tangent_operator.py) solves the same system from the
tangent of the quadrature points: ``cg(tangent, b, x0=None, out=None)``.  The product and ``p . q`` come from the operator's two kernels
through the same seam (``_FreeOperator`` in ``_Operator``'s place; the same control block, modes and ordered dot), block-Jacobi from the
operator's diagonal-block kernels followed by THIS module's inverse kernel on the block array -- a BSR values array whose diagonal
table is ``0 .. n-1`` --, and the start, update and direction kernels are used as they are.  The multilevel preconditioner is an
instance built on the same operator, ``MultilevelPreconditioner(A)`` (program ``FCAMD_CG_PRECOND = 2`` as with a matrix): it needs no
fine matrix, its first coarse level is gathered from the element matrices (``multilevel.py``).  The string form "multilevel" builds
the preconditioner of a matrix and stays refused with an operator.

*The seam and the driver.*  What differs between a matrix and an operator is in ``_Operator`` and ``_FreeOperator`` (base ``_Seam``: the
check of a call's first argument, the node without a block of its own, the device tables, the product, the array the inverse kernel
reads the nodes' own blocks from); nothing else in the solvers or in ``multilevel.py`` asks which of the two ``K`` is.  What every
Krylov solver does on the host -- the validation of the options, the prelude of a call, the inverses, the loop of looks and batches,
the ``SolveResult`` -- is ``_Krylov``, once; ``ConjugateGradient`` here and ``bicgstab._BiCGStab`` supply a workspace, the start and "enqueue
one iteration" ("One Krylov driver").

LDS of a block: ``lds_bytes(kernel)``; the same ``LDS_CAP`` as the other operators.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import jit
from ._fe_common import overlap, per_device, upload
from .force import compile_without_scratch, kernel_resources
from .gradient import BLOCKS_PER_CU, LDS_CAP
from .matrix import TangentMatrix
from .tangent_operator import MODE_QUIET as _MODE_QUIET
from .tangent_operator import TangentOperator

MATVEC_KERNEL = "fcamd_cg_matvec_kernel"
UPDATE_KERNEL = "fcamd_cg_update_kernel"
DIRECTION_KERNEL = "fcamd_cg_direction_kernel"
INVERSE_KERNEL = "fcamd_cg_inverse_kernel"
DOT_KERNEL = "fcamd_cg_dot_kernel"
KERNELS = (MATVEC_KERNEL, UPDATE_KERNEL, DIRECTION_KERNEL, INVERSE_KERNEL, DOT_KERNEL)
#: entries of a segment of the ordered dot: 256 lanes x 12, divisible by 1, 2 and 3
SEG = 3072
#: doubles of values a wave of the matrix-vector kernel holds in LDS at a time
SLAB = 1024
PRECONDITIONERS = ("block_jacobi", None)
#: the status codes of the control block, in the kernels' order
STATUSES = ("running", "converged", "maxiter", "indefinite", "singular_block", "nonfinite")
_MODE_START, _MODE_ITERATE, _MODE_PLAIN = 0, 1, 2
#: doubles of the control block; the first four are what the host reads at a look: rr, bb and, as four int32, status, iterations,
#: maxiter and the counter
_SCALARS = 12
_LOOK = 4
_RR, _BB = 0, 1
_STATUS, _ITERATIONS, _MAXITER, _COUNTER = 4, 5, 6, 7  # int32 positions
_RZ, _RZ_OLD, _PQ, _THR2, _RTOL, _ATOL, _DOT = range(4, 11)

__all__ = ["ConjugateGradient", "SolveResult", "compile_kernels", "dot", "lds_bytes", "matvec", "program"]


def lds_bytes(kernel: str = MATVEC_KERNEL, preconditioned: bool = True, slab: int = SLAB) -> int:
    """LDS of one block of ``kernel``: the tree of the dot and the last-block flag (258 doubles) and, in the matrix-vector kernel,
    four wave regions of ``slab`` doubles, in the preconditioned update kernel the residual of a segment"""
    tree = 8 * (256 + 2)
    return {MATVEC_KERNEL: 8 * 4 * slab + tree, UPDATE_KERNEL: (8 * SEG if preconditioned else 0) + tree, DOT_KERNEL: tree, DIRECTION_KERNEL: 0, INVERSE_KERNEL: 0}[kernel]


def program(gdim: int, preconditioned: bool, slab: int = SLAB) -> str:
    """the program text of one block size (the compile cache is keyed by it)"""
    lines = [f"#define FCAMD_CG_D {int(gdim)}", f"#define FCAMD_CG_PRECOND {1 if preconditioned else 0}", f"#define FCAMD_CG_SLAB {int(slab)}",
             '#include "conjugate_gradient.hip"']
    return "\n".join(lines) + "\n"


def compile_kernels(gdim: int, preconditioned: bool, slab: int = SLAB):
    """The code object of one block size, all five kernels in it (no GPU needed).  A kernel with scratch, or a slab that does not
    fit the LDS, is a ``ValueError``."""
    if gdim not in (1, 2, 3):
        raise ValueError(f"the dofs per node must be 1, 2 or 3, got {gdim}")
    if slab < 128 or slab % 128:
        raise ValueError(f"the slab must be a positive multiple of 128 doubles, got {slab}")
    if lds_bytes(MATVEC_KERNEL, slab=slab) > LDS_CAP:
        raise ValueError(f"four wave regions of {slab} doubles need {lds_bytes(MATVEC_KERNEL, slab=slab)} bytes of LDS per block; at most {LDS_CAP} fit")
    return compile_without_scratch(program(gdim, preconditioned, slab), f"conjugate_gradient_{gdim}d", MATVEC_KERNEL, KERNELS)


class Args(C.Structure):
    """ctypes mirror of Args (conjugate_gradient.hip)"""

    _fields_ = [(name, C.c_void_p) for name in ("values", "indptr", "indices", "diag", "groups", "b", "x", "r", "z", "p", "q", "inv", "va", "vb",
                                                "partials", "sc")] + \
               [("n", C.c_int64), ("nnz", C.c_int64), ("nseg", C.c_int64), ("n_nodes", C.c_int64),
                ("csr", C.c_int32), ("mode", C.c_int32), ("has_x0", C.c_int32), ("pad", C.c_int32)]


@dataclass
class SolveResult:
    """``x``: the device tensor of the solution (``out`` when given); ``status``: one of ``STATUSES[1:]``; ``residual_norm``: the
    square root of the recurrence's ``r . r``; ``rhs_norm``: that of ``b . b``"""

    x: object
    iterations: int
    converged: bool
    status: str
    residual_norm: float
    rhs_norm: float
    looks: int = 0  #: times the host read the 32 bytes of status, count, rr and bb back (each waits for the stream)


def _segments(n: int) -> int:
    return -(-n // SEG)


class _Control:
    """the control block of one device, ``scalars`` doubles of it: the device copy, the page-locked host copy and the partial sums"""

    def __init__(self, dev: int, nseg: int, scalars: int = _SCALARS):
        import torch

        d = torch.device("cuda", dev)
        self.device_block = torch.zeros(scalars, dtype=torch.float64, device=d)
        self.pinned = torch.zeros(scalars, dtype=torch.float64).pin_memory()
        self.host = self.pinned.numpy()
        self.ints = self.host.view(np.int32)
        self.partials = torch.zeros(3 * max(nseg, 1), dtype=torch.float64, device=d)

    def upload(self, rtol=0.0, atol=0.0, maxiter=0):
        """a fresh block: status "running", nothing counted (asynchronous, on torch's current stream)"""
        self.host[:] = 0.0
        self.host[_RTOL], self.host[_ATOL] = rtol, atol
        self.ints[_MAXITER] = maxiter
        self.device_block.copy_(self.pinned, non_blocking=True)

    def download(self, dev: int, doubles: int = _LOOK):
        """the first ``doubles`` of the block as the kernels left them -- 32 bytes: rr, bb, status and count -- (synchronises torch's
        current stream)"""
        import torch

        self.pinned[:doubles].copy_(self.device_block[:doubles], non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()


class _Seam:
    """What the solvers and the multilevel preconditioner ask of ``K`` and nothing else reads it for: the check of a call's first
    argument, the nodes without a block of their own, the tables on the device, ``q = K p`` with ``p . q`` behind it, the array the
    inverse kernel reads the nodes' own blocks from, and the control block of the plain product.  One per matrix or operator, kept on
    that object (``_operator``), so the tables are uploaded once and go with it.  A class gives ``first`` and ``first_numel`` (the name
    and length of the first argument), ``other`` (the refusal of a preconditioner built on another object), ``by_name`` (whether
    ``preconditioner="multilevel"`` can build one), ``block_numel`` (the entries of the ``out`` of ``own_blocks``, 0: it needs none),
    ``_host_tables``, ``args``, ``apply``, ``refuse_missing`` and ``own_blocks``."""

    def __init__(self, K, n: int):
        self.matrix, self.gdim, self.n, self.n_nodes = K, K.gdim, n, K.n_nodes
        self.nseg = _segments(n)
        self._on = {}  # device index -> the tables of _host_tables
        self._control = {}  # device index -> _Control (of the plain product)

    def check(self, values, dev: int) -> None:
        """the first argument of a call: a float64 tensor of ``first_numel`` entries on the device"""
        self.matrix._check(self.first, values, self.first_numel, dev)

    def tables(self, dev: int):
        t = self._on.get(dev)  # (the hit stays inline: this is on the path of every call)
        return t if t is not None else per_device(self._on, dev, lambda d: upload(d, *self._host_tables()))

    def control(self, dev: int) -> _Control:
        c = self._control.get(dev)
        if c is None:
            c = self._control[dev] = _Control(dev, self.nseg)
        return c

    def blocks(self, dev: int) -> int:
        """blocks of a launch over the segments: looked up on ``jit`` at launch"""
        return max(1, min(self.nseg, BLOCKS_PER_CU * jit.num_cu(dev)))


class _Operator(_Seam):
    """the seam of a ``TangentMatrix``: the assembled matrix, its values array the first argument of every call"""

    first, by_name, block_numel = "values", True, 0
    other = "the MultilevelPreconditioner was built for another matrix"

    def __init__(self, matrix: TangentMatrix):
        d_ = matrix.gdim
        dd = d_ * d_
        # the kernels locate value(k, r, s) from indptr; that must be what the matrix's own tables say
        k = np.arange(matrix.nnzb, dtype=np.int64)
        per_row = np.diff(matrix.indptr.astype(np.int64))
        if matrix.format == "bsr":
            base, stride = dd * k, np.full(matrix.nnzb, d_, dtype=np.int64)
        else:
            k0 = matrix.indptr[:-1].astype(np.int64)[matrix.block_row]
            base, stride = dd * k0 + d_ * (k - k0), d_ * per_row[matrix.block_row]
        if not (np.array_equal(base, matrix.dest_base) and np.array_equal(stride, matrix.dest_stride)):
            raise ValueError(f"the values of format {matrix.format!r} are not where the solver's kernels look for them")
        super().__init__(matrix, d_ * matrix.n_nodes)
        self.nnz = self.first_numel = matrix.nnz
        self.csr = 1 if matrix.format == "csr" else 0

    def refuse_missing(self) -> None:
        missing = np.flatnonzero(self.matrix.diag_block < 0)
        if missing.size:
            raise ValueError(f"node {int(missing[0])} has no diagonal block in the pattern: its row is empty, the matrix singular")

    def _host_tables(self):
        """(indptr, indices, diag, groups)"""
        m = self.matrix
        # scalar CSR: the node of the columns of every run of D values (the rows of a block are apart there)
        groups = (m.csr_indices[:: self.gdim] // self.gdim).astype(np.int32) if self.csr and m.nnzb else np.zeros(1, dtype=np.int32)
        return m.indptr, m.indices if m.nnzb else np.zeros(1, dtype=np.int32), np.maximum(m.diag_block, 0).astype(np.int32), groups

    def args(self, dev: int, values, control: _Control) -> Args:
        indptr, indices, diag, groups = self.tables(dev)
        a = Args()
        a.values, a.indptr, a.indices, a.diag, a.groups = values.data_ptr(), indptr.data_ptr(), indices.data_ptr(), diag.data_ptr(), groups.data_ptr()
        a.partials, a.sc = control.partials.data_ptr(), control.device_block.data_ptr()
        a.n, a.nnz, a.nseg, a.n_nodes, a.csr = self.n, self.nnz, self.nseg, self.n_nodes, self.csr
        return a

    def own_blocks(self, dev: int, values, out) -> int:
        """the pointer the inverse kernel reads the nodes' own blocks from, through the diagonal table: the values themselves
        (``out`` is not used)"""
        return values.data_ptr()

    def apply(self, code, dev: int, a: Args, vector_ptr: int, out_ptr: int, mode: int) -> None:
        """``out = K vector`` and the ordered ``vector . out`` (``_MODE_ITERATE``: into ``pq``, under the status; ``_MODE_PLAIN``: into ``dot``)
        by the matrix-vector kernel of ``code`` (``None``: of the program without a preconditioner)"""
        a.va, a.q, a.mode = vector_ptr, out_ptr, mode
        jit.launch(code or _plain_code(self.gdim), dev, self.blocks(dev), a, "ConjugateGradient matrix-vector launch", kernel=MATVEC_KERNEL)


class _FreeOperator(_Seam):
    """The seam of a ``TangentOperator``: ``q = A p`` with ``p . q`` behind it by the operator's own two kernels, from the tangent of
    the quadrature points, the first argument of every call.  The block array the inverse kernel reads is a BSR values array whose
    pattern is the diagonal: ``indptr`` and the diagonal table are both ``0 .. n``, one table on the device."""

    first, by_name = "tangent", False
    other = ("the MultilevelPreconditioner was built for another object: the multilevel preconditioner of a TangentOperator A is "
             "MultilevelPreconditioner(A), built on this very operator")

    def __init__(self, operator: TangentOperator):
        super().__init__(operator, operator.shape[0])
        self.nnz, self.csr = 0, 0
        self.first_numel = operator.tangent_dim * operator.n_points
        self.block_numel = self.gdim**2 * self.n_nodes

    def refuse_missing(self) -> None:
        missing = np.flatnonzero(self.matrix.valence == 0)
        if missing.size:
            raise ValueError(f"node {int(missing[0])} belongs to no cell: it has no diagonal block, its row is empty, the matrix singular")

    def _host_tables(self):
        """(0 .. n_nodes as int32,)"""
        return (np.arange(self.n_nodes + 1, dtype=np.int32),)

    def args(self, dev: int, tangent, control: _Control) -> Args:
        (count,) = self.tables(dev)
        a = Args()
        a.indptr = a.indices = a.diag = a.groups = count.data_ptr()
        a.partials, a.sc = control.partials.data_ptr(), control.device_block.data_ptr()
        a.n, a.nnz, a.nseg, a.n_nodes, a.csr = self.n, self.gdim * self.gdim * self.n_nodes, self.nseg, self.n_nodes, 0
        a.values = tangent.data_ptr()  # (the inverse kernel is launched with the block array in its place)
        return a

    def own_blocks(self, dev: int, tangent, out) -> int:
        """the nodes' own blocks, formed now into ``out``, the caller's ``[n_nodes][D][D]``, by the operator's two diagonal kernels
        (asynchronous): a BSR values array over the diagonal pattern, which is what the table ``0 .. n`` makes of it"""
        return self.matrix.diagonal_blocks(tangent, out=out).data_ptr()

    def apply(self, code, dev: int, a: Args, vector_ptr: int, out_ptr: int, mode: int) -> None:
        """``out = A vector`` and the ordered ``vector . out`` by the operator's kernels (``code``, the solver's program, is not used)"""
        a.va, a.q, a.mode = vector_ptr, out_ptr, mode  # (as _Operator.apply leaves them: the update kernel reads the mode)
        self.matrix._apply(dev, a.values, vector_ptr, out_ptr, mode, a.partials, a.sc)


_dot_control: dict = {}  # device index -> (_Control, segments it holds)


_plain: dict = {}  # dofs per node -> the code object without the preconditioner (solver.matvec, solver.dot)


def _plain_code(gdim: int):
    code = _plain.get(gdim)
    if code is None:
        code = _plain[gdim] = compile_kernels(gdim, False)
    return code


def _operator(matrix: TangentMatrix) -> _Operator:
    """the operator of ``matrix``, made at the first use and kept on the matrix object: it lives and dies with it"""
    op = getattr(matrix, "_solver_operator", None)
    if op is None:
        op = matrix._solver_operator = _FreeOperator(matrix) if isinstance(matrix, TangentOperator) else _Operator(matrix)
    return op


def matvec(K: TangentMatrix, values, p, out=None):
    """``out = K p`` by the solver's matrix-vector kernel (asynchronous, on torch's current stream): ``values`` the array ``K``
    wrote, ``p`` and ``out`` float64 device tensors of ``D n_nodes`` entries.  A row without blocks is ``+0.0``.  With a
    ``TangentOperator`` ``values`` is the tangent of the quadrature points and the product the operator's own.  The ordered
    ``p . out`` is left in the ``dot`` of the control block the seam keeps."""
    import torch

    if not isinstance(K, (TangentMatrix, TangentOperator)):
        raise TypeError(f"K must be a TangentMatrix, got {type(K).__name__}")
    op = _operator(K)
    dev, n = K.device, op.n
    op.check(values, dev)
    K._check("p", p, n, dev)
    if out is not None:
        K._check("out", out, n, dev)
        if _overlap(out, p):
            raise ValueError("out must not alias p")
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=torch.device("cuda", dev))
        if n:
            op.apply(None, dev, op.args(dev, values, op.control(dev)), p.data_ptr(), out.data_ptr(), _MODE_PLAIN)
    return out


def dot(a, b) -> float:
    """``a . b`` of two float64 device tensors in the solver's fixed order (synchronous: it returns the number)"""
    import torch

    from .device import _is_torch

    for name, v in (("a", a), ("b", b)):
        if not _is_torch(v):
            raise TypeError(f"{name} must be a torch CUDA tensor, got {type(v).__name__}")
        if v.dtype != torch.float64:
            raise TypeError(f"{name} must be float64, got {v.dtype}")
        if not v.is_cuda:
            raise ValueError(f"{name} is on {v.device}, not on a GPU")
        if not v.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if a.device != b.device:
        raise ValueError(f"a is on {a.device}, b on {b.device}")
    if a.numel() != b.numel():
        raise ValueError(f"a has {a.numel()} entries, b {b.numel()}")
    n = a.numel()
    if n == 0:
        return 0.0
    dev = a.device.index or 0
    nseg = _segments(n)
    code = _plain_code(1)
    with torch.cuda.device(dev):
        have = _dot_control.get(dev)
        if have is None or have[1] < nseg:
            have = _dot_control[dev] = (_Control(dev, nseg), nseg)
        control = have[0]
        control.upload()
        args = Args()
        args.va, args.vb, args.partials, args.sc, args.n, args.nseg = a.data_ptr(), b.data_ptr(), control.partials.data_ptr(), control.device_block.data_ptr(), n, nseg
        jit.launch(code, dev, max(1, min(nseg, BLOCKS_PER_CU * jit.num_cu(dev))), args, "ConjugateGradient dot launch", kernel=DOT_KERNEL)
        control.download(dev, _SCALARS)
    return float(control.host[_DOT])


_overlap = overlap  # (bicgstab_free.py and multilevel.py read it from here)


class _Krylov:
    """The host side of a Krylov solver on the seam, written once: the validation of the options, the prelude of a call (the checks
    of the tensors, the alias rules, ``x`` from ``x0`` / ``out``, the empty system), the block array of an operator's block-Jacobi, the
    inverses a preconditioner applies, and the loop of uploads, looks and batches that ends in a ``SolveResult``.  A subclass sets
    ``_code``, the code object the inverse kernel is launched from, and supplies ``_workspace(dev)``, the tuple of the control block and
    its vectors, and ``_start(dev, values, b, x, has_x0, work)``, which enqueues everything up to the first look and returns the
    function that enqueues one iteration."""

    _STATUSES = STATUSES

    def __init__(self, K, preconditioner, rtol, atol, maxiter, check_every):
        from .multilevel import MultilevelPreconditioner

        op = _operator(K)
        named = isinstance(preconditioner, str) and preconditioner == "multilevel"
        if named and not op.by_name:
            raise ValueError('preconditioner="multilevel" builds the multilevel preconditioner of a matrix: with a TangentOperator A pass the instance, '
                             f"MultilevelPreconditioner(A), or one of {PRECONDITIONERS}")
        if isinstance(preconditioner, MultilevelPreconditioner):
            if preconditioner.K is not K:
                raise ValueError(op.other)
        elif not (named or preconditioner is None or (isinstance(preconditioner, str) and preconditioner == "block_jacobi")):
            names = PRECONDITIONERS + (("multilevel",) if op.by_name else ())
            raise ValueError(f"preconditioner must be one of {names} or a MultilevelPreconditioner of K, got {preconditioner!r}")
        for name, v in (("rtol", rtol), ("atol", atol)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise TypeError(f"{name} must be a number, got {type(v).__name__}")
            if not (v >= 0.0 and np.isfinite(v)):
                raise ValueError(f"{name} must be finite and not negative, got {v}")
        if maxiter is None:
            maxiter = 10 * op.n
        for name, v, least in (("maxiter", maxiter, 0), ("check_every", check_every, 1)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{name} must be an integer, got {type(v).__name__}")
            if v < least or v >= 2**31:
                raise ValueError(f"{name} must lie in [{least}, 2^31), got {v}")
        op.refuse_missing()
        if named:  # (once everything else has been validated)
            preconditioner = MultilevelPreconditioner(K)
        self.K = K
        self.preconditioner = preconditioner
        self.rtol, self.atol, self.maxiter, self.check_every = float(rtol), float(atol), int(maxiter), int(check_every)
        self._op = op
        #: the multilevel preconditioner (its cycle runs on this solver's control block), or None
        self._ml = preconditioner if isinstance(preconditioner, MultilevelPreconditioner) else None
        self.n = op.n
        self._name = type(self).__name__  # of the launches, in ``jit.launch``'s errors
        self._work = {}  # device index -> _workspace(dev)
        self._work_blocks = {}  # device index -> the block array of a TangentOperator's block-Jacobi

    @property
    def compile_log(self) -> str:
        return self._code.log

    @property
    def device(self) -> int:
        return self.K.device

    def _diagonal_blocks(self, dev: int):
        """the block array of a ``TangentOperator``'s block-Jacobi, ``[n_nodes][D][D]``, one per device (a matrix needs none)"""
        blocks = self._work_blocks.get(dev)
        if blocks is None and self._op.block_numel:
            import torch

            blocks = self._work_blocks[dev] = torch.zeros(self._op.block_numel, dtype=torch.float64, device=torch.device("cuda", dev))
        return blocks

    def _inverses(self, dev: int, values, a: Args, control: _Control) -> None:
        """what the preconditioner applies, formed from ``values``: the multilevel setup, or the inverses of the nodes' own blocks by the
        inverse kernel of ``_code`` on ``a``, or nothing"""
        if self._ml is not None:  # (on an operator ``values`` is the tangent: the preconditioner forms the blocks and level 1 from it)
            self._ml._setup(dev, values, control)
        elif self.preconditioner:
            a.values = self._op.own_blocks(dev, values, self._diagonal_blocks(dev))
            jit.launch(self._code, dev, max(1, min(-(-self._op.n_nodes // 256), BLOCKS_PER_CU * jit.num_cu(dev))), a, f"{self._name} inverse launch",
                       kernel=INVERSE_KERNEL)
            a.values = values.data_ptr()

    def __call__(self, values, b, x0=None, out=None) -> SolveResult:
        """solve ``K x = b`` (synchronous at its end); with a ``TangentOperator`` the first argument is the tangent of the quadrature
        points"""
        import torch

        K, dev, n = self.K, self.device, self.n
        self._op.check(values, dev)
        K._check("b", b, n, dev)
        if x0 is not None:
            K._check("x0", x0, n, dev)
        if out is not None:
            K._check("out", out, n, dev)
            if _overlap(out, b):
                raise ValueError("out must not alias b")
            if x0 is not None and _overlap(out, x0) and out.data_ptr() != x0.data_ptr():
                raise ValueError("out may be x0 itself, not a part of it")
        with torch.cuda.device(dev):
            if out is None:
                x = torch.zeros(n, dtype=torch.float64, device=torch.device("cuda", dev)) if x0 is None else x0.clone()
            else:
                x = out
                if x0 is None:
                    x.zero_()
                elif x.data_ptr() != x0.data_ptr():
                    x.copy_(x0)
            if n == 0:
                return SolveResult(x, 0, True, "converged", 0.0, 0.0, 0)
            work = self._workspace(dev)
            control = work[0]
            control.upload(self.rtol, self.atol, self.maxiter)
            iterate = self._start(dev, values, b, x, x0 is not None, work)
            control.download(dev)  # a solve that ends at its start (b = 0, a singular block, maxiter = 0) enqueues no iteration
            looks = 1
            while int(control.ints[_STATUS]) == 0:
                for _ in range(self.check_every):
                    iterate()
                control.download(dev)
                looks += 1
            h, status = control.host, int(control.ints[_STATUS])
            return SolveResult(x, int(control.ints[_ITERATIONS]), status == 1, self._STATUSES[status], float(np.sqrt(h[_RR])), float(np.sqrt(h[_BB])), looks)


class ConjugateGradient(_Krylov):
    """``cg(values, b, x0=None, out=None) -> SolveResult``: ``K x = b`` by preconditioned conjugate gradients on the GPU.

    ``K``: the ``TangentMatrix`` whose values array is solved with, in either format.  ``preconditioner``: "block_jacobi" -- the
    inverses of the nodes' own blocks, formed from ``values`` at every call --, ``None``, or "multilevel" -- a
    ``MultilevelPreconditioner(K)`` with its defaults -- or such an object built for the same ``K`` (multilevel.py: its Galerkin values
    and inverses are formed at every call, its cycle and closing kernel run between the update and the direction kernel, and a
    preconditioned residual with ``r . z`` not positive ends the solve as ``indefinite``).  The iteration stops at
    ``r . r <= max(rtol^2 b . b, atol^2)`` (the recurrence's residual) or after ``maxiter`` iterations (default ``10 D n_nodes``);
    ``check_every``: iterations enqueued between two looks at the status (the result does not depend on it).

    ``values``, ``b``, ``x0`` and ``out`` are float64 device tensors (``nnz``, and ``D n_nodes`` entries); the solution is ``out`` or a new
    tensor.  ``out`` may be ``x0`` itself, never ``b``.  Everything is validated on the host before anything is uploaded or launched
    (``TypeError`` / ``ValueError`` as for ``TangentMatrix``).  The kernels are compiled at construction (no GPU needed); a pattern in
    which a node has no diagonal block -- an empty row, a singular matrix -- is refused there.  Work vectors, the inverse blocks,
    the partial sums and the control block belong to the object, one set per device, allocated at the first call.  All launches
    go to torch's current stream; THE CALL IS SYNCHRONOUS AT ITS END (and at every look before): it reads the final status, count
    and norms back, so the stream has been waited for when it returns.  Use an object from one stream at a time.

    ``K`` may be a ``TangentOperator`` instead: the call is then ``cg(tangent, b, x0=None, out=None)`` with the ``S*S n_points`` tangent a law
    wrote in the values' place, ``preconditioner`` is "block_jacobi", ``None`` or a ``MultilevelPreconditioner`` built on this very operator
    (translations only; the string "multilevel", or an instance built on another object: a ``ValueError``), and a node that belongs to
    no cell is refused at construction as a missing diagonal block is.  Everything else -- ``x0``, ``check_every``, the statuses, ``SolveResult`` and its ``looks`` -- is the same."""

    def __init__(self, K: TangentMatrix, preconditioner="block_jacobi", rtol: float = 1e-8, atol: float = 0.0, maxiter: int | None = None,
                 check_every: int = 16):
        if not isinstance(K, (TangentMatrix, TangentOperator)):
            raise TypeError(f"K must be a TangentMatrix, got {type(K).__name__}")
        super().__init__(K, preconditioner, rtol, atol, maxiter, check_every)
        # (the multilevel preconditioner's program holds the solver's kernels too: z and rz come from its cycle)
        self._code = self._ml._code if self._ml is not None else compile_kernels(K.gdim, self.preconditioner is not None)

    @property
    def resources(self) -> dict:
        """``{"vgprs", "sgprs", "scratch_bytes", "lds_bytes", "waves_per_simd", ...}`` of the matrix-vector kernel, under "update",
        "direction", "inverse" and "dot" those of the other kernels (compiler remarks), under "slab" the doubles per slab"""
        r = kernel_resources(self._code.log, MATVEC_KERNEL)
        for name, kernel in (("update", UPDATE_KERNEL), ("direction", DIRECTION_KERNEL), ("inverse", INVERSE_KERNEL), ("dot", DOT_KERNEL)):
            r[name] = kernel_resources(self._code.log, kernel)
        r["slab"] = SLAB
        return r

    def _workspace(self, dev: int):
        """(control, r, z, p, q, inv)"""
        w = self._work.get(dev)
        if w is None:
            import torch

            d = torch.device("cuda", dev)
            vectors = [torch.zeros(self.n, dtype=torch.float64, device=d) for _ in range(4 if self.preconditioner else 3)]
            if not self.preconditioner:
                vectors.insert(1, vectors[0])  # z is r
            inv = torch.zeros(self.K.gdim**2 * self.K.n_nodes if self.preconditioner and self._ml is None else 2, dtype=torch.float64, device=d)
            w = self._work[dev] = (_Control(dev, self._op.nseg), *vectors, inv)
        return w

    def _start(self, dev: int, values, b, x, has_x0: bool, work):
        control, r, z, p, q, inv = work
        op, code, ml, n = self._op, self._code, self._ml, self.n
        a = op.args(dev, values, control)
        a.b, a.x, a.r, a.z, a.p, a.q, a.inv = (t.data_ptr() for t in (b, x, r, z, p, q, inv))
        a.has_x0 = 1 if has_x0 else 0
        self._inverses(dev, values, a, control)
        if has_x0:
            op.apply(code, dev, a, x.data_ptr(), q.data_ptr(), _MODE_PLAIN)
        a.mode = _MODE_START
        jit.launch(code, dev, op.blocks(dev), a, "ConjugateGradient start launch", kernel=UPDATE_KERNEL)
        if ml is not None:
            ml._cycle(dev, values, control, r.data_ptr(), z.data_ptr())
            ml._close(dev, control, r, z, p, start=True)
        direction_blocks = max(1, min(-(-n // 256), BLOCKS_PER_CU * jit.num_cu(dev)))

        def iterate():
            op.apply(code, dev, a, p.data_ptr(), q.data_ptr(), _MODE_ITERATE)
            jit.launch(code, dev, op.blocks(dev), a, "ConjugateGradient update launch", kernel=UPDATE_KERNEL)
            if ml is not None:
                ml._cycle(dev, values, control, r.data_ptr(), z.data_ptr())
                ml._close(dev, control, r, z, p, start=False)
            jit.launch(code, dev, direction_blocks, a, "ConjugateGradient direction launch", kernel=DIRECTION_KERNEL)

        return iterate
