"""The Newton step of an unsymmetric tangent solved on the GPU: right-preconditioned BiCGStab on the assembled tangent stiffness.

``BiCGStab(K)`` solves ``K x = b`` for the values array a ``TangentMatrix`` wrote ("bsr" or "csr") when ``K`` is not symmetric --
Drucker-Prager with ``b != b_flow``, a ``JaumannRate`` around any law, a ``UserLaw`` with a non-associated tangent --, where
``ConjugateGradient`` ends as ``indefinite`` or ``maxiter`` or drifts.  Arguments, validation, errors, looks and ``SolveResult`` are
those of the driver both solvers stand on (``solver._Krylov``); one status is new, ``"breakdown"``.

Five run-time compiled kernels (``csrc/jit/bicgstab.hip``) beside the matrix-vector, inverse and dot kernels of
``csrc/jit/conjugate_gradient.hip``, which the program includes.  The arithmetic is fixed as in ``solver.py`` -- the same
matrix-vector product, the same ordered dot (segments of ``SEG`` entries, 256-lane tree, last-block reduction), the same block
inverses, no floating-point atomics, no MFMA, ``-ffp-contract=off``, division is ``/`` -- so that a NumPy oracle reproduces the
bits, and the bits do not depend on the grid size, the CU count, ``check_every`` or the run.  ``M^-1 w`` is ``w`` itself
(``preconditioner=None``), ``m[D v + r] = 0.0; m = m + inv[v][r][s] * w[D v + s]``, ``s`` ascending (block-Jacobi), or one multilevel
cycle (``multilevel.py``; a fixed linear operator that needs no symmetry).

*Start.*  ``x = x0`` (or ``+0.0``), ``r = b - K x0`` (``r = b``, no product, without ``x0``), ``rhat = r``, ``p = r``, ``rr = r . r``,
``rho = rr``, ``bb = b . b``, ``thr2 = max(rtol*rtol*bb, atol*atol)``; ``rr <= thr2``: converged with 0 iterations; a non-finite ``rr``:
``nonfinite``; ``maxiter = 0``: ``maxiter``; a zero or non-finite determinant of a node's own block (any level): ``singular_block``, no
iteration runs, ``x`` is ``x0``.
*One iteration.*

1. ``y = M^-1 p``; ``v = K y``; ``rv = rhat . v`` (the products ``v[e] * rhat[e]``).  ``rv`` zero or not finite: ``breakdown``, nothing
   written.
2. ``alpha = rho / rv``; ``x = x + alpha*y``; ``s = r - alpha*v`` (written over ``r``); ``ss = s . s``; ``rr = ss``.  ``ss <= thr2``: the
   iteration is counted, ``converged``.
3. ``z = M^-1 s``; ``t = K z``; ``ts = t . s``; ``tt = t . t``; ``omega = ts / tt``.  ``tt`` or ``omega`` zero or not finite: ``breakdown``
   (``x`` keeps the half step, the iteration is not counted).
4. ``x = x + omega*z``; ``r = s - omega*t``; ``rr = r . r``; ``rho' = rhat . r`` (the products ``rhat[e] * r[e]``).  The iteration is
   counted; ``rr <= thr2``: ``converged``; else a non-finite ``rr``: ``nonfinite``; else ``rho'`` zero or not finite: ``breakdown``; else the
   count at ``maxiter``: ``maxiter``.
5. ``beta = (rho' / rho) * (alpha / omega)``; ``p = r + beta*(p - omega*v)`` (``omega*v``, the difference, ``beta`` times it, the sum);
   ``rho = rho'``.

``residual_norm`` is the square root of the last ``rr``: the recurrence's residual, which in BiCGStab drifts from ``b - K x`` by a
few digits more than in conjugate gradients.

*Control.*  The scalars live in a 128-byte block in device memory whose first 32 bytes -- ``rr``, ``bb``, status, count, ``maxiter``,
counter -- and ``thr2``, ``rtol``, ``atol`` lie where ``ConjugateGradient``'s block has them, so the host's look and the multilevel
kernels' status test are unchanged.  Every kernel returns at once when the status is not "running"; a scalar the lanes of a
kernel read is written by the last block of an EARLIER kernel only (``alpha`` and ``omega`` travel to the direction kernel in the
block).  Per iteration five launches -- product, half step, product, full step, direction -- and, with the multilevel
preconditioner, its cycle's launches before either product (``p -> y``, ``s -> z``; the closing kernel is not used).  No cooperative
launch, no grid-wide barrier, no kernel that waits on a flag.

LDS of a block: ``lds_bytes(kernel, preconditioner)``.

The recurrence's host side is ``_BiCGStab``, written once on the operator seam of ``solver.py``.  ``BiCGStab`` takes a
``TangentMatrix`` only and adds the assembled products (``K x0`` by the conjugate gradients' matrix-vector kernel, the product kernel
above); ``bicgstab_free.MatrixFreeBiCGStab`` takes a ``TangentOperator`` and adds the operator's own.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import jit, solver
from .force import compile_without_scratch, kernel_resources
from .gradient import BLOCKS_PER_CU, LDS_CAP
from .matrix import TangentMatrix
from .solver import SEG, SLAB

PRODUCT_KERNEL = "fcamd_bcg_product_kernel"
START_KERNEL = "fcamd_bcg_start_kernel"
HALF_KERNEL = "fcamd_bcg_half_kernel"
FULL_KERNEL = "fcamd_bcg_full_kernel"
DIRECTION_KERNEL = "fcamd_bcg_direction_kernel"
KERNELS = (PRODUCT_KERNEL, START_KERNEL, HALF_KERNEL, FULL_KERNEL, DIRECTION_KERNEL)
#: the kernels of conjugate_gradient.hip the solver launches as well: K x0, the block inverses
SHARED_KERNELS = (solver.MATVEC_KERNEL, solver.INVERSE_KERNEL)
#: the status codes of the control block, in the kernels' order ("indefinite" is ConjugateGradient's alone)
STATUSES = solver.STATUSES + ("breakdown",)
#: FCAMD_CG_PRECOND of a preconditioner kind
PRECOND = {None: 0, "block_jacobi": 1, "multilevel": 2}
_DOT_V, _DOT_T = 0, 1
#: entries of a block's trip in the block-Jacobi direction kernel
_CHUNK = 768
#: doubles of the control block: the twelve of ConjugateGradient's layout (rho, rho_old and rv where rz, rz_old and pq are; ts
#: in the spare one) and tt, alpha, omega, one spare
_SCALARS = 16

__all__ = ["BiCGStab", "STATUSES", "compile_kernels", "lds_bytes", "program"]


def _kind(preconditioner) -> int:
    if isinstance(preconditioner, (int, np.integer)) and not isinstance(preconditioner, bool) and preconditioner in (0, 1, 2):
        return int(preconditioner)
    if preconditioner is None or isinstance(preconditioner, str) and preconditioner in PRECOND:
        return PRECOND[preconditioner]
    raise ValueError(f"preconditioner must be one of {tuple(PRECOND)} (or 0, 1, 2), got {preconditioner!r}")


def lds_bytes(kernel: str = PRODUCT_KERNEL, preconditioner="block_jacobi", slab: int = SLAB) -> int:
    """LDS of one block of ``kernel``: the tree of the dots and the last-block flag (258 doubles) and, in the product kernel, four
    wave regions of ``slab`` doubles (the conjugate-gradient product's size: its two trees share one array), in the block-Jacobi
    half-step kernel a segment of ``s``; nothing in the direction kernel"""
    tree = 8 * (256 + 2)
    if kernel in solver.KERNELS:
        return solver.lds_bytes(kernel, _kind(preconditioner) == 1, slab)
    return {PRODUCT_KERNEL: 8 * 4 * slab + tree, START_KERNEL: tree, HALF_KERNEL: (8 * SEG if _kind(preconditioner) == 1 else 0) + tree, FULL_KERNEL: tree,
            DIRECTION_KERNEL: 0}[kernel]


def program(gdim: int, preconditioner="block_jacobi", slab: int = SLAB) -> str:
    """the program text of one block size and preconditioner kind (the compile cache is keyed by it)"""
    return "\n".join([f"#define FCAMD_CG_D {int(gdim)}", f"#define FCAMD_CG_PRECOND {_kind(preconditioner)}", f"#define FCAMD_CG_SLAB {int(slab)}",
                      '#include "bicgstab.hip"']) + "\n"


def compile_kernels(gdim: int, preconditioner="block_jacobi", slab: int = SLAB):
    """The code object of one block size and preconditioner kind (``None``, "block_jacobi", "multilevel" or 0, 1, 2), the five
    kernels and those of conjugate_gradient.hip in it (no GPU needed).  A kernel with scratch, or a slab that does not fit the LDS,
    is a ``ValueError``."""
    if gdim not in (1, 2, 3):
        raise ValueError(f"the dofs per node must be 1, 2 or 3, got {gdim}")
    kind = _kind(preconditioner)
    if slab < 128 or slab % 128:
        raise ValueError(f"the slab must be a positive multiple of 128 doubles, got {slab}")
    if lds_bytes(PRODUCT_KERNEL, slab=slab) > LDS_CAP:
        raise ValueError(f"four wave regions of {slab} doubles need {lds_bytes(PRODUCT_KERNEL, slab=slab)} bytes of LDS per block; at most {LDS_CAP} fit")
    return compile_without_scratch(program(gdim, kind, slab), f"bicgstab_{gdim}d", PRODUCT_KERNEL, KERNELS + SHARED_KERNELS)


class Params(C.Structure):
    """ctypes mirror of fcamd_bcg::Params (bicgstab.hip)"""

    _fields_ = [("cg", solver.Args), ("rhat", C.c_void_p), ("v", C.c_void_p), ("t", C.c_void_p), ("y", C.c_void_p)]


class _Control(solver._Control):
    """the control block of one device, ``_SCALARS`` doubles of it (``upload`` and ``download`` are the conjugate gradients': rtol,
    atol and maxiter lie where they do there)"""

    def __init__(self, dev: int, nseg: int):
        super().__init__(dev, nseg, _SCALARS)


class _BiCGStab(solver._Krylov):
    """The recurrence of the module docstring on the driver of ``solver.py``, written once for both operators: the workspace, the
    start and one iteration -- cycle, product, half step, cycle, product, full step, direction.  A subclass accepts its kind of
    ``K`` and supplies ``_first_product(dev, values, a, x, v)``, which enqueues ``v = K x0``, and ``_products(dev, values, a, control)``, the
    function ``product(vector, result, other, dots)`` that enqueues ``result = K vector`` with the dots ``dots`` against ``other``."""

    _STATUSES = STATUSES

    def __init__(self, K, preconditioner, rtol, atol, maxiter, check_every):
        super().__init__(K, preconditioner, rtol, atol, maxiter, check_every)
        self._kind = 2 if self._ml is not None else _kind(self.preconditioner)
        self._code = compile_kernels(K.gdim, self._kind)

    def _workspace(self, dev: int):
        """(control, r, rhat, p, v, t, y, z, inv)"""
        w = self._work.get(dev)
        if w is None:
            import torch

            d = torch.device("cuda", dev)

            def vector():
                return torch.zeros(self.n, dtype=torch.float64, device=d)

            r, rhat, p, v, t = (vector() for _ in range(5))
            y, z = (vector(), vector()) if self._kind else (p, r)  # without a preconditioner y is p and z is s, which lies over r
            inv = torch.zeros(self.K.gdim**2 * self.K.n_nodes if self._kind == 1 else 2, dtype=torch.float64, device=d)
            w = self._work[dev] = (_Control(dev, self._op.nseg), r, rhat, p, v, t, y, z, inv)
        return w

    def _start(self, dev: int, values, b, x, has_x0: bool, work):
        control, r, rhat, p, v, t, y, z, inv = work
        code, ml, n, name = self._code, self._ml, self.n, self._name
        a = Params()
        a.cg = self._op.args(dev, values, control)
        a.cg.b, a.cg.x, a.cg.r, a.cg.z, a.cg.p, a.cg.inv = (w.data_ptr() for w in (b, x, r, z, p, inv))
        a.rhat, a.v, a.t, a.y = (w.data_ptr() for w in (rhat, v, t, y))
        a.cg.has_x0 = 1 if has_x0 else 0
        cap, blocks = BLOCKS_PER_CU * jit.num_cu(dev), self._op.blocks(dev)
        self._inverses(dev, values, a.cg, control)
        a.cg.q = v.data_ptr()
        if has_x0:
            self._first_product(dev, values, a, x, v)
        jit.launch(code, dev, blocks, a, f"{name} start launch", kernel=START_KERNEL)
        direction_blocks = max(1, min(-(-n // _CHUNK) if self._kind == 1 else -(-(n // 2) // 256), cap))
        product = self._products(dev, values, a, control)
        half, full, direction = f"{name} half-step launch", f"{name} full-step launch", f"{name} direction launch"

        def iterate():
            if ml is not None:
                ml._cycle(dev, values, control, p.data_ptr(), y.data_ptr())
            product(y, v, rhat, _DOT_V)
            jit.launch(code, dev, blocks, a, half, kernel=HALF_KERNEL)
            if ml is not None:
                ml._cycle(dev, values, control, r.data_ptr(), z.data_ptr())
            product(z, t, r, _DOT_T)
            jit.launch(code, dev, blocks, a, full, kernel=FULL_KERNEL)
            jit.launch(code, dev, direction_blocks, a, direction, kernel=DIRECTION_KERNEL)

        return iterate


class BiCGStab(_BiCGStab):
    """``solver(values, b, x0=None, out=None) -> SolveResult``: ``K x = b`` by right-preconditioned BiCGStab on the GPU, for a ``K``
    that need not be symmetric.

    The arguments are ``ConjugateGradient``'s: ``K`` the ``TangentMatrix`` whose values array is solved with, in either format;
    ``preconditioner``: "block_jacobi", ``None``, "multilevel" or a ``MultilevelPreconditioner`` built for the same ``K`` (its cycle is
    applied twice per iteration; its Galerkin values and inverses are formed at every call).  The iteration stops at
    ``r . r <= max(rtol^2 b . b, atol^2)`` (the recurrence's residual, after the half or the full step) or after ``maxiter`` iterations
    (default ``10 D n_nodes``; an iteration costs two products); ``check_every``: iterations enqueued between two looks at the status
    (the result does not depend on it).  ``SolveResult.status`` is one of ``STATUSES[1:]``: "breakdown" says that ``rhat . r``,
    ``rhat . v``, ``t . t`` or ``omega`` came out zero or not finite -- ``x`` is the last iterate; a stronger preconditioner (a multilevel
    cycle) is the remedy on large, strongly unsymmetric systems.

    Validation, the tensors, the stream and the synchronisation at the end of a call are as for ``ConjugateGradient``: everything is
    checked on the host before anything is uploaded or launched; THE CALL IS SYNCHRONOUS AT ITS END (and at every look before)."""

    def __init__(self, K: TangentMatrix, preconditioner="block_jacobi", rtol: float = 1e-8, atol: float = 0.0, maxiter: int | None = None,
                 check_every: int = 16):
        if not isinstance(K, TangentMatrix):
            raise TypeError(f"K must be a TangentMatrix, got {type(K).__name__}")
        super().__init__(K, preconditioner, rtol, atol, maxiter, check_every)

    @property
    def resources(self) -> dict:
        """``{"vgprs", "sgprs", "scratch_bytes", "lds_bytes", "waves_per_simd", ...}`` of the product kernel, under "start", "half",
        "full", "direction", "matvec" and "inverse" those of the other kernels (compiler remarks), under "slab" the doubles per slab"""
        r = kernel_resources(self._code.log, PRODUCT_KERNEL)
        for name, kernel in (("start", START_KERNEL), ("half", HALF_KERNEL), ("full", FULL_KERNEL), ("direction", DIRECTION_KERNEL),
                             ("matvec", solver.MATVEC_KERNEL), ("inverse", solver.INVERSE_KERNEL)):
            r[name] = kernel_resources(self._code.log, kernel)
        r["slab"] = SLAB
        return r

    def lds_bytes(self, kernel: str = PRODUCT_KERNEL) -> int:
        return lds_bytes(kernel, self._kind)

    def _first_product(self, dev: int, values, a: Params, x, v) -> None:
        """``K x0`` into ``v`` (``a.cg.q``), by the conjugate gradients' product"""
        a.cg.va, a.cg.mode = x.data_ptr(), solver._MODE_PLAIN
        jit.launch(self._code, dev, self._op.blocks(dev), a.cg, "BiCGStab matrix-vector launch", kernel=solver.MATVEC_KERNEL)

    def _products(self, dev: int, values, a: Params, control):
        code, blocks = self._code, self._op.blocks(dev)

        def product(vector, result, other, dots):
            a.cg.va, a.cg.q, a.cg.vb, a.cg.mode = vector.data_ptr(), result.data_ptr(), other.data_ptr(), dots
            jit.launch(code, dev, blocks, a, "BiCGStab product launch", kernel=PRODUCT_KERNEL)

        return product
