"""The Newton step of an unsymmetric tangent solved on the GPU WITHOUT a matrix: right-preconditioned BiCGStab on the matrix-free
tangent operator.

``MatrixFreeBiCGStab(A)`` solves ``A x = b`` for a ``TangentOperator`` whose tangent is not symmetric -- Drucker-Prager with
``b != b_flow``, a ``JaumannRate`` around any law, a ``UserLaw`` with a non-associated tangent --: the fourth combination of the two
operators (``TangentMatrix``, ``TangentOperator``) and the two Krylov solvers (``ConjugateGradient``, ``BiCGStab``).  Nothing of the
operator assumes symmetry (``s = C e`` uses the whole ``C``; the diagonal blocks and the first Galerkin step of the multilevel
preconditioner sum full element matrices); what ``BiCGStab`` needs and the operator's own node kernel does not give are its dots:
``rhat . v`` behind the first product of an iteration, ``t . s`` and ``t . t`` behind the second.  ``fc.BiCGStab(A)`` stays a
``TypeError``: this class is the entry point.

*The kernel* (``csrc/jit/bicgstab_free.hip``, a program of its own behind the definitions of ``tangent_operator.program``):
``fcamd_tangent_operator_node_dots_kernel``, the second launch of a product behind the operator's unchanged element kernel.  Layout
and row are the operator's node kernel's -- a block per segment of ``SEG`` dofs, lane ``t`` the dofs ``seg*SEG + t + 256 i``; a
constrained dof: ``y = va[e]``; else ``y = 0.0; y = y + fe[adj[k]*D + r]`` over the node's entries ascending --, which is the lane
order of ``fcamd_bcg_product_kernel``: ``acc = acc + y * vb[e]`` and, for the second product, ``acc2 = acc2 + y * y`` as the rows
complete are the partials of ``solver_util.ordered_dot``, and the trees, the second partial array, the last block and its statements
(``rv``; ``ts``, ``tt``, ``omega = ts / tt``; a zero or non-finite ``rv``, ``tt`` or ``omega``: ``breakdown``) are those of that kernel.  The
second dot adds no pass over memory: ``y`` is in the lane's register.  No floating-point atomics, no MFMA, ``-ffp-contract=off``.

*The solver.*  ``MatrixFreeBiCGStab`` is ``bicgstab._BiCGStab`` (the recurrence of ``bicgstab.py``'s module docstring, its control block
and its start, half-step, full-step and direction kernels of ``bicgstab.compile_kernels(A.gdim, kind)``, unchanged) on the driver and
the operator seam of ``solver.py``, which form block-Jacobi and the multilevel setup as for ``ConjugateGradient(A)``.  This module
adds only the product -- element launch, then node-dots launch -- and ``A x0``, which is the operator's quiet product.  Per iteration
six launches -- element, node-dots, half step, element, node-dots, full step -- and the direction kernel, seven, plus the cycles'.

``product(A, tangent, va, vb, both=False)`` runs the kernel alone.
"""

from __future__ import annotations

import ctypes as C

from . import bicgstab, jit, solver
from .bicgstab import STATUSES
from .force import compile_without_scratch, kernel_resources
from .solver import SEG
from .tangent_operator import ELEMENT_KERNEL, MODE_ITERATE, MODE_QUIET, NodeArgs, TangentOperator

NODE_DOTS_KERNEL = "fcamd_tangent_operator_node_dots_kernel"
#: the dots of a product: ``q . vb`` alone (into ``rv``), or ``q . vb`` and ``q . q`` (into ``ts`` and ``tt``, ``omega = ts / tt``)
DOT_V, DOT_T = 0, 1
#: doubles of the control block the products' last blocks write (fcamd_bcg::Block)
_RV, _TS, _TT, _OMEGA = 6, 11, 12, 14

__all__ = ["MatrixFreeBiCGStab", "NODE_DOTS_KERNEL", "NodeDotsArgs", "STATUSES", "compile_kernels", "product", "program"]


def program(gdim: int, nodes_per_cell: int, points_per_cell: int, affine: bool, slab: int, waves: int) -> str:
    """the program text of one shape (the compile cache is keyed by it): the definitions of ``tangent_operator.program`` before
    ``bicgstab_free.hip``"""
    lines = [f"#define FCAMD_TO_D {int(gdim)}", f"#define FCAMD_TO_A {int(nodes_per_cell)}", f"#define FCAMD_TO_Q {int(points_per_cell)}",
             f"#define FCAMD_TO_AFFINE {1 if affine else 0}", f"#define FCAMD_TO_SLAB {int(slab)}", f"#define FCAMD_TO_WAVES {int(waves)}",
             '#include "bicgstab_free.hip"']
    return "\n".join(lines) + "\n"


def compile_kernels(gdim: int, nodes_per_cell: int, points_per_cell: int, affine: bool, slab: int, waves: int):
    """The code object of one shape (no GPU needed): the node-dots kernel next to the kernels of the files it includes.  ``slab`` and
    ``waves`` are those the operator's own program was compiled with (``A.resources``).  Scratch in the kernel is a ``ValueError``."""
    if gdim not in (1, 2, 3):
        raise ValueError(f"the geometric dimension must be 1, 2 or 3, got {gdim}")
    name = f"bicgstab_free_{gdim}d_{nodes_per_cell}n_{points_per_cell}q"
    return compile_without_scratch(program(gdim, nodes_per_cell, points_per_cell, affine, slab, waves), name, NODE_DOTS_KERNEL, (NODE_DOTS_KERNEL,))


class NodeDotsArgs(C.Structure):
    """ctypes mirror of NodeDotsArgs (bicgstab_free.hip): ``NodeArgs`` and, behind it, the dot vector and the dots"""

    _fields_ = NodeArgs._fields_ + [("vb", C.c_void_p), ("dots", C.c_int32), ("pad2", C.c_int32)]


class _Product:
    """The product of one ``TangentOperator`` with BiCGStab's dots: the code object of its shape and, for ``product``, a control
    block per device.  One per operator, kept on the operator object (``_product``): it lives and dies with it."""

    def __init__(self, A: TangentOperator):
        self.A = A
        self.code = compile_kernels(A.gdim, A.nodes_per_cell, A.points_per_cell, A.op.affine, A._code.slab, A._code.waves)
        self.nseg = -(-A.shape[0] // SEG)
        self._control = {}  # device index -> bicgstab._Control (of the module's ``product``)

    def control(self, dev: int):
        c = self._control.get(dev)
        if c is None:
            c = self._control[dev] = bicgstab._Control(dev, self.nseg)
        return c

    def launch(self, dev: int, tangent_ptr: int, va_ptr: int, q_ptr: int, vb_ptr: int, dots: int, control) -> None:
        """``q = A va`` and the ordered ``q . vb`` (``DOT_V``) or ``q . vb`` and ``q . q`` (``DOT_T``) into ``control``, under its status: the
        operator's element launch as it stands, then the node-dots launch in the place of its node launch"""
        sc, partials = control.device_block.data_ptr(), control.partials.data_ptr()
        *element, node = self.A._launches(dev, tangent_ptr, va_ptr, q_ptr, MODE_ITERATE, partials, sc)
        for code, kernel, blocks, args, what in element:
            jit.launch(code, dev, blocks, args, what, kernel=kernel)
        _, _, blocks, na, _ = node
        a = NodeDotsArgs()
        for name, _ in NodeArgs._fields_:
            setattr(a, name, getattr(na, name))
        a.vb, a.dots = vb_ptr, dots
        jit.launch(self.code, dev, blocks, a, "MatrixFreeBiCGStab node-dots launch", kernel=NODE_DOTS_KERNEL)


def _product(A: TangentOperator) -> _Product:
    p = getattr(A, "_bicgstab_product", None)
    if p is None:
        p = A._bicgstab_product = _Product(A)
    return p


def product(A: TangentOperator, tangent, va, vb, both: bool = False, out=None):
    """``(q, q . vb)`` or, with ``both``, ``(q, q . vb, q . q)``: ``q = A va`` for this tangent by the operator's element kernel and the
    node-dots kernel, the dots in the solver's fixed order (``q`` is ``out`` or a new tensor; ``out`` must alias neither vector).  The
    launches run on a fresh control block -- its status "running" -- and are asynchronous; the call then waits for the scalars.  A zero
    or non-finite ``q . vb`` (``both``: ``q . q`` or their quotient) leaves the status ``breakdown`` in the block; ``q`` is written all the
    same."""
    import torch

    if not isinstance(A, TangentOperator):
        raise TypeError(f"A must be a TangentOperator, got {type(A).__name__}")
    dev, n = A.device, A.shape[0]
    solver._operator(A).check(tangent, dev)
    A._check("va", va, n, dev)
    A._check("vb", vb, n, dev)
    if out is not None:
        A._check("out", out, n, dev)
        if solver._overlap(out, va) or solver._overlap(out, vb):
            raise ValueError("out must not alias va or vb")
    p = _product(A)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=torch.device("cuda", dev))
        if n == 0:
            return (out, 0.0, 0.0) if both else (out, 0.0)
        control = p.control(dev)
        control.upload()
        p.launch(dev, tangent.data_ptr(), va.data_ptr(), out.data_ptr(), vb.data_ptr(), DOT_T if both else DOT_V, control)
        control.download(dev, bicgstab._SCALARS)
    h = control.host
    return (out, float(h[_TS]), float(h[_TT])) if both else (out, float(h[_RV]))


class MatrixFreeBiCGStab(bicgstab._BiCGStab):
    """``solver(tangent, b, x0=None, out=None) -> SolveResult``: ``A x = b`` by right-preconditioned BiCGStab on the GPU, ``A`` a
    ``TangentOperator`` whose tangent need not be symmetric and no matrix anywhere.

    ``A``: the ``TangentOperator`` (anything else, a ``TangentMatrix`` included, is a ``TypeError``: that is ``BiCGStab``'s).
    ``preconditioner``: "block_jacobi" -- the inverses of the nodes' own blocks, formed from the tangent at every call --, ``None``, or
    a ``MultilevelPreconditioner`` built on this very operator (its cycle is applied twice per iteration; the string "multilevel" and
    an instance built on another object are a ``ValueError``, as for ``ConjugateGradient(A)``).  ``rtol``, ``atol``, ``maxiter`` (default
    ``10 D n_nodes``; an iteration costs two products), ``check_every``, the statuses (``STATUSES[1:]``, "breakdown" among them) and
    ``SolveResult`` are ``BiCGStab``'s.  A node that belongs to no cell is refused at construction.

    ``tangent`` is the ``S*S n_points`` array a law wrote, ``b``, ``x0`` and ``out`` float64 device tensors of ``D n_nodes`` entries; ``out``
    may be ``x0`` itself, never ``b``.  Everything is validated on the host before anything is uploaded or launched; the kernels are
    compiled at construction (no GPU needed); THE CALL IS SYNCHRONOUS AT ITS END (and at every look before)."""

    def __init__(self, A: TangentOperator, preconditioner="block_jacobi", rtol: float = 1e-8, atol: float = 0.0, maxiter: int | None = None,
                 check_every: int = 16):
        if not isinstance(A, TangentOperator):
            raise TypeError(f"A must be a TangentOperator, got {type(A).__name__}")
        super().__init__(A, preconditioner, rtol, atol, maxiter, check_every)
        self.A = A
        self._product = _product(A)

    @property
    def resources(self) -> dict:
        """``{"vgprs", "sgprs", "scratch_bytes", "lds_bytes", "waves_per_simd", ...}`` of the node-dots kernel, the same under
        "node_dots", under "element" those of the operator's element kernel (the product's first launch) and under "start", "half",
        "full", "direction" and "inverse" those of the kernels of ``bicgstab.compile_kernels`` (compiler remarks)"""
        r = kernel_resources(self._product.code.log, NODE_DOTS_KERNEL)
        r["node_dots"] = kernel_resources(self._product.code.log, NODE_DOTS_KERNEL)
        r["element"] = kernel_resources(self.A.compile_log, ELEMENT_KERNEL)
        for name, kernel in (("start", bicgstab.START_KERNEL), ("half", bicgstab.HALF_KERNEL), ("full", bicgstab.FULL_KERNEL),
                             ("direction", bicgstab.DIRECTION_KERNEL), ("inverse", solver.INVERSE_KERNEL)):
            r[name] = kernel_resources(self._code.log, kernel)
        return r

    @property
    def compile_log(self) -> str:
        """hiprtc's log of the node-dots program, then that of the program of ``bicgstab.compile_kernels``"""
        return self._product.code.log + self._code.log

    def lds_bytes(self, kernel: str = NODE_DOTS_KERNEL) -> int:
        """LDS of one block of ``kernel``: the tree of the dots and the last-block flag in the node-dots kernel; else as on ``BiCGStab``"""
        if kernel == NODE_DOTS_KERNEL:
            return 8 * (256 + 2)
        return bicgstab.lds_bytes(kernel, self._kind)

    def _first_product(self, dev: int, tangent, a, x, v) -> None:
        """``A x0`` into ``v``, by the operator's quiet product"""
        self.A._apply(dev, tangent.data_ptr(), x.data_ptr(), v.data_ptr(), MODE_QUIET)

    def _products(self, dev: int, tangent, a, control):
        launch, tangent_ptr = self._product.launch, tangent.data_ptr()

        def product(vector, result, other, dots):
            launch(dev, tangent_ptr, vector.data_ptr(), result.data_ptr(), other.data_ptr(), dots, control)

        return product
