"""What the finite-element operators share on the host: ``DisplacementGradient``, ``InternalForce``, ``TangentMatrix``,
``TangentOperator`` and the operator side of the multilevel preconditioner.  No kernel, no program text and
no argument structure lives here; each module keeps its own and states its own rules in its docstring.

* ``check_tensor``: the check of a device tensor argument;  ``overlap``, ``even``.
* ``per_device``, ``upload``, ``doubles``: one upload (or allocation) per device, kept in a dict the owner names (``_on``, ``_fe``,
  ``_scratch``, ...), empty until the first use.
* ``ConstraintMask``: ``set_constrained`` and ``_mask_table`` of an object with ``shape``, ``gdim`` and ``_mask_on``.
* ``compile_ladder``: the register-budget ladder of the three programs with several kernels; the caller says which kernels must be
  free of scratch, its register test and what exhaustion raises.  ``kernel_resources``, ``vector_registers``: one kernel's remarks.
* ``ChunkedPass``: a bounded scratch of whole tiles of cells and the walk over its chunks.
* ``launch_cap``, ``blocks_for``, ``tile_blocks``: the grid of a launch.  None of them clamps at one block: a site that launches at
  least one block says ``max(1, ...)`` itself.

``jit.launch``, ``jit.num_cu`` and ``jit.compile_program`` are looked up on ``jit`` at the call, as the tests that patch them need.
"""

from __future__ import annotations

import re

import numpy as np

from . import jit
from .device import _is_torch

#: register budgets (waves per SIMD) tried in order
WAVES_LADDER = (8, 4, 2)
#: blocks per compute unit the grid is capped at (the waves loop over the remaining tiles)
BLOCKS_PER_CU = 16
#: bytes of element matrices between two kernels unless the caller says otherwise: 256 MiB, 466 033 hexahedra of 576 doubles
SCRATCH_BYTES = 256 * 1024 * 1024


# ---- small helpers ---------------------------------------------------------------------------------------------------------------
def check_tensor(name: str, a, numel: int, dev: int) -> None:
    """``a`` is a contiguous float64 tensor of ``numel`` entries on ``cuda:dev``, on the 16-byte grid (``TypeError`` / ``ValueError``)"""
    import torch

    if not _is_torch(a):
        raise TypeError(f"{name} must be a torch CUDA tensor, got {type(a).__name__}")
    if a.dtype != torch.float64:
        raise TypeError(f"{name} must be float64, got {a.dtype}")
    if not a.is_cuda or (a.device.index or 0) != dev:
        raise ValueError(f"{name} is on {a.device}, the operator on cuda:{dev}")
    if not a.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if a.numel() != numel:
        raise ValueError(f"{name} has {a.numel()} entries, expected {numel}")
    if a.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned")


def overlap(a, b) -> bool:
    """two float64 tensors share memory"""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + 8 * b.numel() and b0 < a0 + 8 * a.numel()


def even(n: int) -> int:
    return (n + 1) // 2 * 2


# ---- one upload per device -------------------------------------------------------------------------------------------------------
def per_device(cache: dict, dev: int, make):
    """``cache[dev]``, made at the first use by ``make(torch device)`` with that device current"""
    t = cache.get(dev)
    if t is None:
        import torch

        d = torch.device("cuda", dev)
        with torch.cuda.device(d):
            t = cache[dev] = make(d)
    return t


def upload(d, *arrays) -> tuple:
    """the host arrays as device tensors"""
    from .hostio import to_device

    return tuple(to_device(x, d) for x in arrays)


def doubles(n: int, d):
    """an uninitialised float64 tensor of ``n`` entries"""
    import torch

    return torch.empty(n, dtype=torch.float64, device=d)


# ---- constraints -----------------------------------------------------------------------------------------------------------------
class ConstraintMask:
    """``set_constrained`` and ``_mask_table`` of a matrix or an operator with ``shape``, ``gdim`` and ``_mask_on = {}`` (device index
    -> (version, mask tensor)).  The class says which nodes have no block of their own -- ``_without_own_block(nodes)``, a bool per
    node -- and, in ``_no_own_block``, how the refusal of a constrained dof there ends."""

    _mask = None
    _mask_version = 0

    def set_constrained(self, mask) -> None:
        """``mask``: bool ``[D n_nodes]``, true at the Dirichlet dofs, or ``None``.  Uploaded at the next call, and again only when
        it changes.  A constrained dof whose node has no block of its own (no diagonal block in a matrix's pattern, no cell in an
        operator's mesh) is a ``ValueError``"""
        if mask is None:
            if self._mask is not None:
                self._mask, self._mask_version = None, self._mask_version + 1
            return
        if not isinstance(mask, np.ndarray):
            raise TypeError(f"mask must be a numpy.ndarray or None, got {type(mask).__name__}")
        if mask.dtype != np.bool_:
            raise TypeError(f"mask must be bool, got {mask.dtype}")
        if mask.shape != (self.shape[0],):
            raise ValueError(f"mask must have shape {(self.shape[0],)} (one entry per dof), got {mask.shape}")
        nodes = np.flatnonzero(mask) // self.gdim
        missing = nodes[self._without_own_block(nodes)]
        if missing.size:
            raise ValueError(f"node {int(missing[0])} has a constrained dof and {self._no_own_block}")
        if self._mask is None or not np.array_equal(self._mask, mask):
            self._mask, self._mask_version = np.ascontiguousarray(mask).copy(), self._mask_version + 1

    def _mask_table(self, dev: int):
        """the mask on the device as bytes (``None`` without one): one upload per device and version"""
        if self._mask is None:
            return None
        have = self._mask_on.get(dev)
        if have is None or have[0] != self._mask_version:
            import torch

            d = torch.device("cuda", dev)
            with torch.cuda.device(d):
                have = self._mask_on[dev] = (self._mask_version, upload(d, self._mask.view(np.uint8))[0])
        return have[1]


# ---- the register-budget ladder --------------------------------------------------------------------------------------------------
def kernel_resources(log: str, kernel: str) -> dict:
    """``jit.parse_resources`` of the remarks of ONE kernel of a program that holds several"""
    parts = re.split(r"(?=Function Name: )", log)
    for part in parts:
        if part.startswith(f"Function Name: {kernel}"):
            return jit.parse_resources(part)
    raise RuntimeError(f"no resource remarks for {kernel} in the compile log")


def vector_registers(log: str, kernel: str) -> int:
    """VGPRs and AGPRs of one kernel of a program: what a wave of it takes of the SIMD's 512 vector registers per lane"""
    res = kernel_resources(log, kernel)
    return res["vgprs"] + (res["agprs"] or 0)


def compile_ladder(make_program, name: str, entry: str, waves, kernels, accept, exhausted, keep_overrun: bool = False, **note):
    """The code object of ``make_program(w)`` for the first budget ``w`` of ``WAVES_LADDER`` at which none of ``kernels`` has scratch
    and ``accept(log, w)``, the caller's register test, holds.  ``code.waves`` is the budget and ``note`` (``slab=...``) is set on every
    code object compiled; an explicit ``waves`` is compiled and returned unchecked.  ``keep_overrun``: when no budget passes, the
    first one without scratch is returned.  Otherwise ``exhausted(scratch bytes of ``kernels`` at the last budget)`` is raised."""
    fallback = spilled = None
    for w in WAVES_LADDER if waves is None else (waves,):
        code = jit.compile_program(make_program(w), name, entry)
        code.waves = w
        vars(code).update(note)
        if waves is not None:
            return code
        spilled = [kernel_resources(code.log, k)["scratch_bytes"] for k in kernels]
        if any(spilled):
            continue
        if accept(code.log, w):
            return code
        if keep_overrun and fallback is None:
            fallback = code
    if fallback is not None:
        return fallback
    raise exhausted(spilled)


# ---- the grid of a launch --------------------------------------------------------------------------------------------------------
def launch_cap(dev: int) -> int:
    """the most blocks of a grid: ``num_cu`` is looked up on ``jit`` at launch"""
    return BLOCKS_PER_CU * jit.num_cu(dev)


def blocks_for(n_lanes: int, cap: int) -> int:
    """a lane per entry, 256 lanes per block (0 for nothing)"""
    return min((n_lanes + 255) // 256, cap)


def tile_blocks(tiles: int, cap: int) -> int:
    """a wave per tile, 4 waves per block (0 for nothing)"""
    return min((tiles + 3) // 4, cap)


# ---- the chunked element pass ----------------------------------------------------------------------------------------------------
class ChunkedPass:
    """An element kernel whose per-cell results pass through a bounded scratch to a consumer kernel on the same stream: the cells
    of ``force``'s mesh in ascending chunks of whole tiles, ``chunk_cells = scratch_bytes // bytes_per_cell // cells_per_tile *
    cells_per_tile``.  ``scratch_bytes``: ``None`` for ``SCRATCH_BYTES``, not an integer: ``TypeError``, less than one tile:
    ``ValueError(too_small(scratch_bytes, bytes of a tile))``.  The scratch tensor belongs to whoever launches the kernels: ``buffer``
    sizes it into the owner's own dict."""

    def __init__(self, force, scratch_bytes, bytes_per_cell: int, cells_per_tile: int, too_small):
        if scratch_bytes is None:
            scratch_bytes = SCRATCH_BYTES
        if isinstance(scratch_bytes, bool) or not isinstance(scratch_bytes, (int, np.integer)):
            raise TypeError(f"scratch_bytes must be an integer, got {type(scratch_bytes).__name__}")
        if scratch_bytes < cells_per_tile * bytes_per_cell:
            raise ValueError(too_small(scratch_bytes, cells_per_tile * bytes_per_cell))
        op = force.op
        self.force, self.n_cells = force, op.n_cells
        self.scratch_bytes, self.bytes_per_cell, self.cells_per_tile = int(scratch_bytes), bytes_per_cell, cells_per_tile
        self.chunk_cells = int(scratch_bytes) // bytes_per_cell // cells_per_tile * cells_per_tile  # whole tiles
        q = op.points_per_cell
        #: bytes of a cell in the tangent, the inverse Jacobians and the weights
        self.strides = (8 * force.stress_dim**2 * q, 8 * op.gdim**2 * (1 if op.affine else q), 8 * q)

    def chunks(self) -> list:
        """the ascending cell ranges ``(first, end)`` that run one after the other"""
        return [(c, min(c + self.chunk_cells, self.n_cells)) for c in range(0, self.n_cells, self.chunk_cells)]

    def block_ranges(self, contributions: np.ndarray, blk_ptr: np.ndarray, nnzb: int, pairs: int) -> list:
        """``(first, end)`` per chunk: the range of blocks its cells touch, a later chunk's consumer runs over it alone.
        ``contributions`` / ``blk_ptr``: ``matrix.contribution_lists`` of ``nnzb`` blocks, ``pairs = A*A`` contributions per cell"""
        if not (self.n_cells and nnzb):
            return []
        block_of = np.empty(contributions.size, dtype=np.int32)  # by c*A*A + a*A + b
        block_of[contributions] = np.repeat(np.arange(nnzb, dtype=np.int32), np.diff(blk_ptr))
        starts = np.arange(0, self.n_cells, self.chunk_cells, dtype=np.int64) * pairs
        return list(zip(np.minimum.reduceat(block_of, starts).tolist(), (np.maximum.reduceat(block_of, starts) + 1).tolist()))

    def buffer(self, cache: dict, dev: int):
        """the scratch of a chunk on ``dev``, made once into the owner's ``cache`` (device index -> tensor)"""
        t = cache.get(dev)
        return t if t is not None else per_device(cache, dev, lambda d: doubles(min(self.chunk_cells, self.n_cells) * self.bytes_per_cell // 8, d))

    def walk(self, dev: int, tangent, cap: int):
        """``(k, c0, c1, tangent_ptr, jinv_ptr, weights_ptr, element_blocks)`` of every chunk: its number and cells, where its
        cells start in ``tangent``, in the inverse Jacobians and in the weights, and the grid of its element launch"""
        t0, j0, w0 = tangent.data_ptr(), self.force.op._tables(dev)[2].data_ptr(), self.force._tables(dev)[0].data_ptr()
        ts, js, ws = self.strides
        for k, (c0, c1) in enumerate(self.chunks()):
            yield k, c0, c1, t0 + ts * c0, j0 + js * c0, w0 + ws * c0, tile_blocks(-(-(c1 - c0) // self.cells_per_tile), cap)
