#!/usr/bin/env python3
"""The partly yielding cube of cube_tension_device_solve.py solved on the GPU without a matrix.

The loop is that of cube_tension_device_solve.py -- ``DisplacementGradient``, ``ResidentState.evaluate`` and ``InternalForce`` on the
device, ``fc.ConjugateGradient`` solving ``K dx = f`` there -- with ``fc.TangentOperator`` in the matrix's place: the product of every
iteration is formed from the tangent that sits in HBM anyway, the block-Jacobi preconditioner from the nodes' own blocks of the
same tangent, and no ``TangentMatrix`` is ever constructed: neither its values array nor its assembly scratch is allocated.
Problem, load path and convergence criterion are those of ``fe_mini.tension_test``; the direct solve on the host is the comparison.
Prints the Newton counts, the conjugate-gradient iterations of every solve and the device bytes the loop does not allocate.

    python examples/cube_tension_matrix_free_solve.py [cells per edge]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import DeviceSolveLoop, tension_test_device_solve  # noqa: E402
from cube_tension_matrix_free import CG_RTOL, DeviceLoop, cube_operators  # noqa: E402


class MatrixFreeSolveLoop(DeviceSolveLoop):
    """``DeviceSolveLoop`` with a ``TangentOperator`` where the matrix was: ``constrain`` and ``residual_norms`` are inherited, ``solve``
    hands the tangent itself to the conjugate gradients"""

    def __init__(self, resident_state, op, force, operator, cg):
        import torch

        DeviceLoop.__init__(self, resident_state, op, force)  # (no values array: AssembledLoop's is what this loop does without)
        self.K, self.cg = operator, cg
        self.solves = 0
        self._dx = torch.empty_like(self._f)
        self._zero = torch.zeros((), dtype=torch.float64, device=self._f.device)

    def solve(self):
        import torch

        self.solves += 1
        result = self.cg(self.rs.tangent, torch.where(self._mask, self._zero, self._f), out=self._dx)
        self.bytes_up += 96  # the control block, once per solve
        self.bytes_down += 32 * result.looks  # status, count and the two norms, at every look
        return self._down(result.x), result


def bytes_not_allocated(mesh, scratch_bytes=None):
    """(values, assembly scratch, diagonal blocks and their scratch): the device bytes of a ``TangentMatrix`` of the mesh in block CSR,
    counted from the pattern alone, and what the operator's block-Jacobi takes instead"""
    from fenics_constitutive_amd import matrix

    cells = np.ascontiguousarray(mesh.cells, dtype=np.int32)
    indptr, indices = matrix.block_pattern(cells, mesh.n_nodes)
    cap = matrix.SCRATCH_BYTES if scratch_bytes is None else scratch_bytes
    values = 8 * 9 * int(indices.size)
    scratch = min(cap, 8 * 24 * 24 * mesh.n_cells)
    ours = 8 * 9 * mesh.n_nodes + min(cap, 8 * 8 * 9 * mesh.n_cells)
    return values, scratch, ours


def main():
    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd.resident import ResidentState

    m = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    mesh = FE.Cube(m, m, m)
    params = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
    op, force = cube_operators(mesh)
    A = fc.TangentOperator(force)
    cg = fc.ConjugateGradient(A, preconditioner="block_jacobi", rtol=CG_RTOL)
    loop = MatrixFreeSolveLoop(ResidentState(fc.VonMises3D(params), mesh.n_points, placement="torch"), op, force, A, cg)
    reactions, norms, u, solves = tension_test_device_solve(mesh, loop, steps=8)
    for k, (r, h) in enumerate(zip(reactions, norms), 1):
        print(f"load step {k}: reaction {r:10.3f}   Newton residuals " + "  ".join(f"{x:.2e}" for x in h))
    host = FE.ResidentProtocolState(ResidentState(fc.VonMises3D(params), mesh.n_points), mesh.n_points)
    reactions_direct, norms_direct, _ = FE.tension_test(mesh, host, steps=8)
    difference = np.max(np.abs(reactions - reactions_direct)) / np.max(np.abs(reactions_direct))
    values, scratch, ours = bytes_not_allocated(mesh)
    print(f"{mesh.n_points} quadrature points, {mesh.n_dofs} dofs, no matrix: Newton iterations {[len(h) for h in norms]} "
          f"(direct solve on the host: {[len(h) for h in norms_direct]}); {len(solves)} solves on the device with "
          f"{min(solves)} .. {max(solves)} conjugate-gradient iterations each: {solves}")
    print(f"device bytes this loop does not allocate: {values / 1e6:.2f} MB of values and {scratch / 1e6:.2f} MB of assembly scratch "
          f"(it takes {ours / 1e6:.2f} MB for the nodes' own blocks and their scratch instead; the tangent, {288 * mesh.n_points / 1e6:.2f} MB, is in HBM "
          f"either way); largest relative reaction difference to the direct solve {difference:.2e}")
    assert difference <= 1e-8 and [len(h) for h in norms] == [len(h) for h in norms_direct]


if __name__ == "__main__":
    main()
