#!/usr/bin/env python3
"""The partly yielding cube of cube_tension_device_solve.py solved on the GPU without a matrix AND with the multilevel preconditioner.

The loop is ``MatrixFreeSolveLoop`` of cube_tension_matrix_free_solve.py as it is; only the solver differs:
``fc.ConjugateGradient(A, preconditioner=fc.MultilevelPreconditioner(A, cycle=...))`` with ``A = fc.TangentOperator(force)``.  The
hierarchy is built once from the mesh's block pattern; at every solve the first coarse level is gathered from the element matrices
of the tangent that sits in HBM anyway, the nodes' own blocks come from the operator's diagonal kernels, and no ``TangentMatrix``
is ever constructed.  Printed: the Newton counts and the conjugate-gradient iterations of every solve under both cycles next to
block-Jacobi's on the same operator.

    python examples/cube_tension_matrix_free_multilevel.py [cells per edge]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_test_device_solve  # noqa: E402
from cube_tension_matrix_free import CG_RTOL, cube_operators  # noqa: E402
from cube_tension_matrix_free_solve import MatrixFreeSolveLoop  # noqa: E402

VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}


def matrix_free_multilevel_loop(mesh, law, preconditioner="multiplicative", rtol=CG_RTOL, scratch_bytes=None, **options):
    """the ``MatrixFreeSolveLoop`` of ``mesh`` and ``law`` with ``preconditioner``: a cycle of the multilevel preconditioner of the operator
    (``options``: its other arguments) or "block_jacobi" """
    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd.resident import ResidentState

    op, force = cube_operators(mesh)
    A = fc.TangentOperator(force, scratch_bytes=scratch_bytes)
    pc = preconditioner if preconditioner == "block_jacobi" else fc.MultilevelPreconditioner(A, cycle=preconditioner, **options)
    return MatrixFreeSolveLoop(ResidentState(law, mesh.n_points, placement="torch"), op, force, A, fc.ConjugateGradient(A, preconditioner=pc, rtol=rtol))


def main():
    import fenics_constitutive_amd as fc

    m = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    mesh = FE.Cube(m, m, m)
    runs = {}
    for pc in ("block_jacobi", "additive", "multiplicative"):
        loop = matrix_free_multilevel_loop(mesh, fc.VonMises3D(VM_P), pc)
        reactions, norms, u, solves = tension_test_device_solve(mesh, loop, steps=8)
        runs[pc] = (reactions, [len(h) for h in norms], solves)
        levels = "" if pc == "block_jacobi" else f", levels {[lv['nodes'] for lv in loop.cg.preconditioner.levels]}"
        print(f"{pc:>14}: Newton iterations {runs[pc][1]}, conjugate-gradient iterations per solve {solves} (sum {sum(solves)}){levels}")
        assert not any(isinstance(x, fc.TangentMatrix) for x in vars(loop).values())  # no matrix anywhere in the loop
    reference = runs["block_jacobi"]
    for pc in ("additive", "multiplicative"):
        difference = np.max(np.abs(runs[pc][0] - reference[0])) / np.max(np.abs(reference[0]))
        print(f"{pc:>14}: largest relative reaction difference to block-Jacobi {difference:.2e}, "
              f"{sum(runs[pc][2]) / sum(reference[2]):.2f} of its conjugate-gradient iterations")
        assert difference <= 1e-8 and runs[pc][1] == reference[1]


if __name__ == "__main__":
    main()
