#!/usr/bin/env python3
"""The tension cube of cube_tension_nonsymmetric.py -- a law whose tangent is NOT symmetric -- solved on the GPU without a matrix.

``DruckerPrager3D`` with ``b != b_flow`` (non-associated flow) gives a consistent tangent that is not symmetric: conjugate gradients
are not a solver for the Newton step, and ``fc.BiCGStab`` wants the assembled ``TangentMatrix``.  Here the loop is
``MatrixFreeSolveLoop`` of cube_tension_matrix_free_solve.py as it is -- gradient producer, resident law and force operator on the
device, ``fc.TangentOperator`` where the matrix was --; only the solver differs: ``fc.MatrixFreeBiCGStab(A)``, with block-Jacobi from
the nodes' own blocks of the tangent or with a cycle of ``fc.MultilevelPreconditioner(A)``.  No ``TangentMatrix`` is ever constructed:
neither its values array nor its assembly scratch is allocated.  Problem, load path and convergence criterion are those of
``fe_mini.tension_test``; the direct solve on the host is the comparison.

The load is applied in ``max(8, 4 m)`` steps for ``m`` cells per edge, as in cube_tension_nonsymmetric.py.

    python examples/cube_tension_matrix_free_nonsymmetric.py [cells per edge]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_test_device_solve  # noqa: E402
from cube_tension_matrix_free import CG_RTOL, cube_operators  # noqa: E402
from cube_tension_matrix_free_solve import MatrixFreeSolveLoop, bytes_not_allocated  # noqa: E402
from cube_tension_nonsymmetric import TOP_DISPLACEMENT, drucker_prager  # noqa: E402


class MatrixFreeNonsymmetricLoop(MatrixFreeSolveLoop):
    """``MatrixFreeSolveLoop`` of ``mesh`` and ``law`` with ``fc.MatrixFreeBiCGStab`` as its solver.  ``preconditioner``: "block_jacobi",
    ``None`` or a cycle of the multilevel preconditioner of the operator (``options``: its other arguments)"""

    def __init__(self, mesh, law, preconditioner="block_jacobi", rtol=CG_RTOL, scratch_bytes=None, **options):
        import fenics_constitutive_amd as fc
        from fenics_constitutive_amd.resident import ResidentState

        op, force = cube_operators(mesh)
        A = fc.TangentOperator(force, scratch_bytes=scratch_bytes)
        pc = preconditioner if preconditioner in ("block_jacobi", None) else fc.MultilevelPreconditioner(A, cycle=preconditioner, **options)
        super().__init__(ResidentState(law, mesh.n_points, placement="torch"), op, force, A, fc.MatrixFreeBiCGStab(A, preconditioner=pc, rtol=rtol))


def main():
    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd.resident import ResidentState

    m = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    steps = max(8, 4 * m)
    mesh = FE.Cube(m, m, m)
    host = FE.ResidentProtocolState(ResidentState(drucker_prager(), mesh.n_points), mesh.n_points)
    with np.errstate(all="ignore"):
        reactions_direct, norms_direct, _ = FE.tension_test(mesh, host, steps=steps, top_displacement=TOP_DISPLACEMENT)
    for pc in ("block_jacobi", "additive"):
        loop = MatrixFreeNonsymmetricLoop(mesh, drucker_prager(), pc, rtol=1e-12)
        reactions, norms, u, solves = tension_test_device_solve(mesh, loop, steps=steps, top_displacement=TOP_DISPLACEMENT)
        assert not any(isinstance(x, fc.TangentMatrix) for x in vars(loop).values())  # no matrix anywhere in the loop
        difference = np.max(np.abs(reactions - reactions_direct)) / np.max(np.abs(reactions_direct))
        levels = "" if pc == "block_jacobi" else f", levels {[lv['nodes'] for lv in loop.cg.preconditioner.levels]}"
        print(f"{pc:>14}: Newton iterations {[len(h) for h in norms]} (direct solve on the host: {[len(h) for h in norms_direct]}); "
              f"{len(solves)} solves on the device with {min(solves)} .. {max(solves)} BiCGStab iterations each (sum {sum(solves)}){levels}; "
              f"largest relative reaction difference to the direct solve {difference:.2e}")
        # (a load step whose last Newton residual lies at the tolerance may take one iteration more or less behind an iterative solve)
        assert difference <= 1e-8 and all(abs(len(h) - len(g)) <= 1 for h, g in zip(norms, norms_direct))
    values, scratch, ours = bytes_not_allocated(mesh)
    print(f"{mesh.n_points} quadrature points, {mesh.n_dofs} dofs, no matrix: device bytes this loop does not allocate: {values / 1e6:.2f} MB of values "
          f"and {scratch / 1e6:.2f} MB of assembly scratch (block-Jacobi takes {ours / 1e6:.2f} MB for the nodes' own blocks and their scratch instead)")


if __name__ == "__main__":
    main()
