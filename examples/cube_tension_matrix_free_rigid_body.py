#!/usr/bin/env python3
"""The partly yielding cube of cube_tension_matrix_free_multilevel.py with the rigid-body modes in the coarse space: no matrix AND the
iteration counts of cube_tension_rigid_body.py.

The loop is ``matrix_free_multilevel_loop`` of cube_tension_matrix_free_multilevel.py as it is; the preconditioner is
``fc.MultilevelPreconditioner(A, cycle=..., coarse_space="rigid_body", coordinates=mesh.nodes)`` with ``A = fc.TangentOperator(force)``.
The aggregates rotate too: the nodes of the coarse levels carry six dofs, the first coarse level is gathered from the element
matrices as ``P_i^T ke P_j`` with the nodes' offsets from their aggregates' positions, and no ``TangentMatrix`` is ever constructed.
Printed: the Newton counts and the conjugate-gradient iterations of every solve under both cycles next to the translations' on
the same operator.

    python examples/cube_tension_matrix_free_rigid_body.py [cells per edge]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_test_device_solve  # noqa: E402
from cube_tension_matrix_free import CG_RTOL  # noqa: E402
from cube_tension_matrix_free_multilevel import VM_P, matrix_free_multilevel_loop  # noqa: E402


def matrix_free_rigid_body_loop(mesh, law, cycle="multiplicative", rtol=CG_RTOL, scratch_bytes=None, **options):
    """``matrix_free_multilevel_loop`` of ``mesh`` and ``law`` with the rigid-body coarse space placed at the mesh's nodes
    (``options``: the other arguments of the preconditioner)"""
    return matrix_free_multilevel_loop(mesh, law, cycle, rtol=rtol, scratch_bytes=scratch_bytes, coarse_space="rigid_body", coordinates=mesh.nodes, **options)


def main():
    import fenics_constitutive_amd as fc

    m = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    mesh = FE.Cube(m, m, m)
    for cycle in ("additive", "multiplicative"):
        runs = {}
        for space in ("translations", "rigid_body"):
            loop = (matrix_free_multilevel_loop if space == "translations" else matrix_free_rigid_body_loop)(mesh, fc.VonMises3D(VM_P), cycle)
            reactions, norms, u, solves = tension_test_device_solve(mesh, loop, steps=8)
            runs[space] = (reactions, [len(h) for h in norms], solves)
            pc = loop.cg.preconditioner
            print(f"{cycle:>14} {space:>12}: Newton iterations {runs[space][1]}, conjugate-gradient iterations per solve {solves} (sum {sum(solves)}), "
                  f"levels {[lv['nodes'] for lv in pc.levels]} of {pc.coarse_dofs} dofs per coarse node")
            assert pc.coarse_space == space and not any(isinstance(x, fc.TangentMatrix) for x in vars(loop).values())  # no matrix anywhere in the loop
        plain, rigid = runs["translations"], runs["rigid_body"]
        difference = np.max(np.abs(rigid[0] - plain[0])) / np.max(np.abs(plain[0]))
        print(f"{cycle:>14}: largest relative reaction difference to the translations {difference:.2e}, "
              f"{sum(rigid[2]) / sum(plain[2]):.2f} of their conjugate-gradient iterations")
        assert difference <= 1e-8 and rigid[1] == plain[1]


if __name__ == "__main__":
    main()
