#!/usr/bin/env python3
"""The partly yielding cube of cube_tension_multilevel.py with both coarse spaces of the multilevel preconditioner side by side.

The loop is ``DeviceSolveLoop`` as it is; only the preconditioner differs: ``fc.MultilevelPreconditioner(K, cycle=...)`` -- piecewise
constant translations on every aggregate -- against ``fc.MultilevelPreconditioner(K, cycle=..., coarse_space="rigid_body",
coordinates=mesh.nodes)`` -- translations and rotations, ``6 x 6`` coarse blocks.  Printed: the Newton counts and the
conjugate-gradient iterations of every solve, the two coarse spaces next to each other, for both cycles.

    python examples/cube_tension_rigid_body.py [cells per edge]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_test_device_solve  # noqa: E402
from cube_tension_multilevel import VM_P, multilevel_loop  # noqa: E402


def main():
    import fenics_constitutive_amd as fc

    m = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    mesh = FE.Cube(m, m, m)
    for cycle in ("additive", "multiplicative"):
        runs = {}
        for space, options in (("translations", {}), ("rigid_body", {"coarse_space": "rigid_body", "coordinates": mesh.nodes})):
            loop = multilevel_loop(mesh, fc.VonMises3D(VM_P), cycle, **options)
            reactions, norms, u, solves = tension_test_device_solve(mesh, loop, steps=8)
            pc = loop.cg.preconditioner
            runs[space] = (reactions, [len(h) for h in norms], solves)
            print(f"{cycle:>14} {space:>12}: levels {[lv['nodes'] for lv in pc.levels]} with {pc.coarse_dofs} dofs per coarse node, Newton iterations {runs[space][1]}")
        plain, rigid = runs["translations"], runs["rigid_body"]
        print(f"{cycle:>14}: conjugate-gradient iterations per solve, translations | rigid body")
        for k, (a, b) in enumerate(zip(plain[2], rigid[2]), 1):
            print(f"{'':>14}  solve {k:3d}: {a:5d} | {b:5d}")
        difference = np.max(np.abs(rigid[0] - plain[0])) / np.max(np.abs(plain[0]))
        print(f"{cycle:>14}: sum {sum(plain[2])} | {sum(rigid[2])} ({sum(rigid[2]) / sum(plain[2]):.2f}); largest relative reaction difference {difference:.2e}")
        assert difference <= 1e-8 and rigid[1] == plain[1]


if __name__ == "__main__":
    main()
