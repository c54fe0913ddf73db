#!/usr/bin/env python3
"""The tension cube of cube_tension_device_solve.py with a law whose tangent is NOT symmetric, solved on the GPU by BiCGStab.

``DruckerPrager3D`` with ``b != b_flow`` (non-associated flow) gives a consistent tangent that is not symmetric, so the assembled
stiffness is not either, and conjugate gradients are not a solver for it.  The loop is ``DeviceSolveLoop`` as it is -- gradient
producer, resident law, force operator, tangent matrix, all on the device --; only the solver differs: ``fc.BiCGStab(K)``, with
block-Jacobi or a multilevel cycle as preconditioner.  Problem, load path and convergence criterion are those of
``fe_mini.tension_test``; the run of cube_tension_assembled.py (values downloaded, SciPy's direct solver) is the comparison.

The load is applied in ``max(8, 4 m)`` steps for ``m`` cells per edge: the first Newton iterate of a load step puts the whole
increment into the top layer of cells, and the tip of the classic surface must stay out of its reach.

    python examples/cube_tension_nonsymmetric.py [cells per edge] [block_jacobi | multiplicative | additive]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_mini as FE  # noqa: E402
from cube_tension_assembled import AssembledLoop, tension_test_assembled  # noqa: E402
from cube_tension_device_solve import DeviceSolveLoop, tension_test_device_solve  # noqa: E402
from cube_tension_matrix_free import CG_RTOL, cube_operators  # noqa: E402

#: classic Drucker-Prager, f = sqrt(J2) + b I1 - a, flow without dilatancy (b_flow = 0): the surface's tip I1 = a / b = 4000 stays out
#: of reach of the Newton iterates of this load path, and most of the cube yields
DP_P = {"mu": 80769.0, "kappa": 175000.0, "a": 600.0, "b": 0.15, "b_flow": 0.0}
TOP_DISPLACEMENT = 0.005


def drucker_prager():
    import fenics_constitutive_amd as fc

    return fc.DruckerPrager3D({k: np.array([v]) for k, v in DP_P.items()})


def nonsymmetric_loop(mesh, law, preconditioner="block_jacobi", format="bsr", rtol=CG_RTOL, **options):
    """the ``DeviceSolveLoop`` of ``mesh`` and ``law`` with ``fc.BiCGStab`` as its solver; ``preconditioner``: "block_jacobi", ``None`` or a
    cycle of the multilevel preconditioner (``options``: its other arguments)"""
    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd.resident import ResidentState

    op, force = cube_operators(mesh)
    K = fc.TangentMatrix(force, format=format)
    pc = preconditioner if preconditioner in ("block_jacobi", None) else fc.MultilevelPreconditioner(K, cycle=preconditioner, **options)
    return DeviceSolveLoop(ResidentState(law, mesh.n_points, placement="torch"), op, force, K, fc.BiCGStab(K, preconditioner=pc, rtol=rtol))


def main():
    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd.resident import ResidentState

    m = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    pc = sys.argv[2] if len(sys.argv) > 2 else "block_jacobi"
    steps = max(8, 4 * m)
    mesh = FE.Cube(m, m, m)
    loop = nonsymmetric_loop(mesh, drucker_prager(), pc, rtol=1e-12)
    reactions, norms, u, solves = tension_test_device_solve(mesh, loop, steps=steps, top_displacement=TOP_DISPLACEMENT)
    for k, (r, h) in enumerate(zip(reactions, norms), 1):
        print(f"load step {k}: reaction {r:10.3f}   Newton residuals " + "  ".join(f"{x:.2e}" for x in h))
    # the comparison: the values downloaded, SciPy's sparse direct solver on the host
    op2, force2 = cube_operators(mesh)
    K2 = fc.TangentMatrix(force2, format="csr")
    direct = AssembledLoop(ResidentState(drucker_prager(), mesh.n_points, placement="torch"), op2, force2, K2)
    reactions_direct, norms_direct, _, _ = tension_test_assembled(mesh, direct, steps=steps, top_displacement=TOP_DISPLACEMENT, compare_cg=False)
    # how far from symmetric the last assembled stiffness is
    a = loop.K.to_scipy(loop._values)
    asym = float(abs(a - a.T).power(2).sum() ** 0.5 / abs(a).power(2).sum() ** 0.5)
    difference = np.max(np.abs(reactions - reactions_direct)) / np.max(np.abs(reactions_direct))
    print(f"{mesh.n_points} quadrature points, {mesh.n_dofs} dofs: Newton iterations {[len(h) for h in norms]} (direct solve of the downloaded matrix: "
          f"{[len(h) for h in norms_direct]}); {len(solves)} solves on the device with {min(solves)} .. {max(solves)} BiCGStab iterations each "
          f"({pc}): {solves}")
    print(f"|K - K^T| / |K| of the last stiffness {asym:.3f}; largest relative reaction difference to the direct solve {difference:.2e}")
    # (a load step whose last Newton residual lies at the tolerance may take one iteration more or less behind an iterative solve)
    assert difference <= 1e-8 and all(abs(len(h) - len(g)) <= 1 for h, g in zip(norms, norms_direct))


if __name__ == "__main__":
    main()
