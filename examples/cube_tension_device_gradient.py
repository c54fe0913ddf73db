#!/usr/bin/env python3
"""The partly yielding cube of cube_tension_fe.py with the displacement gradient formed on the GPU: per Newton iteration the
host sends the nodal increment u - u_prev (3 doubles per node) instead of the gradient (9 doubles per quadrature point),
``DisplacementGradient`` turns it into ``grad_del_u`` on the device and ``ResidentState.evaluate_into`` reads that tensor where
it is.  Prints the Newton residuals of every load step and compares the reactions with the host-gradient run.

    python examples/cube_tension_device_gradient.py [cells per edge]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_mini as FE  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd.gradient import hex8_reference_gradients, inverse_jacobians  # noqa: E402
from fenics_constitutive_amd.resident import ResidentState  # noqa: E402


class IncrementMesh:
    """the Cube with ``gradient`` handing the nodal increment on unchanged: the state below applies the operator on the GPU"""

    def __init__(self, mesh):
        self._mesh = mesh

    def __getattr__(self, name):
        return getattr(self._mesh, name)

    def gradient(self, du):
        return du


class DeviceGradientState(FE.ResidentProtocolState):
    def __init__(self, resident_state, n, op):
        super().__init__(resident_state, n)
        self.op = op

    def evaluate(self, t, del_t, du):
        self.rs.evaluate_into(t, del_t, self.op(du), self.stress, self.tangent)


def cube_operator(mesh, layout="grad"):
    """the operator of a fe_mini Cube (fe_mini's own gradient is d u_r / d x_c: layout "grad")"""
    ref = hex8_reference_gradients()
    return fc.DisplacementGradient(np.ascontiguousarray(mesh.cells, dtype=np.int32), ref, inverse_jacobians(mesh.nodes[mesh.cells], ref),
                                   mesh.n_nodes, layout=layout)


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    mesh = FE.Cube(m, m, m)
    params = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
    op = cube_operator(mesh)
    state = DeviceGradientState(ResidentState(fc.VonMises3D(params), mesh.n_points), mesh.n_points, op)
    reactions, norms, u = FE.tension_test(IncrementMesh(mesh), state, steps=8)
    for k, (r, h) in enumerate(zip(reactions, norms), 1):
        print(f"load step {k}: reaction {r:10.3f}   Newton residuals " + "  ".join(f"{x:.2e}" for x in h))
    host = FE.ResidentProtocolState(ResidentState(fc.VonMises3D(params), mesh.n_points), mesh.n_points)
    reactions_host, norms_host, _ = FE.tension_test(mesh, host, steps=8)
    orders = FE.convergence_orders(norms)
    print(f"{mesh.n_points} quadrature points, {mesh.n_dofs} dofs: {8 * mesh.n_dofs} B of increment instead of {72 * mesh.n_points} B of "
          f"gradient per iteration; {sum(len(h) - 1 for h in norms)} Newton iterations, convergence orders {min(orders):.2f} .. {max(orders):.2f}; "
          f"largest reaction difference to the host gradient {np.max(np.abs(reactions - reactions_host)):.2e}")
    assert [len(h) for h in norms] == [len(h) for h in norms_host]
    assert np.max(np.abs(reactions - reactions_host)) <= 1e-8 * np.max(np.abs(reactions_host))
    assert max(orders) >= 1.8


if __name__ == "__main__":
    main()
