#!/usr/bin/env python3
"""The partly yielding cube of cube_tension_fe.py solved matrix-free with stress and tangent never leaving the GPU.

Per Newton iteration the host sends the nodal increment ``u - u_prev``; ``DisplacementGradient`` forms ``grad_del_u`` on the
device, ``ResidentState.evaluate`` runs the law there (no stress or tangent download) and ``InternalForce`` assembles the nodal
internal force, which comes back.  The linear solve is conjugate gradients on a ``LinearOperator`` whose product is
``force.tangent_action(rs.tangent, op(v))`` restricted to the free dofs: a nodal vector up, a nodal vector down.  Problem, load
path and convergence criterion are those of ``fe_mini.tension_test``.  Prints the Newton residuals, the reactions against the
direct-solve run on ndarrays and the bytes that crossed the link per iteration.

    python examples/cube_tension_matrix_free.py [cells per edge]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_mini as FE  # noqa: E402

#: relative residual the conjugate gradients stop at
CG_RTOL = 1e-12


def tension_test_matrix_free(mesh, loop, steps: int = 8, top_displacement: float = 0.0065, tilt: float = 0.6, rtol: float = 1e-10,
                             maxit: int = 12, cg_rtol: float = CG_RTOL):
    """``fe_mini.tension_test`` with the assembly behind ``loop``: ``loop.residual(t, del_t, du)`` evaluates the law at the
    gradient of the nodal increment and returns the nodal internal force, ``loop.tangent_action(v)`` the product of the tangent
    stiffness of that evaluate with a nodal vector, ``loop.commit()`` commits the load step.  Returns the reactions, the Newton
    residual norms and the displacement like ``tension_test``, and the conjugate-gradient iterations of every solve."""
    import scipy.sparse.linalg as spla

    X = mesh.nodes
    top, bottom = np.flatnonzero(X[:, 2] > 1 - 1e-12), np.flatnonzero(X[:, 2] < 1e-12)
    fixed = set((3 * bottom + 2).tolist()) | set((3 * top + 2).tolist())
    origin = int(np.flatnonzero((np.abs(X) < 1e-12).all(axis=1))[0])
    xcorner = int(np.flatnonzero((np.abs(X - [1.0, 0.0, 0.0]) < 1e-12).all(axis=1))[0])
    fixed |= {3 * origin, 3 * origin + 1, 3 * xcorner + 1}
    fixed = np.array(sorted(fixed))
    free = np.setdiff1d(np.arange(mesh.n_dofs), fixed)
    shape = 1.0 + tilt * (X[top, 0] - 0.5)
    u, u_prev = np.zeros(mesh.n_dofs), np.zeros(mesh.n_dofs)
    full = np.zeros(mesh.n_dofs)

    def matvec(x):
        full[free] = x
        return loop.tangent_action(full)[free]

    K = spla.LinearOperator((free.size, free.size), matvec=matvec, dtype=np.float64)
    reactions, histories, solves = [], [], []
    for step in range(1, steps + 1):
        u[3 * top + 2] = top_displacement * step / steps * shape
        norms = []
        for it in range(maxit + 1):
            f = loop.residual(float(step - 1), 1.0, u - u_prev)
            r = f[free]
            norms.append(float(np.linalg.norm(r)))
            if norms[-1] <= rtol * max(np.linalg.norm(f[fixed]), 1.0):
                break
            count = [0]
            dx, info = spla.cg(K, r, rtol=cg_rtol, atol=0.0, maxiter=10 * free.size, callback=lambda _: count.__setitem__(0, count[0] + 1))
            if info != 0:
                raise RuntimeError(f"conjugate gradients of load step {step}, iteration {it} did not converge (info {info})")
            solves.append(count[0])
            u[free] -= dx
        else:
            raise RuntimeError(f"Newton iteration of load step {step} did not converge: {norms}")
        loop.commit()
        u_prev[:] = u
        reactions.append(float(f[3 * top + 2].sum()))
        histories.append(norms)
    return np.array(reactions), histories, u, solves


class DeviceLoop:
    """gradient producer -> resident law -> force operator, all on the device; nodal vectors are what crosses the link"""

    def __init__(self, resident_state, op, force):
        import torch

        self.rs, self.op, self.force = resident_state, op, force
        dev = torch.device("cuda", op.device)
        self._grad = torch.empty(op.gdim**2 * op.n_points, dtype=torch.float64, device=dev)
        self._grad_v = torch.empty_like(self._grad)
        self._f = torch.empty(op.gdim * op.n_nodes, dtype=torch.float64, device=dev)
        self.bytes_up = self.bytes_down = self.evaluations = self.actions = 0

    def _down(self, x):
        from fenics_constitutive_amd.hostio import to_host

        self.bytes_down += 8 * x.numel()
        return to_host(x)

    def residual(self, t, del_t, du):
        self.bytes_up += du.nbytes
        self.evaluations += 1
        self.rs.evaluate(t, del_t, self.op(du, out=self._grad))
        return self._down(self.force(self.rs.stress, out=self._f))

    def tangent_action(self, v):
        self.bytes_up += v.nbytes
        self.actions += 1
        return self._down(self.force.tangent_action(self.rs.tangent, self.op(v, out=self._grad_v), out=self._f))

    def commit(self):
        self.rs.update()


def cube_operators(mesh):
    """(op, force) of a fe_mini Cube in the layout the laws read"""
    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd.gradient import hex8_reference_gradients, integration_weights, inverse_jacobians

    ref = hex8_reference_gradients()
    x = mesh.nodes[mesh.cells]
    op = fc.DisplacementGradient(np.ascontiguousarray(mesh.cells, dtype=np.int32), ref, inverse_jacobians(x, ref), mesh.n_nodes)
    return op, fc.InternalForce(op, integration_weights(x, ref, np.ones(8)))


def main():
    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd.resident import ResidentState

    m = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    mesh = FE.Cube(m, m, m)
    params = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
    op, force = cube_operators(mesh)
    loop = DeviceLoop(ResidentState(fc.VonMises3D(params), mesh.n_points, placement="torch"), op, force)
    reactions, norms, u, solves = tension_test_matrix_free(mesh, loop, steps=8)
    for k, (r, h) in enumerate(zip(reactions, norms), 1):
        print(f"load step {k}: reaction {r:10.3f}   Newton residuals " + "  ".join(f"{x:.2e}" for x in h))
    host = FE.ResidentProtocolState(ResidentState(fc.VonMises3D(params), mesh.n_points), mesh.n_points)
    reactions_host, norms_host, _ = FE.tension_test(mesh, host, steps=8)
    newton = loop.evaluations
    per_iteration = (loop.bytes_up + loop.bytes_down) / newton
    ndarray_path = (72 + 48 + 288) * mesh.n_points
    difference = np.max(np.abs(reactions - reactions_host)) / np.max(np.abs(reactions_host))
    print(f"{mesh.n_points} quadrature points, {mesh.n_dofs} dofs: {newton} law evaluations, {len(solves)} solves with {min(solves)} .. "
          f"{max(solves)} conjugate-gradient iterations ({loop.actions} tangent actions); {per_iteration / 1e3:.1f} kB of nodal vectors per Newton iteration over the link "
          f"(its solve included) against {ndarray_path / 1e3:.1f} kB of gradient, stress and tangent on the ndarray path; "
          f"largest relative reaction difference to the direct solve {difference:.2e}")
    assert difference <= 1e-8


if __name__ == "__main__":
    main()
