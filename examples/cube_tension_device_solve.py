#!/usr/bin/env python3
"""The partly yielding cube of cube_tension_assembled.py with the linear solve on the GPU as well.

Per Newton iteration the host sends the nodal increment ``u - u_prev``; ``DisplacementGradient``, ``ResidentState.evaluate``,
``InternalForce`` and ``TangentMatrix`` run on the device as in cube_tension_assembled.py, and ``fc.ConjugateGradient`` -- block-Jacobi
preconditioned conjugate gradients on the values that stay in HBM -- solves ``K dx = f`` there, the right-hand side zeroed at the
Dirichlet dofs by ``torch.where`` on the device mask.  The Newton update ``dx`` comes down, and per solve 96 bytes of control block
go up and 32 bytes of status, count and norms come down at every look; of the residual only three scalars do
(its norm over the free dofs, over the fixed dofs, and the reaction).  Problem, load path and convergence criterion are those of
``fe_mini.tension_test``; the run of cube_tension_assembled.py (values downloaded, SciPy's direct solver) is the comparison.

    python examples/cube_tension_device_solve.py [cells per edge]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_mini as FE  # noqa: E402
from cube_tension_assembled import AssembledLoop, tension_test_assembled  # noqa: E402
from cube_tension_matrix_free import CG_RTOL, cube_operators  # noqa: E402


def tension_constraints(mesh):
    """(mask of the Dirichlet dofs, the z dofs of the top face) of ``fe_mini.tension_test``"""
    X = mesh.nodes
    top, bottom = np.flatnonzero(X[:, 2] > 1 - 1e-12), np.flatnonzero(X[:, 2] < 1e-12)
    fixed = set((3 * bottom + 2).tolist()) | set((3 * top + 2).tolist())
    origin = int(np.flatnonzero((np.abs(X) < 1e-12).all(axis=1))[0])
    xcorner = int(np.flatnonzero((np.abs(X - [1.0, 0.0, 0.0]) < 1e-12).all(axis=1))[0])
    fixed |= {3 * origin, 3 * origin + 1, 3 * xcorner + 1}
    mask = np.zeros(mesh.n_dofs, dtype=bool)
    mask[sorted(fixed)] = True
    return mask, 3 * top + 2


def tension_test_device_solve(mesh, loop, steps: int = 8, top_displacement: float = 0.0065, tilt: float = 0.6, rtol: float = 1e-10,
                              maxit: int = 12):
    """``fe_mini.tension_test`` with assembly and solve behind ``loop``: ``loop.constrain(mask, top)`` names the Dirichlet dofs and
    the dofs whose internal force sums to the reaction; ``loop.residual_norms(t, del_t, du)`` evaluates the law at the gradient of
    the nodal increment and returns (norm of the internal force over the free dofs, over the fixed dofs, the reaction);
    ``loop.solve()`` solves the tangent stiffness of that evaluate against that internal force (zero at the fixed dofs) and returns
    (the nodal vector ``dx``, a result with ``converged`` and ``iterations``); ``loop.commit()`` commits the load step.  Returns the
    reactions, the Newton residual norms, the displacement and the conjugate-gradient iterations of every solve."""
    mask, top_dofs = tension_constraints(mesh)
    free = np.flatnonzero(~mask)
    shape = 1.0 + tilt * (mesh.nodes[top_dofs // 3, 0] - 0.5)
    loop.constrain(mask, top_dofs)
    u, u_prev = np.zeros(mesh.n_dofs), np.zeros(mesh.n_dofs)
    reactions, histories, solves = [], [], []
    for step in range(1, steps + 1):
        u[top_dofs] = top_displacement * step / steps * shape
        norms = []
        for it in range(maxit + 1):
            norm_free, norm_fixed, reaction = loop.residual_norms(float(step - 1), 1.0, u - u_prev)
            norms.append(norm_free)
            if norm_free <= rtol * max(norm_fixed, 1.0):
                break
            dx, result = loop.solve()
            if not result.converged:
                raise RuntimeError(f"conjugate gradients of load step {step}, iteration {it} ended with status {result.status!r} after "
                                   f"{result.iterations} iterations")
            solves.append(result.iterations)
            u[free] -= dx[free]
        else:
            raise RuntimeError(f"Newton iteration of load step {step} did not converge: {norms}")
        loop.commit()
        u_prev[:] = u
        reactions.append(reaction)
        histories.append(norms)
    return np.array(reactions), histories, u, solves


class DeviceSolveLoop(AssembledLoop):
    """gradient producer -> resident law -> force operator -> tangent matrix -> conjugate gradients, all on the device; the nodal
    increment goes up, the Newton update and three scalars come down"""

    def __init__(self, resident_state, op, force, matrix, cg):
        import torch

        super().__init__(resident_state, op, force, matrix)
        self.cg = cg
        self._dx = torch.empty_like(self._f)
        self._zero = torch.zeros((), dtype=torch.float64, device=self._f.device)

    def constrain(self, mask, top_dofs):
        from fenics_constitutive_amd.hostio import to_device

        self.K.set_constrained(mask)  # (uploaded once: the mask does not change)
        dev = self._f.device
        self._mask = to_device(mask, dev)
        self._free, self._fixed = to_device(np.flatnonzero(~mask), dev), to_device(np.flatnonzero(mask), dev)
        self._top = to_device(np.asarray(top_dofs, dtype=np.int64), dev)

    def residual_norms(self, t, del_t, du):
        import torch

        self.bytes_up += du.nbytes
        self.evaluations += 1
        self.rs.evaluate(t, del_t, self.op(du, out=self._grad))
        f = self.force(self.rs.stress, out=self._f)
        scalars = torch.stack([torch.linalg.vector_norm(f[self._free]), torch.linalg.vector_norm(f[self._fixed]), f[self._top].sum()])
        self.bytes_down += 8 * 3
        return tuple(float(x) for x in scalars.cpu())

    def solve(self):
        import torch

        self.assemblies += 1
        values = self.K(self.rs.tangent, out=self._values)
        result = self.cg(values, torch.where(self._mask, self._zero, self._f), out=self._dx)
        self.bytes_up += 96  # the control block, once per solve
        self.bytes_down += 32 * result.looks  # status, count and the two norms, at every look
        return self._down(result.x), result


def main():
    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd.resident import ResidentState

    m = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    mesh = FE.Cube(m, m, m)
    params = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
    op, force = cube_operators(mesh)
    K = fc.TangentMatrix(force, format="bsr")
    cg = fc.ConjugateGradient(K, preconditioner="block_jacobi", rtol=CG_RTOL)
    loop = DeviceSolveLoop(ResidentState(fc.VonMises3D(params), mesh.n_points, placement="torch"), op, force, K, cg)
    reactions, norms, u, solves = tension_test_device_solve(mesh, loop, steps=8)
    for k, (r, h) in enumerate(zip(reactions, norms), 1):
        print(f"load step {k}: reaction {r:10.3f}   Newton residuals " + "  ".join(f"{x:.2e}" for x in h))
    # the comparison: the values downloaded, SciPy's sparse direct solver on the host
    op2, force2 = cube_operators(mesh)
    K2 = fc.TangentMatrix(force2, format="csr")
    direct = AssembledLoop(ResidentState(fc.VonMises3D(params), mesh.n_points, placement="torch"), op2, force2, K2)
    reactions_direct, norms_direct, _, _ = tension_test_assembled(mesh, direct, steps=8, compare_cg=False)
    difference = np.max(np.abs(reactions - reactions_direct)) / np.max(np.abs(reactions_direct))
    per_iteration = (loop.bytes_up + loop.bytes_down) / loop.evaluations
    per_iteration_direct = (direct.bytes_up + direct.bytes_down) / direct.evaluations
    print(f"{mesh.n_points} quadrature points, {mesh.n_dofs} dofs, {K.nnzb} blocks: Newton iterations {[len(h) for h in norms]} "
          f"(direct solve of the downloaded matrix: {[len(h) for h in norms_direct]}); {len(solves)} solves on the device with "
          f"{min(solves)} .. {max(solves)} conjugate-gradient iterations each: {solves}")
    print(f"link bytes per Newton iteration: {per_iteration / 1e3:.1f} kB with the solve on the device (the increment up, the update down, "
          f"the scalars) against {per_iteration_direct / 1e3:.1f} kB with the values downloaded ({8 * K.nnz / 1e3:.1f} kB of them); "
          f"largest relative reaction difference to the direct solve {difference:.2e}")
    assert difference <= 1e-8 and [len(h) for h in norms] == [len(h) for h in norms_direct]


if __name__ == "__main__":
    main()
