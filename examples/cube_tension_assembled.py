#!/usr/bin/env python3
"""The partly yielding cube of cube_tension_fe.py with the tangent stiffness assembled on the GPU.

Per Newton iteration the host sends the nodal increment ``u - u_prev``; ``DisplacementGradient`` forms ``grad_del_u`` on the
device, ``ResidentState.evaluate`` runs the law there, ``InternalForce`` assembles the nodal internal force and ``TangentMatrix``
the values of the sparse tangent stiffness -- with the Dirichlet rows and columns already made the identity's -- from the tangent
that stays in HBM.  The nodal force and the values array come down; the linear solve is SciPy's sparse direct solver on
``K.to_scipy(values)``.  Problem, load path and convergence criterion are those of ``fe_mini.tension_test``.

Every linear system is also solved matrix-free by conjugate gradients (``force.tangent_action``), once plain and once with the
inverses of ``K.diagonal_blocks(values)`` as a block-Jacobi preconditioner.  Prints the Newton counts, the conjugate-gradient
iterations with and without the preconditioner and the bytes that crossed the link per Newton iteration.

    python examples/cube_tension_assembled.py [cells per edge]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_mini as FE  # noqa: E402
from cube_tension_matrix_free import CG_RTOL, DeviceLoop, cube_operators  # noqa: E402


def tension_test_assembled(mesh, loop, steps: int = 8, top_displacement: float = 0.0065, tilt: float = 0.6, rtol: float = 1e-10,
                           maxit: int = 12, compare_cg: bool = True, cg_rtol: float = CG_RTOL):
    """``fe_mini.tension_test`` with the assembly behind ``loop``: ``loop.residual(t, del_t, du)`` evaluates the law at the
    gradient of the nodal increment and returns the nodal internal force; ``loop.matrix(mask)`` returns the tangent stiffness of
    that evaluate as a SciPy sparse matrix whose rows and columns of the dofs in ``mask`` are the identity's, and the diagonal
    blocks ``[n_nodes][3][3]`` of the same matrix; ``loop.tangent_action(v)`` its product with a nodal vector (matrix-free);
    ``loop.commit()`` commits the load step.  The Newton update is the direct solve.  ``compare_cg``: every system is solved again
    by conjugate gradients on ``loop.tangent_action``, plain and block-Jacobi preconditioned.  Returns the reactions, the Newton
    residual norms, the displacement, and per solve the pair (plain, preconditioned) of conjugate-gradient iterations."""
    import scipy.sparse.linalg as spla

    X = mesh.nodes
    top, bottom = np.flatnonzero(X[:, 2] > 1 - 1e-12), np.flatnonzero(X[:, 2] < 1e-12)
    fixed = set((3 * bottom + 2).tolist()) | set((3 * top + 2).tolist())
    origin = int(np.flatnonzero((np.abs(X) < 1e-12).all(axis=1))[0])
    xcorner = int(np.flatnonzero((np.abs(X - [1.0, 0.0, 0.0]) < 1e-12).all(axis=1))[0])
    fixed |= {3 * origin, 3 * origin + 1, 3 * xcorner + 1}
    fixed = np.array(sorted(fixed))
    mask = np.zeros(mesh.n_dofs, dtype=bool)
    mask[fixed] = True
    free = np.flatnonzero(~mask)
    shape = 1.0 + tilt * (X[top, 0] - 0.5)
    u, u_prev = np.zeros(mesh.n_dofs), np.zeros(mesh.n_dofs)
    full = np.zeros(mesh.n_dofs)

    def matvec(x):
        full[free] = x
        return loop.tangent_action(full)[free]

    action = spla.LinearOperator((free.size, free.size), matvec=matvec, dtype=np.float64)
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
            K, blocks = loop.matrix(mask)
            rhs = np.where(mask, 0.0, f)
            dx = spla.spsolve(K.tocsc(), rhs)  # identity rows and columns at the fixed dofs: dx is zero there
            if compare_cg:
                inverse = np.linalg.inv(blocks)  # (a fixed dof is an identity row and column of its block, of the inverse too)

                def jacobi(x):
                    full[free] = x
                    return np.einsum("nrs,ns->nr", inverse, full.reshape(-1, 3)).reshape(-1)[free]

                counts = []
                for m in (None, spla.LinearOperator((free.size, free.size), matvec=jacobi, dtype=np.float64)):
                    count = [0]
                    x, info = spla.cg(action, r, rtol=cg_rtol, atol=0.0, maxiter=10 * free.size, M=m,
                                      callback=lambda _: count.__setitem__(0, count[0] + 1))
                    if info != 0 or np.linalg.norm(x - dx[free]) > 1e-6 * np.linalg.norm(dx[free]):
                        raise RuntimeError(f"conjugate gradients of load step {step}, iteration {it} do not reproduce the direct solve (info {info})")
                    counts.append(count[0])
                solves.append(tuple(counts))
            u[free] -= dx[free]
        else:
            raise RuntimeError(f"Newton iteration of load step {step} did not converge: {norms}")
        loop.commit()
        u_prev[:] = u
        reactions.append(float(f[3 * top + 2].sum()))
        histories.append(norms)
    return np.array(reactions), histories, u, solves


class AssembledLoop(DeviceLoop):
    """gradient producer -> resident law -> force operator and tangent matrix, all on the device; nodal vectors and the values
    of the matrix are what crosses the link"""

    def __init__(self, resident_state, op, force, matrix):
        import torch

        super().__init__(resident_state, op, force)
        self.K = matrix
        self._values = torch.empty(matrix.nnz, dtype=torch.float64, device=torch.device("cuda", op.device))
        self.assemblies = 0

    def matrix(self, mask):
        self.K.set_constrained(mask)  # (uploaded once: the mask does not change)
        self.assemblies += 1
        values = self.K(self.rs.tangent, out=self._values)
        blocks = self._down(self.K.diagonal_blocks(values))
        return self.K.to_scipy(self._down(values)), blocks


def main():
    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd.resident import ResidentState

    m = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    mesh = FE.Cube(m, m, m)
    params = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
    op, force = cube_operators(mesh)
    K = fc.TangentMatrix(force, format="csr")
    loop = AssembledLoop(ResidentState(fc.VonMises3D(params), mesh.n_points, placement="torch"), op, force, K)
    reactions, norms, u, solves = tension_test_assembled(mesh, loop, steps=8)
    for k, (r, h) in enumerate(zip(reactions, norms), 1):
        print(f"load step {k}: reaction {r:10.3f}   Newton residuals " + "  ".join(f"{x:.2e}" for x in h))
    host = FE.ResidentProtocolState(ResidentState(fc.VonMises3D(params), mesh.n_points), mesh.n_points)
    reactions_host, norms_host, _ = FE.tension_test(mesh, host, steps=8)
    difference = np.max(np.abs(reactions - reactions_host)) / np.max(np.abs(reactions_host))
    plain, jacobi = [s[0] for s in solves], [s[1] for s in solves]
    direct = 8 * (2 * mesh.n_dofs + K.nnz + 9 * mesh.n_nodes)  # du up; f, the values and the diagonal blocks down
    print(f"{mesh.n_points} quadrature points, {mesh.n_dofs} dofs, {K.nnzb} blocks: Newton iterations {[len(h) for h in norms]} "
          f"(direct solve on the host: {[len(h) for h in norms_host]}); conjugate gradients {min(plain)} .. {max(plain)} iterations plain, "
          f"{min(jacobi)} .. {max(jacobi)} with the block-Jacobi preconditioner from diagonal_blocks")
    print(f"link bytes per Newton iteration: {direct / 1e3:.1f} kB with the assembled matrix (nodal vectors, {8 * K.nnz / 1e3:.1f} kB of values), "
          f"{16 * mesh.n_dofs * (1 + np.mean(jacobi)) / 1e3:.1f} kB matrix-free with the preconditioner, {16 * mesh.n_dofs * (1 + np.mean(plain)) / 1e3:.1f} kB "
          f"without, {(72 + 48 + 288) * mesh.n_points / 1e3:.1f} kB of gradient, stress and tangent on the ndarray path; "
          f"largest relative reaction difference to the host run {difference:.2e}")
    assert difference <= 1e-8 and [len(h) for h in norms] == [len(h) for h in norms_host]


if __name__ == "__main__":
    main()
