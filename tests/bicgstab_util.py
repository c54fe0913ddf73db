"""Shared by the tests of the device BiCGStab (fenics_constitutive_amd.bicgstab, csrc/jit/bicgstab.hip): the ordered NumPy oracle --
the recurrence of the module docstring on solver_util's product, ordered dot, block inverses and their application, and on
multilevel_util.Oracle for the multilevel cycle, the same operations in the same order: bit for bit what the kernels compute --
and the unsymmetric systems the tests of both files solve."""

from types import SimpleNamespace

import numpy as np
from solver_util import apply_inverse, block_inverses, diagonal_of, matvec, ordered_dot


def _unusable(d):
    return not d != 0.0 or not np.isfinite(d)


def bicgstab(indptr, indices, blocks, b, x0=None, preconditioner="block_jacobi", rtol=1e-8, atol=0.0, maxiter=None):
    """what BiCGStab computes, on the bits: a namespace of x, iterations, converged, status, residual_norm, rhs_norm.
    ``preconditioner``: "block_jacobi", None or a multilevel_util.Oracle of the pattern (set up here from ``blocks``)"""
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    n = b.size
    maxiter = 10 * n if maxiter is None else maxiter
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64).reshape(-1)
    status = "running"
    if preconditioner is None:
        apply = lambda w: w  # noqa: E731
    elif isinstance(preconditioner, str):
        assert preconditioner == "block_jacobi"
        inv, det = block_inverses(diagonal_of(indptr, indices, blocks))
        if (~(det != 0.0) | ~np.isfinite(det)).any():
            status = "singular_block"
        apply = lambda w: apply_inverse(inv, w)  # noqa: E731
    else:
        preconditioner.setup(blocks)
        if preconditioner.singular:
            status = "singular_block"
        apply = preconditioner.apply
    with np.errstate(all="ignore"):
        r = b.copy() if x0 is None else b - matvec(indptr, indices, blocks, x)
        rhat, p = r.copy(), r.copy()
        rr = ordered_dot(r, r)
        rho = rr
        bb = ordered_dot(b, b)
        r2, a2 = rtol * rtol * bb, atol * atol
        thr2 = r2 if r2 > a2 else a2
        iterations = 0
        if status == "running":
            status = "converged" if rr <= thr2 else "nonfinite" if not np.isfinite(rr) else "maxiter" if iterations >= maxiter else "running"
        while status == "running":
            y = apply(p)
            v = matvec(indptr, indices, blocks, y)
            rv = ordered_dot(v, rhat)
            if _unusable(rv):
                status = "breakdown"
                break
            alpha = rho / rv
            x = x + alpha * y
            r = r - alpha * v  # s
            rr = ordered_dot(r, r)
            if rr <= thr2:
                iterations += 1
                status = "converged"
                break
            z = apply(r)
            t = matvec(indptr, indices, blocks, z)
            ts, tt = ordered_dot(t, r), ordered_dot(t, t)
            omega = ts / tt
            if _unusable(tt) or _unusable(omega):
                status = "breakdown"
                break
            x = x + omega * z
            r = r - omega * t
            rr = ordered_dot(r, r)
            rho_new = ordered_dot(rhat, r)
            iterations += 1
            if rr <= thr2:
                status = "converged"
            elif not np.isfinite(rr):
                status = "nonfinite"
            elif _unusable(rho_new):
                status = "breakdown"
            elif iterations >= maxiter:
                status = "maxiter"
            else:
                beta = (rho_new / rho) * (alpha / omega)
                p = r + beta * (p - omega * v)
            rho = rho_new
    return SimpleNamespace(x=x, iterations=iterations, converged=status == "converged", status=status, residual_norm=float(np.sqrt(rr)),
                           rhs_norm=float(np.sqrt(bb)))


# ---- the systems ---------------------------------------------------------------------------------------------------------------
def elastic_mandel(E=210000.0, nu=0.3):
    """the elastic tangent in Mandel form"""
    lam, mu = E * nu / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu))
    c = 2.0 * mu * np.eye(6)
    c[:3, :3] += lam
    return c


def nonassociated_tangent(n, b=0.6, b_flow=0.0, H=2000.0, frac=0.3, seed=5):
    """flat [n 36]: ``C`` at the elastic points and ``T = C - outer(C n_f, n_y C) / (n_y C n_f + H)`` at a seeded fraction ``frac``
    of them, ``n_y = s + b one``, ``n_f = s + b_flow one``, ``s`` a seeded unit deviator-like direction: unsymmetric where
    ``b != b_flow``"""
    c = elastic_mandel()
    rng = np.random.default_rng(seed)
    pl = rng.random(n) < frac
    out = np.tile(c, (n, 1, 1))
    one = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    s = rng.normal(size=(int(pl.sum()), 6))  # (row by row: the draws of the plastic points in ascending order)
    s[:, :3] -= s[:, :3].mean(axis=1, keepdims=True)
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    n_y, n_f = s + b * one, s + b_flow * one
    c_nf, ny_c = n_f @ c.T, n_y @ c
    out[pl] = c - c_nf[:, :, None] * ny_c[:, None, :] / (np.einsum("ij,ij->i", ny_c, n_f) + H)[:, None, None]
    return out.reshape(-1)


def asymmetry(a):
    """``|K - K^T|_F / |K|_F`` of a SciPy sparse matrix"""
    import scipy.sparse.linalg as spla

    return spla.norm(a - a.T) / spla.norm(a)


def oracle_solve_loop(state, dofmap, ref, jinv, weights, n_nodes, **options):
    """solver_util.oracle_solve_loop with the oracle BiCGStab (``options``) in place of the conjugate gradients"""
    import solver_util
    from matrix_util import matrix_oracle

    loop = solver_util.oracle_solve_loop(state, dofmap, ref, jinv, weights, n_nodes)

    def solve():
        indptr, indices, blocks = matrix_oracle(loop.state.tangent, *loop.tables, loop.weights, loop.n_nodes, constrained=loop.mask)
        rhs = np.where(loop.mask, 0.0, loop.f)
        result = bicgstab(indptr, indices, blocks, rhs, **options)
        loop.systems.append((indptr, indices, blocks, rhs, result))
        return result.x, result

    loop.solve = solve
    return loop


def skew_blocks(indptr, indices, d_, seed):
    """[nnzb][D][D]: a skew-symmetric matrix of small integers on a (structurally symmetric) block pattern: ``w^T K w`` is exactly
    zero for every integer ``w``, in every summation order"""
    n = indptr.size - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    cols = np.asarray(indices, dtype=np.int64)
    m = np.random.default_rng(seed).integers(-3, 4, size=(cols.size, d_, d_)).astype(np.float64)
    key, mirrored = rows * n + cols, cols * n + rows
    order = np.argsort(key, kind="stable")
    at = order[np.searchsorted(key[order], mirrored)]
    assert np.array_equal(key[at], mirrored), "the pattern is not structurally symmetric"
    return m - m[at].transpose(0, 2, 1)
