"""Shared by the tests of the device solver (fenics_constitutive_amd.solver): the ordered NumPy oracle of
csrc/jit/conjugate_gradient.hip -- the segmented dot, the matrix-vector product over the block pattern, the explicit block
inverses and the conjugate-gradient recurrence, the same operations in the same order: bit for bit what the kernels compute --
and the inputs the tests of both files build their systems from."""

import math
from types import SimpleNamespace

import numpy as np

SEG = 3072
LANES = 256
EPS = 2.0**-52


def _tree(acc):
    """acc[.., t] = acc[.., t] + acc[.., t + h], h = 128, 64, .., 1; returns acc[.., 0]"""
    acc = acc.copy()
    h = LANES // 2
    while h >= 1:
        acc[..., :h] = acc[..., :h] + acc[..., h: 2 * h]
        h //= 2
    return acc[..., 0]


def _lane_sums(terms):
    """terms[.., i, t]: acc = 0.0; acc = acc + terms[i], i ascending"""
    acc = np.zeros(terms.shape[:-2] + (LANES,))
    for i in range(terms.shape[-2]):
        acc = acc + terms[..., i, :]
    return acc


def ordered_dot(a, b):
    """the solver's dot: segments of SEG entries, lane t of 256 over e = seg SEG + t + 256 i, the tree, the partials by segment, the
    same lane-strided sum and tree over the partials"""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    n = a.size
    nseg = -(-n // SEG)
    if nseg == 0:
        return 0.0
    prod = np.zeros(nseg * SEG)
    prod[:n] = a * b  # (a skipped entry and an added +0.0 are the same: acc starts at +0.0 and never becomes -0.0)
    partials = _tree(_lane_sums(prod.reshape(nseg, SEG // LANES, LANES)))
    rounds = -(-nseg // LANES)
    padded = np.zeros(rounds * LANES)
    padded[:nseg] = partials
    return float(_tree(_lane_sums(padded.reshape(rounds, LANES))))


def dot_bound(a, b):
    """(SEG/256 + 8 + ceil(segments/256) + 8) 2^-52 sum |a_i b_i|: the sums of a lane, the tree, the sums over the partials, the tree"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    nseg = -(-a.size // SEG)
    return (SEG // LANES + 8 + -(-nseg // LANES) + 8) * EPS * math.fsum(np.abs(a * b))


def matvec(indptr, indices, blocks, p):
    """q[D v + r] = 0.0; q = q + blocks[k][r][s] * p[D indices[k] + s] over k = indptr[v] .. indptr[v + 1] ascending, s ascending"""
    n_nodes, d_ = indptr.size - 1, blocks.shape[1]
    q = np.zeros((n_nodes, d_))
    pn = np.asarray(p, dtype=np.float64).reshape(n_nodes, d_)
    per_row = np.diff(indptr)
    first = indptr[:-1].astype(np.int64)
    for j in range(int(per_row.max()) if per_row.size else 0):
        rows = np.flatnonzero(per_row > j)
        k = first[rows] + j
        for s in range(d_):
            q[rows] = q[rows] + blocks[k, :, s] * pn[indices[k], s, None]
    return q.reshape(-1)


def block_inverses(diag):
    """(inv[n][D][D], det[n]) by the explicit formulas of the kernel"""
    d_ = diag.shape[1]
    a = diag
    inv = np.empty_like(diag)
    with np.errstate(all="ignore"):
        if d_ == 1:
            det = a[:, 0, 0].copy()
            inv[:, 0, 0] = 1.0 / det
        elif d_ == 2:
            det = a[:, 0, 0] * a[:, 1, 1] - a[:, 0, 1] * a[:, 1, 0]
            inv[:, 0, 0], inv[:, 0, 1], inv[:, 1, 0], inv[:, 1, 1] = a[:, 1, 1] / det, -a[:, 0, 1] / det, -a[:, 1, 0] / det, a[:, 0, 0] / det
        else:
            m = lambda i, j: a[:, i, j]  # noqa: E731
            c = [[m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1), m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2), m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0)],
                 [m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2), m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0), m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1)],
                 [m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1), m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2), m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)]]
            det = m(0, 0) * c[0][0] + m(0, 1) * c[0][1] + m(0, 2) * c[0][2]
            for i in range(3):
                for j in range(3):
                    inv[:, i, j] = c[j][i] / det
    return inv, det


def apply_inverse(inv, r):
    """z[D v + r] = 0.0; z = z + inv[v][r][s] * r_[D v + s], s ascending"""
    n_nodes, d_ = inv.shape[:2]
    rn = r.reshape(n_nodes, d_)
    z = np.zeros((n_nodes, d_))
    for s in range(d_):
        z = z + inv[:, :, s] * rn[:, s, None]
    return z.reshape(-1)


def diagonal_of(indptr, indices, blocks):
    """[n_nodes][D][D]: every node's own block (a node without one is an AssertionError)"""
    n_nodes = indptr.size - 1
    rows = np.repeat(np.arange(n_nodes), np.diff(indptr))
    on = np.flatnonzero(rows == indices)
    assert np.array_equal(rows[on], np.arange(n_nodes)), "a node has no diagonal block"
    return blocks[on]


def conjugate_gradient(indptr, indices, blocks, b, x0=None, preconditioner="block_jacobi", rtol=1e-8, atol=0.0, maxiter=None):
    """what ConjugateGradient computes, on the bits: a namespace of x, iterations, converged, status, residual_norm, rhs_norm"""
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    n = b.size
    maxiter = 10 * n if maxiter is None else maxiter
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64).reshape(-1)
    status = "running"
    inv = None
    if preconditioner is not None:
        inv, det = block_inverses(diagonal_of(indptr, indices, blocks))
        if (~(det != 0.0) | ~np.isfinite(det)).any():
            status = "singular_block"
    with np.errstate(all="ignore"):
        r = b.copy() if x0 is None else b - matvec(indptr, indices, blocks, x)
        z = r if inv is None else apply_inverse(inv, r)
        p = z.copy()
        rr = ordered_dot(r, r)
        rz = rr if inv is None else ordered_dot(r, z)
        bb = ordered_dot(b, b)
        r2, a2 = rtol * rtol * bb, atol * atol
        thr2 = r2 if r2 > a2 else a2
        iterations = 0

        def ended(rr):
            if rr <= thr2:
                return "converged"
            if not np.isfinite(rr):
                return "nonfinite"
            if iterations >= maxiter:
                return "maxiter"
            return "running"

        if status == "running":
            status = ended(rr)
        while status == "running":
            q = matvec(indptr, indices, blocks, p)
            pq = ordered_dot(p, q)
            if not pq > 0.0:
                status = "indefinite"
                break
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * q
            z = r if inv is None else apply_inverse(inv, r)
            rr = ordered_dot(r, r)
            rz_new = rr if inv is None else ordered_dot(r, z)
            iterations += 1
            status = ended(rr)
            if status == "running":
                beta = rz_new / rz
                p = z + beta * p
            rz = rz_new
    return SimpleNamespace(x=x, iterations=iterations, converged=status == "converged", status=status, residual_norm=float(np.sqrt(rr)),
                           rhs_norm=float(np.sqrt(bb)))


def csr_order(indptr, indices, blocks):
    """the blocks' entries in the order of the scalar CSR (matrix_util.csr_values)"""
    from matrix_util import csr_values

    return csr_values(indptr, indices, blocks)


def from_format(fmt, indptr, indices, flat, d_):
    """values of format ``fmt`` as blocks [nnzb][D][D]"""
    flat = np.asarray(flat, dtype=np.float64).reshape(-1)
    if fmt == "bsr":
        return flat.reshape(-1, d_, d_)
    perm = csr_order(indptr, indices, np.arange(flat.size, dtype=np.float64).reshape(-1, d_, d_)).astype(np.int64)
    out = np.empty(flat.size)
    out[perm] = flat
    return out.reshape(-1, d_, d_)


def full_pattern(dofmap, n_nodes):
    """a pattern dofmap in which every node has a diagonal block: the cells and, for every node no cell touches, a cell of its own"""
    unused = np.flatnonzero(np.bincount(dofmap.reshape(-1), minlength=n_nodes) == 0)
    return np.concatenate([dofmap, np.repeat(unused.astype(np.int32)[:, None], dofmap.shape[1], axis=1)]), unused


def spd_tangent(n_points, s_, seed, integer):
    """a symmetric positive definite tangent per point, flat [n_points S S]"""
    rng = np.random.default_rng(seed)
    m = rng.integers(-2, 3, size=(n_points, s_, s_)).astype(np.float64) if integer else rng.normal(size=(n_points, s_, s_))
    c = m @ m.transpose(0, 2, 1) + (4.0 if integer else 1.0) * np.eye(s_)
    return (c if integer else 1e4 * c).reshape(-1)


def oracle_solve_loop(state, dofmap, ref, jinv, weights, n_nodes, **cg_options):
    """the ``loop`` of examples/cube_tension_device_solve.py on the CPU: force_util.OracleLoop, the oracle matrix of matrix_util and
    the oracle conjugate gradients (``cg_options``); ``loop.systems`` keeps (indptr, indices, blocks, rhs, result) of every solve"""
    from force_util import OracleLoop, force_oracle
    from gradient_util import oracle
    from matrix_util import matrix_oracle

    class Loop(OracleLoop):
        systems = []

        def constrain(self, mask, top_dofs):
            self.mask, self.top_dofs = mask, top_dofs

        def residual_norms(self, t, del_t, du):
            self.state.evaluate(t, del_t, oracle(du, *self.tables, self.layout))
            self.f = f = force_oracle(self.state.stress, *self.tables, self.weights, self.n_nodes)
            return float(np.linalg.norm(f[~self.mask])), float(np.linalg.norm(f[self.mask])), float(f[self.top_dofs].sum())

        def solve(self):
            indptr, indices, blocks = matrix_oracle(self.state.tangent, *self.tables, self.weights, self.n_nodes, constrained=self.mask)
            rhs = np.where(self.mask, 0.0, self.f)
            result = conjugate_gradient(indptr, indices, blocks, rhs, **cg_options)
            self.systems.append((indptr, indices, blocks, rhs, result))
            return result.x, result

    loop = Loop(state, dofmap, ref, jinv, weights, n_nodes)
    loop.systems = []
    return loop
