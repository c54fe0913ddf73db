"""Shared by the tests of the rigid-body coarse space of the multilevel preconditioner (fenics_constitutive_amd.multilevel with
``coarse_space="rigid_body"``, csrc/jit/multilevel_rigid.hip): the NumPy oracle -- positions and offsets node by node, the
prolongation blocks, the Galerkin triple products, restriction and prolongation in the order the module docstring states, the 6 x 6
Gauss-Jordan inverse in the kernel's order, and both cycles on multilevel_util.Oracle (whose sweeps, products and conjugate
gradients work on blocks of any size): bit for bit what the kernels compute."""

import numpy as np
import multilevel_util as MU
import solver_util
from multilevel_util import _ragged
from solver_util import apply_inverse, diagonal_of

EPS = MU.EPS


def coarse_dofs(g):
    return {1: 1, 2: 3, 3: 6}[g]


def place(levels, coordinates):
    """(positions, offsets) per level: a coarse node's position is s = 0.0; s = s + x_i over its members ascending, then s / count;
    o_i = x_i - x_agg(i) (the coarsest level has no offsets: None)"""
    positions, offsets = [np.array(coordinates, dtype=np.float64)], []
    for lv in levels[:-1]:
        x = positions[-1]
        n_agg = lv.roots.size
        total, count = np.zeros((n_agg, x.shape[1])), np.zeros(n_agg)
        for i, a in enumerate(lv.agg.tolist()):
            total[a] = total[a] + x[i]
            count[a] += 1.0
        positions.append(total / count[:, None])
        offsets.append(x - positions[-1][lv.agg])
    return positions, offsets + [None]


def b_matrix(o):
    """[n][G][R]: theta -> theta x o"""
    n, g = o.shape
    if g == 2:
        return np.stack([-o[:, 1], o[:, 0]], axis=1)[:, :, None]
    zero = np.zeros(n)
    return np.stack([np.stack([zero, o[:, 2], -o[:, 1]], axis=1), np.stack([-o[:, 2], zero, o[:, 0]], axis=1),
                     np.stack([o[:, 1], -o[:, 0], zero], axis=1)], axis=1)


def p_blocks(o, df):
    """[n][Df][Dc]: [I B(o)] for Df = G, [[I, B(o)], [0, I]] for Df = Dc"""
    n, g = o.shape
    dc = coarse_dofs(g)
    p = np.zeros((n, df, dc))
    p[:, np.arange(df), np.arange(df)] = 1.0
    p[:, :g, g:] = b_matrix(o)
    return p


def galerkin(folds, blocks, rows, cols, p):
    """f = 0.0; per fine block k = (i, j) of the fold list, ascending: t = 0.0; for a: u = 0.0; u = u + K[a][b] * P_j[b][s], b
    ascending; t = t + P_i[a][r] * u; f = f + t"""
    table, lengths = _ragged(folds)
    df, dc = p.shape[1:]
    out = np.zeros((len(folds), dc, dc))
    for j in range(table.shape[1]):
        on = np.flatnonzero(lengths > j)
        k = table[on, j]
        kk, pi, pj = blocks[k], p[rows[k]], p[cols[k]]
        t = np.zeros((on.size, dc, dc))
        for a in range(df):
            u = np.zeros((on.size, dc))
            for b in range(df):
                u = u + kk[:, a, b, None] * pj[:, b, :]
            t = t + pi[:, a, :, None] * u[:, None, :]
        out[on] = out[on] + t
    return out


def restrict(agg, n_agg, d, p):
    """rc[I][c] = 0.0; per member i ascending: t = 0.0; t = t + P_i[a][c] * d_i[a], a ascending; rc = rc + t"""
    members = [[] for _ in range(n_agg)]
    for i, a in enumerate(agg.tolist()):
        members[a].append(i)
    table, lengths = _ragged(members)
    df, dc = p.shape[1:]
    dn = d.reshape(agg.size, df)
    out = np.zeros((n_agg, dc))
    for j in range(table.shape[1]):
        on = np.flatnonzero(lengths > j)
        i = table[on, j]
        t = np.zeros((on.size, dc))
        for a in range(df):
            t = t + p[i, a, :] * dn[i, a, None]
        out[on] = out[on] + t
    return out.reshape(-1)


def prolong(agg, x, xc, p, mask=None):
    """t = 0.0; t = t + P_i[r][c] * xc[agg[i]][c], c ascending; x_i[r] = x_i[r] + t, skipped where the mask is set"""
    df, dc = p.shape[1:]
    xa = xc.reshape(-1, dc)[agg]
    t = np.zeros((agg.size, df))
    for c in range(dc):
        t = t + p[:, :, c] * xa[:, c, None]
    new = (x.reshape(-1, df) + t).reshape(-1)
    return new if mask is None else np.where(mask, x, new)


def block_inverses(diag):
    """(inv, det) as solver_util.block_inverses; 6 x 6: Gauss-Jordan in place, pivots 0 .. 5 in order, no search; ``det`` is 1.0 or,
    with a zero or non-finite pivot, 0.0"""
    if diag.shape[1] != 6:
        return solver_util.block_inverses(diag)
    m = np.array(diag, dtype=np.float64)
    det = np.ones(m.shape[0])
    with np.errstate(all="ignore"):
        for k in range(6):
            piv = m[:, k, k].copy()
            det[~(piv != 0.0) | ~np.isfinite(piv)] = 0.0
            m[:, k, k] = 1.0
            for j in range(6):
                m[:, k, j] = m[:, k, j] / piv
            for i in range(6):
                if i == k:
                    continue
                f = m[:, i, k].copy()
                m[:, i, k] = 0.0
                for j in range(6):
                    m[:, i, j] = m[:, i, j] - f * m[:, k, j]
    return m, det


class Oracle(MU.Oracle):
    """multilevel_util.Oracle with the rigid-body coarse space: ``Oracle(indptr, indices, coordinates, ...)``; ``p[l]`` the
    prolongation blocks of level ``l``, ``positions[l]``, ``offsets[l]``"""

    def __init__(self, indptr, indices, coordinates, **options):
        super().__init__(indptr, indices, **options)
        g = coordinates.shape[1]
        self.positions, self.offsets = place(self.levels, coordinates)
        self.dofs = [g] + [coarse_dofs(g)] * (len(self.levels) - 1)
        self.p = [p_blocks(o, df) for o, df in zip(self.offsets[:-1], self.dofs)]

    def setup(self, blocks):
        self.values = [np.asarray(blocks, dtype=np.float64)]
        with np.errstate(all="ignore"):
            for lv, p in zip(self.levels[:-1], self.p):
                rows = np.repeat(np.arange(lv.indptr.size - 1), np.diff(lv.indptr))
                self.values.append(galerkin(lv.folds, self.values[-1], rows, lv.indices, p))
        both = [block_inverses(diagonal_of(lv.indptr, lv.indices, v)) for lv, v in zip(self.levels, self.values)]
        self.inv, self.det = [b[0] for b in both], [b[1] for b in both]
        self.singular = any((~(det != 0.0) | ~np.isfinite(det)).any() for det in self.det)
        return self

    def _multiplicative(self, l, b):
        if l == len(self.levels) - 1:
            return self.sweeps(l, b, None, self.coarsest_sweeps)
        lv = self.levels[l]
        x = self.sweeps(l, b, None, self.smoothing)
        xc = self._multiplicative(l + 1, restrict(lv.agg, lv.roots.size, b - self.product(l, x), self.p[l]))
        return self.sweeps(l, b, prolong(lv.agg, x, xc, self.p[l], self._mask(l)), self.smoothing)

    def _additive(self, r):
        last = len(self.levels) - 1
        b, z = [np.asarray(r, dtype=np.float64)], []
        for l in range(last):
            z.append(apply_inverse(self.inv[l], b[l]))
            b.append(restrict(self.levels[l].agg, self.levels[l].roots.size, b[l], self.p[l]))
        z.append(self.sweeps(last, b[last], None, self.coarsest_sweeps))
        for l in range(last - 1, -1, -1):
            z[l] = prolong(self.levels[l].agg, z[l], z[l + 1], self.p[l], self._mask(l))
        return z[0]


conjugate_gradient = MU.conjugate_gradient


def rigid_modes(x, x0, dofs):
    """[n dofs][Dc]: the rigid-body modes about ``x0`` at the positions ``x``: for nodes of G dofs the displacements ``t + theta x (x -
    x0)``, for nodes of Dc dofs those and the rotation itself -- the columns of P with the offset x - x0"""
    return p_blocks(x - x0, dofs).reshape(x.shape[0] * dofs, -1)
