"""Shared by the tests of the multilevel preconditioner (fenics_constitutive_amd.multilevel, csrc/jit/multilevel.hip): the NumPy oracle
-- the aggregation written out node by node as the module states it, the Galerkin sums over the fold lists, restriction,
prolongation, the damped sweeps, both cycles and the conjugate gradients around them, the same operations in the same order: bit
for bit what the kernels compute."""

from types import SimpleNamespace

import numpy as np
from solver_util import apply_inverse, block_inverses, diagonal_of, matvec, ordered_dot

EPS = 2.0**-52


def aggregate(indptr, indices):
    """(agg, roots) by the three passes, node by node (the module's own is partly vectorised)"""
    n = indptr.size - 1
    nb = [indices[indptr[v]: indptr[v + 1]].tolist() for v in range(n)]
    agg = [-1] * n
    roots = []
    for v in range(n):
        if all(agg[u] < 0 for u in nb[v] + [v]):
            for u in nb[v] + [v]:
                agg[u] = len(roots)
            roots.append(v)
    first = list(agg)
    for v in range(n):
        if first[v] < 0:
            near = [u for u in sorted(nb[v]) if first[u] >= 0]
            if near:
                agg[v] = first[near[0]]
    for v in range(n):
        if agg[v] < 0:
            agg[v] = len(roots)
            roots.append(v)
    return np.array(agg, dtype=np.int64).reshape(n), np.array(roots, dtype=np.int64).reshape(-1)


def coarsen(indptr, indices, agg, n_agg):
    """(indptr, indices, folds): the coarse pattern from the set of aggregate pairs, folds[K] the fine blocks of coarse block K"""
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    lists = {}
    for k, (i, j) in enumerate(zip(agg[rows].tolist(), agg[indices].tolist())):
        lists.setdefault((i, j), []).append(k)
    pairs = sorted(lists)
    c_indptr = np.zeros(n_agg + 1, dtype=np.int64)
    for i, _ in pairs:
        c_indptr[i + 1] += 1
    return np.cumsum(c_indptr), np.array([j for _, j in pairs], dtype=np.int64).reshape(-1), [lists[p] for p in pairs]


def hierarchy(indptr, indices, coarsest_nodes=64, max_levels=10):
    """[namespace(indptr, indices, agg, roots, folds)], finest first (the last level has no agg)"""
    levels = [SimpleNamespace(indptr=np.asarray(indptr, dtype=np.int64), indices=np.asarray(indices, dtype=np.int64), agg=None, roots=None, folds=None)]
    while levels[-1].indptr.size - 1 > coarsest_nodes and len(levels) < max_levels:
        fine = levels[-1]
        agg, roots = aggregate(fine.indptr, fine.indices)
        if roots.size >= fine.indptr.size - 1:
            break
        c_indptr, c_indices, folds = coarsen(fine.indptr, fine.indices, agg, roots.size)
        fine.agg, fine.roots, fine.folds = agg, roots, folds
        levels.append(SimpleNamespace(indptr=c_indptr, indices=c_indices, agg=None, roots=None, folds=None))
    return levels


def _ragged(lists):
    """(table[n][longest], lengths): the lists side by side, padded with 0"""
    lengths = np.array([len(x) for x in lists], dtype=np.int64).reshape(-1)
    table = np.zeros((len(lists), int(lengths.max()) if lengths.size else 0), dtype=np.int64)
    for i, x in enumerate(lists):
        table[i, : len(x)] = x
    return table, lengths


def galerkin(folds, blocks):
    """f = 0.0; f = f + blocks[k] over the fold list of every coarse block, ascending"""
    table, lengths = _ragged(folds)
    out = np.zeros((len(folds),) + blocks.shape[1:])
    for j in range(table.shape[1]):
        on = np.flatnonzero(lengths > j)
        out[on] = out[on] + blocks[table[on, j]]
    return out


def restrict(agg, n_agg, d):
    """rc[I] = 0.0; rc = rc + d[i] over the members i of I, ascending"""
    members = [[] for _ in range(n_agg)]
    for i, a in enumerate(agg.tolist()):
        members[a].append(i)
    table, lengths = _ragged(members)
    dn = d.reshape(agg.size, -1)
    out = np.zeros((n_agg, dn.shape[1]))
    for j in range(table.shape[1]):
        on = np.flatnonzero(lengths > j)
        out[on] = out[on] + dn[table[on, j]]
    return out.reshape(-1)


def prolong(agg, x, xc, mask=None):
    """x[i] = x[i] + xc[agg[i]], skipped where the mask is set"""
    d_ = x.size // agg.size
    new = (x.reshape(-1, d_) + xc.reshape(-1, d_)[agg]).reshape(-1)
    return new if mask is None else np.where(mask, x, new)


class Oracle:
    """the preconditioner of one matrix: ``setup(blocks)`` then ``apply(r)``; ``values[l]``, ``inv[l]``, ``det[l]`` per level"""

    def __init__(self, indptr, indices, cycle="multiplicative", smoothing=1, omega=0.5, coarsest_nodes=64, coarsest_sweeps=8, max_levels=10, mask=None):
        self.levels = hierarchy(indptr, indices, coarsest_nodes, max_levels)
        self.cycle, self.smoothing, self.omega, self.coarsest_sweeps, self.mask = cycle, smoothing, omega, coarsest_sweeps, mask

    def setup(self, blocks):
        self.values = [np.asarray(blocks, dtype=np.float64)]
        for lv in self.levels[:-1]:
            self.values.append(galerkin(lv.folds, self.values[-1]))
        both = [block_inverses(diagonal_of(lv.indptr, lv.indices, v)) for lv, v in zip(self.levels, self.values)]
        self.inv, self.det = [b[0] for b in both], [b[1] for b in both]
        self.singular = any((~(det != 0.0) | ~np.isfinite(det)).any() for det in self.det)
        return self

    def product(self, l, x):
        lv = self.levels[l]
        return matvec(lv.indptr, lv.indices, self.values[l], x)

    def sweeps(self, l, b, x, count):
        """``count`` sweeps; ``x`` None: from zero"""
        for _ in range(count):
            if x is None:
                x = self.omega * apply_inverse(self.inv[l], b)
            else:
                x = x + self.omega * apply_inverse(self.inv[l], b - self.product(l, x))
        return x

    def apply(self, r):
        with np.errstate(all="ignore"):
            return self._additive(r) if self.cycle == "additive" else self._multiplicative(0, np.asarray(r, dtype=np.float64))

    def _mask(self, l):
        return self.mask if l == 0 else None

    def _multiplicative(self, l, b):
        if l == len(self.levels) - 1:
            return self.sweeps(l, b, None, self.coarsest_sweeps)
        lv = self.levels[l]
        x = self.sweeps(l, b, None, self.smoothing)
        xc = self._multiplicative(l + 1, restrict(lv.agg, lv.roots.size, b - self.product(l, x)))
        return self.sweeps(l, b, prolong(lv.agg, x, xc, self._mask(l)), self.smoothing)

    def _additive(self, r):
        last = len(self.levels) - 1
        b, z = [np.asarray(r, dtype=np.float64)], []
        for l in range(last):
            z.append(apply_inverse(self.inv[l], b[l]))
            b.append(restrict(self.levels[l].agg, self.levels[l].roots.size, b[l]))
        z.append(self.sweeps(last, b[last], None, self.coarsest_sweeps))
        for l in range(last - 1, -1, -1):
            z[l] = prolong(self.levels[l].agg, z[l], z[l + 1], self._mask(l))
        return z[0]


def conjugate_gradient(oracle, blocks, b, x0=None, rtol=1e-8, atol=0.0, maxiter=None):
    """what ``ConjugateGradient(K, preconditioner=<multilevel>)`` computes, on the bits (solver_util.conjugate_gradient with the cycle
    behind the update and the closing kernel's status: a counted iteration whose r . z is not positive ends as "indefinite")"""
    fine = oracle.levels[0]
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    n = b.size
    maxiter = 10 * n if maxiter is None else maxiter
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64).reshape(-1)
    oracle.setup(blocks)
    status = "singular_block" if oracle.singular else "running"
    with np.errstate(all="ignore"):
        r = b.copy() if x0 is None else b - matvec(fine.indptr, fine.indices, oracle.values[0], x)
        rr, bb = ordered_dot(r, r), ordered_dot(b, b)
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

        def close():
            z = oracle.apply(r)
            rz = ordered_dot(r, z)
            return z, rz, "running" if rz > 0.0 else "indefinite"

        if status == "running":
            status = ended(rr)
        if status == "running":
            z, rz, status = close()
            p = z.copy()
        while status == "running":
            q = matvec(fine.indptr, fine.indices, oracle.values[0], p)
            pq = ordered_dot(p, q)
            if not pq > 0.0:
                status = "indefinite"
                break
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * q
            rr = ordered_dot(r, r)
            iterations += 1
            status = ended(rr)
            if status == "running":
                z, rz_new, status = close()
                if status == "running":
                    p = z + (rz_new / rz) * p
                    rz = rz_new
    return SimpleNamespace(x=x, iterations=iterations, converged=status == "converged", status=status, residual_norm=float(np.sqrt(rr)),
                           rhs_norm=float(np.sqrt(bb)))
