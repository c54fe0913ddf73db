"""Shared by the tests of the multilevel preconditioner of a matrix-free operator (fenics_constitutive_amd.MultilevelPreconditioner
on a TangentOperator, csrc/jit/multilevel_free.hip): multilevel_util.Oracle with the fine matrix taken out -- the values of level 1
summed straight from matrix_util.element_matrices by the rule of the module docstring, the nodes' own blocks and the products of
level 0 from tangent_operator_util -- and the conjugate gradients around it, the same operations in the same order: bit for bit
what the kernels compute."""

from types import SimpleNamespace

import numpy as np

import multilevel_util as MU
from matrix_util import contributions, element_matrices, pattern
from solver_util import block_inverses, diagonal_of, full_pattern, ordered_dot
from tangent_operator_util import diagonal_blocks_oracle, product_oracle

EPS = MU.EPS


def level1_values(tangent, dofmap, ref, jinv, weights, n_nodes, agg, indptr1, indices1, mask=None, chunk_cells=None, absolute=False, ke_all=None):
    """values[K][r][s] of level 1, K = (I, J): f = the number of constrained dofs D i + r among the members i of I (I == J and r == s)
    or 0.0; over the contributions (c, a, b) with agg[dofmap[c][a]] == I and agg[dofmap[c][b]] == J, ascending c*A*A + a*A + b, the
    cells in ascending chunks (a later chunk goes on from what is there): nothing where dof D dofmap[c][a] + r or D dofmap[c][b] + s
    is constrained, else f = f + ke[c][a][r][b][s].  ``absolute``: every factor of ke replaced by its absolute value (the S of the
    rounding bound; the counts are what they are); ``ke_all``: these element matrices [C][A][D][A][D] in the place of those of the tangent"""
    c_, a_ = dofmap.shape
    q_, _, d_ = ref.shape
    n_agg = indptr1.size - 1
    agg = np.asarray(agg, dtype=np.int64)
    values = np.zeros((indices1.size, d_, d_))
    m = np.zeros((n_nodes, d_), dtype=bool) if mask is None else mask.reshape(n_nodes, d_)
    rows1 = np.repeat(np.arange(n_agg), np.diff(indptr1))
    for k in np.flatnonzero(rows1 == indices1):
        held = m[agg == rows1[k]].sum(axis=0)  # per direction r
        values[k][np.arange(d_), np.arange(d_)] = held.astype(np.float64)
    coarse_dofmap = agg[dofmap]
    order, block, _ = contributions(coarse_dofmap, n_agg, indptr1.astype(np.int64), indices1.astype(np.int64))  # (ascending within a block: stable)
    cell = order // (a_ * a_)
    chunk_cells = max(c_, 1) if chunk_cells is None else chunk_cells
    cmat = None if ke_all is not None else np.asarray(tangent, dtype=np.float64).reshape(c_, -1)
    for c0 in range(0, c_, chunk_cells):
        c1 = min(c0 + chunk_cells, c_)
        ke = ke_all[c0:c1] if ke_all is not None else element_matrices(cmat[c0:c1].reshape(-1), ref, jinv[c0:c1], weights[c0:c1], absolute)
        terms = np.ascontiguousarray(ke.transpose(0, 1, 3, 2, 4)).reshape(-1, d_, d_)  # [(c - c0)*A*A + a*A + b][r][s]
        mine = np.flatnonzero((cell >= c0) & (cell < c1))  # this chunk's contributions, in list order
        blk, key = block[mine], order[mine]
        an, bn = key % (a_ * a_) // a_, key % a_
        skip = m[dofmap[cell[mine], an]][:, :, None] | m[dofmap[cell[mine], bn]][:, None, :]
        first = np.searchsorted(blk, blk, side="left")  # (blk ascends: the lists are stored block after block)
        rank = np.arange(blk.size) - first
        by_rank = np.argsort(rank, kind="stable")
        bounds = np.searchsorted(rank[by_rank], np.arange(int(rank.max()) + 2 if rank.size else 1))
        for j in range(bounds.size - 1):
            sel = by_rank[bounds[j]: bounds[j + 1]]  # every coarse block at most once: the sums of a block run in order
            at = blk[sel]
            values[at] = np.where(skip[sel], values[at], values[at] + terms[key[sel] - c0 * a_ * a_])
    return values


def longest_chain(dofmap, agg, indptr1, indices1):
    """the most terms any entry of level 1 sums: the contributions of its coarse block and, on the diagonal, the members its start
    counts"""
    n_agg = indptr1.size - 1
    _, block, _ = contributions(np.asarray(agg, dtype=np.int64)[dofmap], n_agg, indptr1.astype(np.int64), indices1.astype(np.int64))
    return int(np.bincount(block).max()) + int(np.bincount(agg).max())


def own_blocks(ke, dofmap, n_nodes, mask=None):
    """tangent_operator_util.diagonal_blocks_oracle from element matrices that exist already: de[c][a] = ke[c][a][.][a][.] added per
    node in ascending c*A + a; an entry whose row or column dof is constrained is the constant 1.0 (diagonal) or 0.0"""
    a_, d_ = ke.shape[1], ke.shape[2]
    de = np.stack([ke[:, a, :, a, :] for a in range(a_)], axis=1).reshape(-1, d_, d_)  # [c*A + a][r][s]
    flat = dofmap.reshape(-1)
    order = np.argsort(flat, kind="stable")
    node = flat[order]
    rank = np.arange(node.size) - np.searchsorted(node, node, side="left")
    out = np.zeros((n_nodes, d_, d_))
    for k in range(int(rank.max()) + 1 if rank.size else 0):
        sel = rank == k  # every node at most once: the sums of a node run in order
        out[node[sel]] = out[node[sel]] + de[order[sel]]
    if mask is not None:
        m = mask.reshape(n_nodes, d_)
        hit = m[:, :, None] | m[:, None, :]
        out[hit] = np.broadcast_to(np.eye(d_), out.shape)[hit]
    return out


class FreeOracle(MU.Oracle):
    """the preconditioner of one operator: ``setup(tangent)`` then ``apply(r)``; ``values[0]`` is None, ``values[1]`` comes from the
    element matrices, the deeper levels from multilevel_util.galerkin; ``diagonal`` are the nodes' own blocks of level 0"""

    def __init__(self, dofmap, ref, jinv, weights, n_nodes, mask=None, chunk_cells=None, **options):
        self.tables = (dofmap, ref, jinv, weights, n_nodes)
        self.chunk_cells = chunk_cells
        # (a node of no cell has a row of its own block, as the preconditioner gives it: zero, the setup singular)
        super().__init__(*pattern(full_pattern(dofmap, n_nodes)[0], n_nodes), mask=mask, **options)

    def setup(self, tangent):
        self.tangent = np.asarray(tangent, dtype=np.float64).reshape(-1)
        dofmap, ref, jinv, weights, n_nodes = self.tables
        # (the element matrices once for both: neither the blocks nor the values of level 1 depend on the chunks, which
        # tangent_operator_util.diagonal_blocks_oracle and level1_values' own chunk_cells show)
        ke = element_matrices(self.tangent, ref, jinv, weights) if self.chunk_cells is None else None
        self.diagonal = diagonal_blocks_oracle(self.tangent, *self.tables, mask=self.mask) if ke is None else own_blocks(ke, dofmap, n_nodes, self.mask)
        self.values = [None]
        if len(self.levels) > 1:
            fine, coarse = self.levels[0], self.levels[1]
            self.values.append(level1_values(self.tangent, *self.tables, fine.agg, coarse.indptr, coarse.indices, mask=self.mask, chunk_cells=self.chunk_cells,
                                             ke_all=ke))
        for lv in self.levels[1:-1]:
            self.values.append(MU.galerkin(lv.folds, self.values[-1]))
        with np.errstate(all="ignore"):
            both = [block_inverses(self.diagonal)] + [block_inverses(diagonal_of(lv.indptr, lv.indices, v)) for lv, v in zip(self.levels[1:], self.values[1:])]
        self.inv, self.det = [b[0] for b in both], [b[1] for b in both]
        self.singular = any((~(det != 0.0) | ~np.isfinite(det)).any() for det in self.det)
        return self

    def product(self, l, x):
        if l == 0:
            return product_oracle(self.tangent, x, *self.tables, mask=self.mask)
        return super().product(l, x)


def conjugate_gradient(oracle, tangent, b, x0=None, rtol=1e-8, atol=0.0, maxiter=None, setup=True):
    """what ``ConjugateGradient(A, preconditioner=MultilevelPreconditioner(A))(tangent, b)`` computes, on the bits:
    multilevel_util.conjugate_gradient with the operator's product in the matrix's place (``setup=False``: the oracle has been set up
    for this tangent already)"""
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    n = b.size
    maxiter = 10 * n if maxiter is None else maxiter
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64).reshape(-1)
    if setup:
        oracle.setup(tangent)
    status = "singular_block" if oracle.singular else "running"
    with np.errstate(all="ignore"):
        r = b.copy() if x0 is None else b - oracle.product(0, x)
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
            q = oracle.product(0, p)
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


def oracle_free_multilevel_loop(state, dofmap, ref, jinv, weights, n_nodes, rtol=1e-8, **options):
    """the ``loop`` of examples/cube_tension_matrix_free_multilevel.py on the CPU: solver_util.oracle_solve_loop with the oracle
    operator and this module's preconditioner (``options``) in the matrix's place; ``loop.systems`` keeps (tangent, rhs, result)"""
    from solver_util import oracle_solve_loop

    loop = oracle_solve_loop(state, dofmap, ref, jinv, weights, n_nodes)

    def solve():
        tangent = np.array(loop.state.tangent, dtype=np.float64).reshape(-1)
        rhs = np.where(loop.mask, 0.0, loop.f)
        result = conjugate_gradient(FreeOracle(dofmap, ref, jinv, weights, n_nodes, mask=loop.mask, **options), tangent, rhs, rtol=rtol)
        loop.systems.append((tangent, rhs, result))
        return result.x, result

    loop.solve = solve
    return loop


__all__ = ["EPS", "FreeOracle", "conjugate_gradient", "level1_values", "longest_chain", "oracle_free_multilevel_loop"]
