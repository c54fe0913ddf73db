"""Shared by the tests of the rigid-body coarse space on a matrix-free operator (fenics_constitutive_amd.MultilevelPreconditioner(A,
coarse_space="rigid_body") with a TangentOperator, csrc/jit/multilevel_free_rigid.hip): rigid_body_util.Oracle with the fine matrix
taken out -- the values of level 1 by the rule of the module docstring, straight from matrix_util.element_matrices with the
prolongation blocks of level 0, the nodes' own blocks and the products of level 0 from tangent_operator_util --, and the conjugate
gradients, BiCGStab and the Newton loops of the examples around it: the same operations in the same order, bit for bit what the
kernels compute."""

import numpy as np

import bicgstab_free_util as BF
import multilevel_free_util as MF
import rigid_body_util as RU
from matrix_util import contributions, element_matrices, pattern
from solver_util import diagonal_of, full_pattern
from solver_util import block_inverses as small_inverses
from tangent_operator_util import diagonal_blocks_oracle, product_oracle

EPS = RU.EPS


def level1_values(tangent, dofmap, ref, jinv, weights, n_nodes, agg, indptr1, indices1, offsets, mask=None, chunk_cells=None, absolute=False, ke_all=None):
    """values[K][r][s] of level 1, K = (I, J), Dc x Dc, with P_i = [I_D B(o_i)] of the level-0 ``offsets``:
    first chunk: f = 0.0; with a mask and I == J, over the members i of I ascending: t = 0.0; for a ascending where dof D i + a is
    constrained: t = t + P_i[a][r] * P_i[a][s]; f = f + t.  Then over the contributions (c, a, b) of the block, ascending c*A*A + a*A +
    b, the cells in ascending chunks (a later chunk goes on from what is there), i = dofmap[c][a], j = dofmap[c][b]: t = 0.0; for a'
    ascending, skipped where dof D i + a' is constrained: u = 0.0; for b' ascending, skipped where dof D j + b' is constrained: u = u +
    ke[c][a][a'][b][b'] * P_j[b'][s]; t = t + P_i[a'][r] * u; f = f + t.  ``absolute``: every factor replaced by its absolute value
    (the S of the rounding bound); ``ke_all``: these element matrices [C][A][D][A][D] in the place of those of the tangent"""
    c_, a_ = dofmap.shape
    d_ = offsets.shape[1]
    n_agg = indptr1.size - 1
    agg = np.asarray(agg, dtype=np.int64)
    p = RU.p_blocks(offsets, d_)  # [n][D][Dc]
    if absolute:
        p = np.abs(p)
    dc = p.shape[2]
    values = np.zeros((indices1.size, dc, dc))
    m = np.zeros((n_nodes, d_), dtype=bool) if mask is None else mask.reshape(n_nodes, d_)
    rows1 = np.repeat(np.arange(n_agg), np.diff(indptr1))
    with np.errstate(all="ignore"):
        if mask is not None:  # the start: every member takes part, one with no constrained dof adds 0.0
            for k in np.flatnonzero(rows1 == indices1):
                f = np.zeros((dc, dc))
                for i in np.flatnonzero(agg == rows1[k]):
                    t = np.zeros((dc, dc))
                    for a in range(d_):
                        if m[i, a]:
                            t = t + p[i, a, :, None] * p[i, a, None, :]
                    f = f + t
                values[k] = f
        order, block, _ = contributions(agg[dofmap], n_agg, indptr1.astype(np.int64), indices1.astype(np.int64))  # (ascending within a block: stable)
        cell = order // (a_ * a_)
        chunk_cells = max(c_, 1) if chunk_cells is None else chunk_cells
        cmat = None if ke_all is not None else np.asarray(tangent, dtype=np.float64).reshape(c_, -1)
        for c0 in range(0, c_, chunk_cells):
            c1 = min(c0 + chunk_cells, c_)
            ke = ke_all[c0:c1] if ke_all is not None else element_matrices(cmat[c0:c1].reshape(-1), ref, jinv[c0:c1], weights[c0:c1], absolute)
            if absolute:
                ke = np.abs(ke)
            sub = np.ascontiguousarray(ke.transpose(0, 1, 3, 2, 4)).reshape(-1, d_, d_)  # [(c - c0)*A*A + a*A + b][a'][b']
            mine = np.flatnonzero((cell >= c0) & (cell < c1))  # this chunk's contributions, in list order
            blk, key = block[mine], order[mine]
            an, bn = key % (a_ * a_) // a_, key % a_
            ni, nj = dofmap[cell[mine], an], dofmap[cell[mine], bn]
            first = np.searchsorted(blk, blk, side="left")  # (blk ascends: the lists are stored block after block)
            rank = np.arange(blk.size) - first
            by_rank = np.argsort(rank, kind="stable")
            bounds = np.searchsorted(rank[by_rank], np.arange(int(rank.max()) + 2 if rank.size else 1))
            for j in range(bounds.size - 1):
                sel = by_rank[bounds[j]: bounds[j + 1]]  # every coarse block at most once: the sums of a block run in order
                kq, pi, pj, hi, hj = sub[key[sel] - c0 * a_ * a_], p[ni[sel]], p[nj[sel]], m[ni[sel]], m[nj[sel]]
                t = np.zeros((sel.size, dc, dc))
                for ar in range(d_):
                    u = np.zeros((sel.size, dc))
                    for bc in range(d_):
                        u = np.where(hj[:, bc, None], u, u + kq[:, ar, bc, None] * pj[:, bc, :])
                    t = np.where(hi[:, ar, None, None], t, t + pi[:, ar, :, None] * u[:, None, :])
                values[blk[sel]] = values[blk[sel]] + t
    return values


def longest_chain(dofmap, agg, indptr1, indices1, d_):
    """the floating-point operations of the longest chain a term of an entry of level 1 passes through, on either route: two
    products, at most D sums in u and D in t, and the sums of f -- the contributions of its coarse block and, on the diagonal, the
    members of the start.  (The assembled route adds a term into its fine block, at most the block's contributions, and the fine
    block into the coarse one, at most the fold list: together no more than the contributions of the coarse block plus one.)"""
    return MF.longest_chain(dofmap, agg, indptr1, indices1) + 2 * d_ + 2


class FreeRigidOracle(RU.Oracle):
    """the preconditioner of one operator with the rigid-body coarse space: ``setup(tangent)`` then ``apply(r)``; ``values[0]`` is
    None, ``values[1]`` comes from the element matrices by ``level1``, the deeper levels from rigid_body_util.galerkin;
    ``diagonal`` are the nodes' own blocks of level 0.  ``level1``: the rule (the tests of the mutations put another in its place)"""

    level1 = staticmethod(level1_values)

    def __init__(self, dofmap, ref, jinv, weights, n_nodes, coordinates, mask=None, chunk_cells=None, **options):
        self.tables = (dofmap, ref, jinv, weights, n_nodes)
        self.chunk_cells = chunk_cells
        super().__init__(*pattern(full_pattern(dofmap, n_nodes)[0], n_nodes), coordinates, mask=mask, **options)

    def setup(self, tangent):
        self.tangent = np.asarray(tangent, dtype=np.float64).reshape(-1)
        dofmap, ref, jinv, weights, n_nodes = self.tables
        ke = element_matrices(self.tangent, ref, jinv, weights) if self.chunk_cells is None else None
        self.diagonal = diagonal_blocks_oracle(self.tangent, *self.tables, mask=self.mask) if ke is None else MF.own_blocks(ke, dofmap, n_nodes, self.mask)
        self.values = [None]
        if len(self.levels) > 1:
            fine, coarse = self.levels[0], self.levels[1]
            self.values.append(self.level1(self.tangent, *self.tables, fine.agg, coarse.indptr, coarse.indices, self.offsets[0], mask=self.mask,
                                           chunk_cells=self.chunk_cells, ke_all=ke))
        with np.errstate(all="ignore"):
            for l in range(1, len(self.levels) - 1):
                lv = self.levels[l]
                rows = np.repeat(np.arange(lv.indptr.size - 1), np.diff(lv.indptr))
                self.values.append(RU.galerkin(lv.folds, self.values[-1], rows, lv.indices, self.p[l]))
            both = [small_inverses(self.diagonal)] + [RU.block_inverses(diagonal_of(lv.indptr, lv.indices, v)) for lv, v in zip(self.levels[1:], self.values[1:])]
        self.inv, self.det = [b[0] for b in both], [b[1] for b in both]
        self.singular = any((~(det != 0.0) | ~np.isfinite(det)).any() for det in self.det)
        return self

    def product(self, l, x):
        if l == 0:
            return product_oracle(self.tangent, x, *self.tables, mask=self.mask)
        return super().product(l, x)


#: what ``ConjugateGradient(A, preconditioner=pc)(tangent, b)`` computes with this oracle in the preconditioner's place, on the bits
conjugate_gradient = MF.conjugate_gradient


def bicgstab(oracle, tangent, b, **options):
    """what ``MatrixFreeBiCGStab(A, preconditioner=pc)(tangent, b)`` computes, on the bits (the oracle is set up here)"""
    return BF.operator_solve(tangent, b, *oracle.tables, mask=oracle.mask, preconditioner=oracle, **options)


def oracle_loop(state, dofmap, ref, jinv, weights, n_nodes, coordinates, solver="cg", rtol=1e-8, **options):
    """the ``loop`` of examples/cube_tension_matrix_free_rigid_body.py on the CPU: solver_util.oracle_solve_loop with the oracle
    operator, this module's preconditioner (``options``) and the oracle conjugate gradients (``solver="cg"``) or BiCGStab
    (``"bicgstab"``) in the matrix's place; ``loop.systems`` keeps (tangent, rhs, result)"""
    from solver_util import oracle_solve_loop

    loop = oracle_solve_loop(state, dofmap, ref, jinv, weights, n_nodes)

    def solve():
        tangent = np.array(loop.state.tangent, dtype=np.float64).reshape(-1)
        rhs = np.where(loop.mask, 0.0, loop.f)
        o = FreeRigidOracle(dofmap, ref, jinv, weights, n_nodes, coordinates, mask=loop.mask, **options)
        result = conjugate_gradient(o, tangent, rhs, rtol=rtol) if solver == "cg" else bicgstab(o, tangent, rhs, rtol=rtol)
        loop.systems.append((tangent, rhs, result))
        return result.x, result

    loop.solve = solve
    return loop


__all__ = ["EPS", "FreeRigidOracle", "bicgstab", "conjugate_gradient", "level1_values", "longest_chain", "oracle_loop"]
