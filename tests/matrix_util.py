"""Shared by the tests of the assembled tangent stiffness (fenics_constitutive_amd.matrix): the ordered NumPy oracle of
csrc/jit/tangent_matrix.hip built from force_util's functions (same operations in the same order: bit for bit what the kernels
compute, nothing dropped), the pattern builder, the oracle's "absolute" variant for rounding bounds, and the constraint rule."""

import numpy as np

from force_util import MANDEL_DIM, element_forces, mandel_strain, stress_tensor, tangent_times_strain


def basis_gradients(ref, jinv):
    """element_forces' g[c][q][a][x]: g = 0.0; g = g + ref[q][a][k] * jinv[c(,q)][k][x], k ascending"""
    q_, a_, d_ = ref.shape
    j = jinv if jinv.ndim == 4 else jinv[:, None]
    g = np.zeros((j.shape[0], q_, a_, d_))
    for k in range(d_):
        g = g + ref[None, :, :, k, None] * j[:, :, None, k, :]
    return g


def element_matrices(tangent, ref, jinv, weights, absolute=False):
    """ke[c][a][r][b][s]: column (b, s) is the element force of the unit displacement of local node b in direction s"""
    f = np.abs if absolute else (lambda x: x)
    q_, a_, d_ = ref.shape
    c_ = weights.shape[0]
    s_ = MANDEL_DIM[d_]
    ref, jinv, weights = f(ref), f(jinv), f(weights)
    cmat = f(tangent.reshape(c_, q_, s_, s_))
    g = basis_gradients(ref, jinv)
    ke = np.zeros((c_, a_, d_, a_, d_))
    for b in range(a_):
        for s in range(d_):
            big_g = np.zeros((c_, q_, d_, d_))
            big_g[:, :, s, :] = g[:, :, b, :]
            e = mandel_strain(big_g, d_)
            sv = tangent_times_strain(cmat, e)
            ke[:, :, :, b, s] = element_forces(stress_tensor(sv, d_), ref, jinv, weights)
    return ke


def pattern(dofmap, n_nodes):
    """(indptr[n_nodes + 1], indices[nnzb]): block row v holds the ascending unique nodes u that share a cell with v"""
    d64 = dofmap.astype(np.int64)
    key = np.unique((d64[:, :, None] * n_nodes + d64[:, None, :]).reshape(-1))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(key // n_nodes, minlength=n_nodes))])
    return indptr.astype(np.int32), (key % n_nodes).astype(np.int32)


def contributions(dofmap, n_nodes, indptr, indices):
    """(order, block, rank): the contributions c*A*A + a*A + b in a stable argsort of node(a) * n_nodes + node(b), the block of
    the pattern each belongs to and its place in that block's list"""
    d64 = dofmap.astype(np.int64)
    key = (d64[:, :, None] * n_nodes + d64[:, None, :]).reshape(-1)
    order = np.argsort(key, kind="stable")
    rows = np.repeat(np.arange(n_nodes, dtype=np.int64), np.diff(indptr))
    pat = rows * n_nodes + indices
    block = np.searchsorted(pat, key[order])
    assert (pat[block] == key[order]).all(), "a cell pair is missing from the pattern"
    first = np.searchsorted(key[order], key[order], side="left")
    return order, block, np.arange(order.size) - first


def block_sums(ke, dofmap, n_nodes, indptr, indices, start=None):
    """values[k][r][s] = 0.0 (or start's value);  + ke[c][a][r][b][s] over the block's contributions in ascending c*A*A + a*A + b"""
    c_, a_, d_ = ke.shape[:3]
    nnzb = indices.size
    values = np.zeros((nnzb, d_, d_)) if start is None else np.array(start, dtype=np.float64).reshape(nnzb, d_, d_)
    order, block, rank = contributions(dofmap, n_nodes, indptr, indices)
    blocks = np.ascontiguousarray(ke.transpose(0, 1, 3, 2, 4)).reshape(-1, d_, d_)  # [c*A*A + a*A + b][r][s]
    for k in range(int(rank.max()) + 1 if rank.size else 0):
        sel = rank == k  # every block at most once: the sums of a block run in order
        values[block[sel]] = values[block[sel]] + blocks[order[sel]]
    return values


def apply_constraints(values, indptr, indices, mask):
    """every entry whose row or column dof is constrained: 1.0 on the diagonal, +0.0 elsewhere"""
    d_ = values.shape[1]
    n_nodes = indptr.size - 1
    rows = np.repeat(np.arange(n_nodes), np.diff(indptr))
    row_dof = d_ * rows[:, None, None] + np.arange(d_)[None, :, None] + np.zeros((1, 1, d_), dtype=np.int64)
    col_dof = d_ * indices.astype(np.int64)[:, None, None] + np.arange(d_)[None, None, :] + np.zeros((1, d_, 1), dtype=np.int64)
    hit = mask[row_dof] | mask[col_dof]
    out = values.copy()
    out[hit] = np.where(row_dof[hit] == col_dof[hit], 1.0, 0.0)
    return out


def matrix_oracle(tangent, dofmap, ref, jinv, weights, n_nodes, pattern_dofmap=None, start=None, absolute=False, constrained=None):
    """(indptr, indices, values[nnzb][D][D]): what TangentMatrix computes in format "bsr", on the bits"""
    indptr, indices = pattern(dofmap if pattern_dofmap is None else pattern_dofmap, n_nodes)
    ke = element_matrices(tangent, ref, jinv, weights, absolute)
    values = block_sums(ke, dofmap, n_nodes, indptr, indices, None if start is None else (np.abs(start) if absolute else start))
    if constrained is not None:
        values = apply_constraints(values, indptr, indices, constrained)
    return indptr, indices, values


def to_bsr(indptr, indices, values, n_nodes):
    import scipy.sparse as sp

    d_ = values.shape[1]
    return sp.bsr_matrix((values, indices, indptr), shape=(d_ * n_nodes, d_ * n_nodes))


def csr_values(indptr, indices, values):
    """the values in the order of the scalar CSR: row D v + r holds the columns D u + s ascending"""
    d_ = values.shape[1]
    per_row = np.diff(indptr)
    out = []
    for v in range(indptr.size - 1):
        blk = values[indptr[v]: indptr[v + 1]]  # [n][r][s]
        out.append(blk.transpose(1, 0, 2).reshape(-1))  # [r][n][s]
    assert sum(x.size for x in out) == d_ * d_ * per_row.sum()
    return np.concatenate(out) if out else np.zeros(0)


def max_contributions(dofmap, n_nodes, indptr, indices):
    _, block, _ = contributions(dofmap, n_nodes, indptr, indices)
    return int(np.bincount(block).max()) if block.size else 0


def diagonal_blocks(indptr, indices, values):
    """[n_nodes][D][D]: every node's own block, zeros where the pattern has none"""
    n_nodes, d_ = indptr.size - 1, values.shape[1]
    rows = np.repeat(np.arange(n_nodes), np.diff(indptr))
    out = np.zeros((n_nodes, d_, d_))
    on = np.flatnonzero(rows == indices)
    out[rows[on]] = values[on]
    return out


def oracle_matrix_loop(state, dofmap, ref, jinv, weights, n_nodes):
    """the ``loop`` of examples/cube_tension_assembled.py on the CPU: force_util.OracleLoop plus the oracle matrix"""
    from force_util import OracleLoop

    class Loop(OracleLoop):
        def matrix(self, mask):
            indptr, indices, values = matrix_oracle(self.state.tangent, *self.tables, self.weights, self.n_nodes, constrained=mask)
            return to_bsr(indptr, indices, values, self.n_nodes), diagonal_blocks(indptr, indices, values)

    return Loop(state, dofmap, ref, jinv, weights, n_nodes)
