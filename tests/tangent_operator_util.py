"""Shared by the tests of the matrix-free tangent operator (fenics_constitutive_amd.tangent_operator): the ordered NumPy oracle of
csrc/jit/tangent_operator.hip composed from the oracles the operator's arithmetic is made of -- gradient_util.oracle (the
producer), force_util.tangent_action_oracle (the tangent form of the force operator), matrix_util.element_matrices (the diagonal
blocks) and solver_util.ordered_dot --, the conjugate gradients of solver_util on a product callable, inputs whose cells name
distinct nodes, and the Newton loop of examples/cube_tension_matrix_free_solve.py on the CPU."""

from types import SimpleNamespace

import numpy as np

from force_util import MANDEL_DIM, chain_length, max_valence, random_inputs, tangent_action_oracle
from gradient_util import EPS, SHAPES, _terms, oracle
from matrix_util import element_matrices
from solver_util import apply_inverse, block_inverses, ordered_dot


def distinct_inputs(shape, n_cells, seed, integer, affine, every_node=False):
    """force_util.random_inputs with a dofmap whose cells name distinct nodes (the operator refuses others): every cell a random
    choice of A of the nodes; node 0 and the last node stay in use, node ``lonely`` in the middle of the numbering is in no cell.
    ``every_node``: the nodes are renumbered so that every one is in a cell (``lonely`` is None): a system one can solve"""
    t = random_inputs(shape, n_cells, seed, integer, affine)
    d_, a_, q_, _ = SHAPES[shape] if isinstance(shape, str) else shape
    n_used = t["n_nodes"] - 1
    rng = np.random.default_rng(seed + 2000)
    dofmap = np.stack([rng.permutation(n_used)[:a_] for _ in range(n_cells)]).astype(np.int32)
    if not (dofmap == 0).any():
        dofmap[0, 0] = 0
    if not (dofmap == n_used - 1).any():
        dofmap[-1, -1] = n_used - 1
    if every_node:
        _, inverse = np.unique(dofmap, return_inverse=True)
        dofmap = inverse.reshape(dofmap.shape).astype(np.int32)
        t["n_nodes"], t["lonely"] = int(dofmap.max()) + 1, None
    else:
        dofmap = np.where(dofmap >= t["lonely"], dofmap + 1, dofmap).astype(np.int32)
    assert (np.diff(np.sort(dofmap, axis=1), axis=1) > 0).all()
    t["dofmap"] = dofmap
    t["du"] = t["du"][: d_ * t["n_nodes"]]
    return t


def random_mask(t, d_, seed, fraction=0.2, whole_cell=None):
    """random constrained dofs at the nodes that are in a cell; ``whole_cell``: every dof of that cell's nodes too"""
    used = np.bincount(t["dofmap"].reshape(-1), minlength=t["n_nodes"]) > 0
    mask = (np.random.default_rng(seed).random(d_ * t["n_nodes"]) < fraction) & np.repeat(used, d_)
    if whole_cell is not None:
        mask.reshape(-1, d_)[t["dofmap"][whole_cell]] = True
    return mask


def product_oracle(tangent, v, dofmap, ref, jinv, weights, n_nodes, mask=None, absolute=False):
    """what TangentOperator.__call__ computes, on the bits: the tangent action of the gradient of ``v`` with +0.0 at the constrained
    dofs, and ``v``'s own value there (``absolute``: every factor replaced by its absolute value -- the S of the rounding bound)"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    vm = v if mask is None else np.where(mask, 0.0, v)
    if absolute:
        g = np.ascontiguousarray(_terms(np.abs(vm), dofmap, ref, jinv, True)).reshape(-1)
    else:
        g = oracle(vm, dofmap, ref, jinv, "grad")
    y = tangent_action_oracle(tangent, g, dofmap, ref, jinv, weights, n_nodes, "grad", absolute=absolute)
    return y if mask is None else np.where(mask, np.abs(v) if absolute else v, y)


def product_chain_length(dofmap, ref, n_nodes, row_blocks):
    """roundings between the exact product and EITHER side of the comparison of the operator with the assembled matrix: the
    gradient's A + D + 2 and the tangent action's chain (force_util.chain_length) on the matrix-free side; the entry's chain and
    the D * (blocks of the longest row) + 2 of the row sum on the matrix's"""
    q_, a_, d_ = ref.shape
    valence = max_valence(dofmap, n_nodes)
    return (a_ + d_ + 2) + 2 * chain_length(d_, q_, valence, True) + d_ * row_blocks + 2


def diagonal_blocks_oracle(tangent, dofmap, ref, jinv, weights, n_nodes, mask=None, chunk_cells=None):
    """what TangentOperator.diagonal_blocks computes, on the bits: de[c][a] = ke[c][a][.][a][.] of matrix_util.element_matrices, added
    per node in ascending c*A + a, the cells in ascending chunks (a later chunk goes on from what is there); an entry whose row or
    column dof is constrained is the constant 1.0 (diagonal) or 0.0"""
    c_, a_ = dofmap.shape
    d_ = ref.shape[2]
    s_ = MANDEL_DIM[d_]
    q_ = ref.shape[0]
    out = np.zeros((n_nodes, d_, d_))
    chunk_cells = max(c_, 1) if chunk_cells is None else chunk_cells
    cmat = np.asarray(tangent, dtype=np.float64).reshape(c_, q_ * s_ * s_)
    for c0 in range(0, c_, chunk_cells):
        c1 = min(c0 + chunk_cells, c_)
        ke = element_matrices(cmat[c0:c1].reshape(-1), ref, jinv[c0:c1], weights[c0:c1])
        de = np.stack([ke[:, a, :, a, :] for a in range(a_)], axis=1).reshape(-1, d_, d_)  # [c*A + a][r][s]
        flat = dofmap[c0:c1].reshape(-1)
        order = np.argsort(flat, kind="stable")
        node = flat[order]
        rank = np.arange(node.size) - np.searchsorted(node, node, side="left")
        for k in range(int(rank.max()) + 1 if rank.size else 0):
            sel = rank == k  # every node at most once: the sums of a node run in order
            out[node[sel]] = out[node[sel]] + de[order[sel]]
    if mask is not None:
        m = mask.reshape(n_nodes, d_)
        hit = m[:, :, None] | m[:, None, :]
        out[hit] = np.broadcast_to(np.eye(d_), out.shape)[hit]
    return out


def conjugate_gradient(product, diagonal, b, x0=None, preconditioner="block_jacobi", rtol=1e-8, atol=0.0, maxiter=None):
    """solver_util.conjugate_gradient with the matrix behind a callable: ``product(p) -> K p``; ``diagonal``: the nodes' own blocks
    ``[n_nodes][D][D]`` (read with the preconditioner only).  A namespace of x, iterations, converged, status, residual_norm,
    rhs_norm, on the bits of ConjugateGradient(TangentOperator)"""
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    n = b.size
    maxiter = 10 * n if maxiter is None else maxiter
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64).reshape(-1)
    status = "running"
    inv = None
    if preconditioner is not None:
        inv, det = block_inverses(diagonal)
        if (~(det != 0.0) | ~np.isfinite(det)).any():
            status = "singular_block"
    with np.errstate(all="ignore"):
        r = b.copy() if x0 is None else b - product(x)
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
            q = product(p)
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


def operator_solve(tangent, b, dofmap, ref, jinv, weights, n_nodes, mask=None, **cg_options):
    """the oracle's ConjugateGradient(TangentOperator)(tangent, b)"""
    tables = (dofmap, ref, jinv, weights, n_nodes)
    diagonal = None
    if cg_options.get("preconditioner", "block_jacobi") is not None:
        diagonal = diagonal_blocks_oracle(tangent, *tables, mask=mask)
    return conjugate_gradient(lambda p: product_oracle(tangent, p, *tables, mask=mask), diagonal, b, **cg_options)


def oracle_free_loop(state, dofmap, ref, jinv, weights, n_nodes, **cg_options):
    """the ``loop`` of examples/cube_tension_matrix_free_solve.py on the CPU: solver_util.oracle_solve_loop with the oracle operator
    in the matrix's place; ``loop.systems`` keeps (tangent, rhs, result) of every solve"""
    from solver_util import oracle_solve_loop

    loop = oracle_solve_loop(state, dofmap, ref, jinv, weights, n_nodes)

    def solve():
        tangent = np.array(loop.state.tangent, dtype=np.float64).reshape(-1)
        rhs = np.where(loop.mask, 0.0, loop.f)
        result = operator_solve(tangent, rhs, dofmap, ref, jinv, weights, n_nodes, mask=loop.mask, **cg_options)
        loop.systems.append((tangent, rhs, result))
        return result.x, result

    loop.solve = solve
    return loop


__all__ = ["EPS", "conjugate_gradient", "diagonal_blocks_oracle", "distinct_inputs", "operator_solve", "oracle_free_loop", "product_chain_length",
           "product_oracle", "random_mask"]
