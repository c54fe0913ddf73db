"""Shared by the tests of the force operator (fenics_constitutive_amd.force): the ordered NumPy oracle of
csrc/jit/internal_force.hip (same operations in the same order: bit for bit what the kernels compute), its rounding bound, random
inputs on the tables of gradient_util.random_tables, and a conforming mesh of sheared tetrahedra."""

import itertools

import numpy as np

from gradient_util import EPS, SHAPES, random_tables

#: the double of sqrt(0.5); 1/sqrt(2.0) is one unit in the last place below
H = float(np.array([0x3FE6A09E667F3BCD], dtype=np.uint64).view(np.float64)[0])
assert H == np.sqrt(0.5) and H != 1.0 / np.sqrt(2.0)
MANDEL_DIM = {1: 1, 2: 4, 3: 6}
PAIRS = ((0, 1), (0, 2), (1, 2))


def n_pairs(d_):
    return {1: 0, 2: 1, 3: 3}[d_]


def stress_tensor(s, d_):
    """T[..][i][i] = s[i];  T[..][i][j] = T[..][j][i] = s[3 + m] * H  (the zz entry of D = 2 is not read)"""
    t = np.zeros(s.shape[:-1] + (d_, d_))
    for i in range(d_):
        t[..., i, i] = s[..., i]
    for m in range(n_pairs(d_)):
        i, j = PAIRS[m]
        t[..., i, j] = t[..., j, i] = s[..., 3 + m] * H
    return t


def mandel_strain(g, d_):
    """e of G[..][r][x] = d v_r / d x_x: (G00, G11, G22, H*(G01+G10), H*(G02+G20), H*(G12+G21)); D = 2: (G00, G11, 0.0, H*(G01+G10))"""
    e = np.zeros(g.shape[:-2] + (MANDEL_DIM[d_],))
    for i in range(d_):
        e[..., i] = g[..., i, i]
    for m in range(n_pairs(d_)):
        i, j = PAIRS[m]
        e[..., 3 + m] = H * (g[..., i, j] + g[..., j, i])
    return e


def tangent_times_strain(tangent, e):
    """s[i] = 0.0;  s[i] = s[i] + tangent[..][i][j] * e[j], j ascending"""
    s = np.zeros(e.shape)
    for j in range(e.shape[-1]):
        s = s + tangent[..., :, j] * e[..., None, j]
    return s


def element_forces(t, ref, jinv, weights):
    """fe[c][a][r] from T[c][q][r][x]: g = 0.0; g = g + ref * jinv over k; t = 0.0; t = t + T * g over x; fe = fe + t * w over q"""
    c_, q_, d_, _ = t.shape
    a_ = ref.shape[1]
    j = jinv if jinv.ndim == 4 else jinv[:, None]  # [c][q or 1][k][x]
    g = np.zeros((c_, q_, a_, d_))  # [c][q][a][x]
    for k in range(d_):
        g = g + ref[None, :, :, k, None] * j[:, :, None, k, :]
    fe = np.zeros((c_, a_, d_))
    for q in range(q_):
        tr = np.zeros((c_, a_, d_))
        for x in range(d_):
            tr = tr + t[:, q, None, :, x] * g[:, q, :, None, x]
        fe = fe + tr * weights[:, q, None, None]
    return fe


def node_sums(fe, dofmap, n_nodes, start=None):
    """f[D*v + r] = 0.0 (or start's value);  f = f + fe[c][a][r] over the (c, a) of node v in ascending c*A + a"""
    d_ = fe.shape[2]
    f = np.zeros((n_nodes, d_)) if start is None else np.array(start, dtype=np.float64).reshape(n_nodes, d_)
    flat = dofmap.reshape(-1)
    order = np.argsort(flat, kind="stable")
    node = flat[order]
    first = np.searchsorted(node, node, side="left")
    rank = np.arange(node.size) - first
    rows = fe.reshape(-1, d_)
    for k in range(int(rank.max()) + 1 if rank.size else 0):
        sel = rank == k  # every node at most once: the sums of a node run in order
        f[node[sel]] = f[node[sel]] + rows[order[sel]]
    return f.reshape(-1)


def max_valence(dofmap, n_nodes):
    return int(np.bincount(dofmap.reshape(-1), minlength=n_nodes).max()) if dofmap.size else 0


def _gradient_matrix(grad_v, d_, layout):
    g = grad_v.reshape(-1, d_, d_)
    return g.transpose(0, 2, 1) if layout == "nabla_grad" else g


def force_oracle(stress, dofmap, ref, jinv, weights, n_nodes, start=None, absolute=False):
    """what InternalForce.__call__ computes, on the bits (``absolute``: every factor replaced by its absolute value -- the S of
    the rounding bound)"""
    f = np.abs if absolute else (lambda x: x)
    c_, q_, d_ = dofmap.shape[0], ref.shape[0], ref.shape[2]
    t = stress_tensor(f(stress.reshape(c_, q_, MANDEL_DIM[d_])), d_)
    return node_sums(element_forces(t, f(ref), f(jinv), f(weights)), dofmap, n_nodes, None if start is None else f(start))


def tangent_action_oracle(tangent, grad_v, dofmap, ref, jinv, weights, n_nodes, layout="nabla_grad", start=None, absolute=False):
    """what InternalForce.tangent_action computes, on the bits"""
    f = np.abs if absolute else (lambda x: x)
    c_, q_, d_ = dofmap.shape[0], ref.shape[0], ref.shape[2]
    s_ = MANDEL_DIM[d_]
    e = mandel_strain(f(_gradient_matrix(grad_v, d_, layout)), d_)
    s = tangent_times_strain(f(tangent.reshape(-1, s_, s_)), e)
    t = stress_tensor(s.reshape(c_, q_, s_), d_)
    return node_sums(element_forces(t, f(ref), f(jinv), f(weights)), dofmap, n_nodes, None if start is None else f(start))


def chain_length(d_, q_, valence, action=False):
    """2D + Q + V + 4 roundings in the chain of one entry (D products and sums for g, D for t, Q for the cell sum, V for the node
    sum, the products with H and w and two for the inputs' own rounding); S + 3 more for s = C e and the strain"""
    return 2 * d_ + q_ + valence + 4 + ((MANDEL_DIM[d_] + 3) if action else 0)


def force_bound(stress, dofmap, ref, jinv, weights, n_nodes):
    s = force_oracle(stress, dofmap, ref, jinv, weights, n_nodes, absolute=True)
    return chain_length(ref.shape[2], ref.shape[0], max_valence(dofmap, n_nodes)) * EPS * s


def tangent_action_bound(tangent, grad_v, dofmap, ref, jinv, weights, n_nodes, layout="nabla_grad"):
    s = tangent_action_oracle(tangent, grad_v, dofmap, ref, jinv, weights, n_nodes, layout, absolute=True)
    return chain_length(ref.shape[2], ref.shape[0], max_valence(dofmap, n_nodes), True) * EPS * s


def random_inputs(shape, n_cells, seed, integer, affine):
    """gradient_util.random_tables plus weights, stress, an unsymmetric tangent and a gradient; one more node than the tables use,
    in the middle of the numbering, that no cell touches (node 0 and the last node stay in use)"""
    du, dofmap, ref, jinv, n_nodes = random_tables(shape, n_cells, seed, integer, affine)
    d_, a_, q_, _ = SHAPES[shape] if isinstance(shape, str) else shape
    s_ = MANDEL_DIM[d_]
    lonely = n_nodes // 2
    dofmap = np.where(dofmap >= lonely, dofmap + 1, dofmap).astype(np.int32)  # node `lonely` of n_nodes + 1 is in no cell
    n_nodes += 1
    rng = np.random.default_rng(seed + 1000)
    n = n_cells * q_
    if integer:
        weights = rng.choice(np.array([0.25, 0.5, 1.0, 2.0]), size=(n_cells, q_))
        stress = rng.integers(-8, 9, size=s_ * n).astype(np.float64)
        tangent = rng.integers(-4, 5, size=s_ * s_ * n).astype(np.float64)
        grad_v = rng.integers(-8, 9, size=d_ * d_ * n).astype(np.float64)
    else:
        weights = rng.uniform(0.5, 1.5, size=(n_cells, q_)) * 1e-3
        stress = rng.normal(scale=100.0, size=s_ * n)
        tangent = rng.normal(scale=1e4, size=s_ * s_ * n)
        grad_v = rng.normal(scale=1e-3, size=d_ * d_ * n)
    return dict(dofmap=dofmap, ref=ref, jinv=jinv, n_nodes=n_nodes, weights=weights, stress=stress, tangent=tangent, grad_v=grad_v,
                lonely=lonely, du=np.concatenate([du, np.zeros(d_)]))


def cell_counts(w, q):
    """1, W - 1, W, W + 1, 2W + 1 cells and the count giving about 257 points (W: the shape's cells per tile)"""
    return sorted({1, max(w - 1, 1), w, w + 1, 2 * w + 1, -(-257 // q)})


# ---- a conforming mesh of sheared tetrahedra ------------------------------------------------------------------------------------
def kuhn_tets(nx, ny, nz, shear, jitter=0.0, seed=0):
    """(nodes [N][3], cells [C][4], interior node numbers): every box of an nx x ny x nz grid split into six tetrahedra (one per
    order of the axes, all along the box diagonal), the interior nodes moved by ``jitter`` times the
    grid spacing at random and all nodes mapped by the matrix ``shear`` -- the mesh stays conforming and fills the sheared box"""
    rng = np.random.default_rng(seed)
    grid = np.stack(np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), np.arange(nz + 1), indexing="ij"), axis=-1).reshape(-1, 3)
    nid = np.arange(grid.shape[0]).reshape(nx + 1, ny + 1, nz + 1)
    cells = []
    for i, j, k in itertools.product(range(nx), range(ny), range(nz)):
        for perm in itertools.permutations(range(3)):
            v = np.array([i, j, k])
            tet = [nid[tuple(v)]]
            for axis in perm:
                v = v.copy()
                v[axis] += 1
                tet.append(nid[tuple(v)])
            cells.append(tet)
    x = grid / np.array([nx, ny, nz], dtype=np.float64)
    interior = np.flatnonzero(((grid > 0) & (grid < np.array([nx, ny, nz]))).all(axis=1))
    x[interior] += jitter * rng.uniform(-1.0, 1.0, size=(interior.size, 3)) / np.array([nx, ny, nz])
    return x @ np.asarray(shear).T, np.array(cells, dtype=np.int32), interior


# ---- the matrix-free loop on the CPU ---------------------------------------------------------------------------------------------
class OracleLoop:
    """the ``loop`` of examples/cube_tension_matrix_free.py on the CPU: the ordered oracles of the producer and of the force
    operator around a law with the reference's interface (fe_mini.OracleLaw) under fe_mini's copy protocol"""

    def __init__(self, state, dofmap, ref, jinv, weights, n_nodes, layout="grad"):
        self.state, self.tables, self.weights, self.n_nodes, self.layout = state, (dofmap, ref, jinv), weights, n_nodes, layout

    def residual(self, t, del_t, du):
        from gradient_util import oracle

        self.state.evaluate(t, del_t, oracle(du, *self.tables, self.layout))
        return force_oracle(self.state.stress, *self.tables, self.weights, self.n_nodes)

    def tangent_action(self, v):
        from gradient_util import oracle

        return tangent_action_oracle(self.state.tangent, oracle(v, *self.tables, self.layout), *self.tables, self.weights, self.n_nodes, self.layout)

    def commit(self):
        self.state.commit()
