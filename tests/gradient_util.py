"""Shared by the tests of the gradient producer (fenics_constitutive_amd.gradient): the shape list, the ordered NumPy oracle of
csrc/jit/displacement_gradient.hip (same operations in the same order: bit for bit what the kernel computes), the oracle's
rounding bound, and small meshes."""

import numpy as np

#: name -> (D, A, Q, the natural form of the inverse Jacobians is per cell)
SHAPES = {
    "hex8": (3, 8, 8, False),
    "tet_p1": (3, 4, 1, True),
    "tet_p2": (3, 10, 4, True),
    "q5": (3, 4, 5, True),  # a Q that does not divide 64: cells straddle tile boundaries
    "tri_p2": (2, 6, 3, True),
    "interval": (1, 2, 1, True),
}
LAYOUTS = ("nabla_grad", "grad")
EPS = 2.0**-52


def _terms(du, dofmap, ref, jinv, absolute):
    f = np.abs if absolute else (lambda x: x)
    c_, a_ = dofmap.shape
    q_, _, d_ = ref.shape
    u = f(du.reshape(-1, d_)[dofmap])  # [c][a][r]
    ref = f(ref)
    r = np.zeros((c_, q_, d_, d_))  # [c][q][r][k]
    for a in range(a_):
        r = r + u[:, None, a, :, None] * ref[None, :, a, None, :]
    j = f(jinv if jinv.ndim == 4 else jinv[:, None])  # [c][q or 1][k][x]
    g = np.zeros((c_, q_, d_, d_))  # [c][q][r][x]
    for k in range(d_):
        g = g + r[:, :, :, k, None] * j[:, :, None, k, :]
    return g


def oracle(du, dofmap, ref, jinv, layout="nabla_grad"):
    """R = 0.0; R = R + du * ref over the nodes in order; G = 0.0; G = G + R * jinv over k in order (every product and every sum
    rounded on its own, as the kernel's with -ffp-contract=off); flat [D*D n_points]"""
    g = _terms(du, dofmap, ref, jinv, False)
    if layout == "nabla_grad":
        g = g.transpose(0, 1, 3, 2)
    return np.ascontiguousarray(g).reshape(-1)


def rounding_bound(du, dofmap, ref, jinv, layout="nabla_grad"):
    """(A + D + 2) 2^-52 S per entry, S the oracle's expression with the absolute value of every factor: A + D sums and products
    in a chain (each at most one unit in the last place of a partial sum bounded by S), two more for the inputs' own rounding"""
    s = _terms(du, dofmap, ref, jinv, True)
    if layout == "nabla_grad":
        s = s.transpose(0, 1, 3, 2)
    return (dofmap.shape[1] + ref.shape[2] + 2) * EPS * np.ascontiguousarray(s).reshape(-1)


def cell_counts(q):
    """cells giving 1 cell, the multiple of Q below 64 points, the one at or above, one tile plus a cell, and about 257 points"""
    up = -(-64 // q)
    return sorted({1, max(63 // q, 1), up, up + 1, -(-257 // q)})


def random_tables(shape, n_cells, seed, integer, affine):
    """(du, dofmap, ref, jinv, n_nodes) without geometric meaning: cells share nodes, node 0 and node n_nodes - 1 are both used.
    ``integer``: small integers (jinv: integers and powers of two) -- every product and sum of the oracle is exact"""
    d_, a_, q_, _ = SHAPES[shape] if isinstance(shape, str) else shape
    rng = np.random.default_rng(seed)
    n_nodes = max(a_ + 1, (n_cells * a_) // 3 + 2)
    dofmap = rng.integers(0, n_nodes, size=(n_cells, a_)).astype(np.int32)
    dofmap[0, 0] = 0
    dofmap[-1, -1] = n_nodes - 1
    jshape = (n_cells, d_, d_) if affine else (n_cells, q_, d_, d_)
    if integer:
        du = rng.integers(-8, 9, size=d_ * n_nodes).astype(np.float64)
        ref = rng.integers(-4, 5, size=(q_, a_, d_)).astype(np.float64)
        jinv = rng.choice(np.array([-3.0, -2.0, -1.0, -0.5, 0.25, 0.5, 1.0, 2.0, 3.0, 4.0]), size=jshape)
    else:
        du = rng.normal(scale=1e-3, size=d_ * n_nodes)
        ref = rng.normal(size=(q_, a_, d_))
        jinv = rng.normal(scale=4.0, size=jshape)
    return du, dofmap, ref, np.ascontiguousarray(jinv), n_nodes


# ---- meshes with a geometry ----------------------------------------------------------------------------------------------------
TET_P1_REFERENCE_GRADIENTS = np.array([[[-1.0, -1.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]])  # [1][4][3]


def cube_operator_tables(mesh):
    """(dofmap, ref, jinv) of an examples/fe_mini.py Cube (per-point inverse Jacobians)"""
    from fenics_constitutive_amd.gradient import hex8_reference_gradients, inverse_jacobians

    ref = hex8_reference_gradients()
    dofmap = np.ascontiguousarray(mesh.cells, dtype=np.int32)
    return dofmap, ref, inverse_jacobians(mesh.nodes[mesh.cells], ref)
