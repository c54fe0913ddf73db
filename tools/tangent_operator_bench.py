"""The matrix-free tangent operator (fenics_constitutive_amd.TangentOperator) against the routes the package had, measured on the GPU.

    python tools/tangent_operator_bench.py [--mesh hex8 tet_p2] [--cells-per-edge 108] [--repeats 5] [--solve-repeats 3]
                                           [--out profiles/tangent_operator_bench.json]

One process; two meshes of the unit cube with the same 109^3 nodes (3.9 M dofs) at the default size: trilinear hexahedra with
2 x 2 x 2 points and per-point inverse Jacobians (the cube of tools/solver_bench.py), and 10-node tetrahedra with 4 points, six
per box of 2 x 2 x 2 fine cells.  The tangent is that of linear elasticity, the constraints those of the tension test, the matrix
block CSR.  Everything is built and warmed up outside the timed regions; by device events, the variants ALTERNATING repeat by
repeat, median (min - max):

(a) one product: the fused ``A(tangent, v)``; the unfused pair ``force.tangent_action(tangent, op(v))``; ``solver.matvec(K, values, v)``;
(b) one whole conjugate-gradient iteration each way: a solve with ``rtol = 0`` stopped after ``--iterations`` iterations in one batch,
    divided by their number (block-Jacobi; the call's setup is in it);
(c) the setup of a call: the operator's diagonal blocks and their inverses (a solve with ``maxiter = 0``) against the assembly of
    the values followed by the same call on the matrix;
(d) the whole solve at ``rtol = 1e-8`` each way with its iteration count;
and the device bytes either route allocates: the values and the assembly scratch against the block array and its scratch.
"""

from __future__ import annotations

import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
from bicgstab_bench import timed, trains  # noqa: E402
from gradient_bench import hex_mesh, spread  # noqa: E402
from solver_bench import elastic_tangent  # noqa: E402

MESHES = ("hex8", "tet_p2")
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def tet_p2_reference_gradients():
    """(ref [4][10][3], weights [4]): the gradients of the quadratic basis of the reference tetrahedron -- the four vertices, then the
    midpoints of TET_EDGES -- at the four-point rule of degree 2"""
    a, b = 0.5854101966249685, 0.1381966011250105
    points = np.array([[b, b, b], [a, b, b], [b, a, b], [b, b, a]])
    dlam = np.array([[-1.0, -1.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    ref = np.empty((4, 10, 3))
    for q, x in enumerate(points):
        lam = np.array([1.0 - x.sum(), *x])
        for i in range(4):
            ref[q, i] = (4.0 * lam[i] - 1.0) * dlam[i]
        for e, (i, j) in enumerate(TET_EDGES):
            ref[q, 4 + e] = 4.0 * (lam[i] * dlam[j] + lam[j] * dlam[i])
    return ref, np.full(4, 1.0 / 24.0)


def tet_p2_mesh(m: int):
    """(nodes [(2m+1)^3][3], cells [6 m^3][10] int32): every box of an m^3 grid cut into six tetrahedra along its diagonal (one per
    order of the axes), their edge midpoints the nodes of the grid of half the spacing"""
    n1 = 2 * m + 1
    xs = np.linspace(0.0, 1.0, n1)
    nodes = np.stack(np.meshgrid(xs, xs, xs, indexing="ij"), axis=-1).reshape(-1, 3)
    base = np.stack(np.meshgrid(*(2 * np.arange(m),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    cells = []
    for perm in itertools.permutations(range(3)):
        corner = [np.zeros(3, dtype=np.int64)]
        for axis in perm:
            step = corner[-1].copy()
            step[axis] += 2
            corner.append(step)
        local = corner + [(corner[i] + corner[j]) // 2 for i, j in TET_EDGES]
        ijk = base[:, None, :] + np.array(local)[None, :, :]
        cells.append((ijk[..., 0] * n1 + ijk[..., 1]) * n1 + ijk[..., 2])
    return nodes, np.ascontiguousarray(np.concatenate(cells), dtype=np.int32)


def build(mesh: str, m: int, rng):
    """(op, force, nodes, points per cell) of the mesh at m hexahedra per edge (tetrahedra: m // 2 boxes: the same nodes)"""
    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd.gradient import hex8_reference_gradients, integration_weights, inverse_jacobians

    if mesh == "hex8":
        nodes, cells = hex_mesh(m, rng)
        ref = hex8_reference_gradients()
        x = nodes[cells]
        jinv, weights = inverse_jacobians(x, ref), integration_weights(x, ref, np.ones(8))
    else:
        nodes, cells = tet_p2_mesh(max(m // 2, 1))
        ref, w = tet_p2_reference_gradients()
        x = nodes[cells[:, :4]]
        affine = np.array([[[-1.0, -1.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]])  # the linear map of the vertices
        jinv, weights = inverse_jacobians(x, affine), integration_weights(x, affine, w)
    op = fc.DisplacementGradient(cells, ref, jinv, nodes.shape[0])
    return op, fc.InternalForce(op, weights), nodes


def measure(mesh: str, args, rng) -> dict:
    import torch

    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd import solver
    from fenics_constitutive_amd.hostio import to_device

    op, force, nodes = build(mesh, args.cells_per_edge, rng)
    n, n_nodes = op.n_points, op.n_nodes
    nd = 3 * n_nodes
    mask = np.zeros(nd, dtype=bool)
    mask[3 * np.flatnonzero((nodes[:, 2] < 1e-12) | (nodes[:, 2] > 1 - 1e-12)) + 2] = True
    origin = int(np.flatnonzero((np.abs(nodes) < 1e-12).all(axis=1))[0])
    xcorner = int(np.flatnonzero((np.abs(nodes - [1.0, 0.0, 0.0]) < 1e-12).all(axis=1))[0])
    mask[[3 * origin, 3 * origin + 1, 3 * xcorner + 1]] = True
    zero = torch.zeros((), dtype=torch.float64, device="cuda")
    mask_dev = to_device(mask, "cuda")
    tangent = to_device(elastic_tangent(210000.0, 0.3).reshape(-1), "cuda").repeat(n)
    base = torch.cuda.memory_allocated()
    A = fc.TangentOperator(force)
    A.set_constrained(mask)
    cg_a = {"batch": fc.ConjugateGradient(A, rtol=0.0, maxiter=args.iterations, check_every=args.iterations),
            "setup": fc.ConjugateGradient(A, maxiter=0), "whole": fc.ConjugateGradient(A, rtol=1e-8, maxiter=args.maxiter)}
    b = torch.where(mask_dev, zero, to_device(rng.normal(size=nd), "cuda"))
    v = to_device(rng.normal(size=nd), "cuda")
    y, x_out = torch.empty(nd, dtype=torch.float64, device="cuda"), torch.empty(nd, dtype=torch.float64, device="cuda")
    after_vectors = torch.cuda.memory_allocated()
    assert cg_a["setup"](tangent, b, out=x_out).status == "maxiter"
    operator_bytes = torch.cuda.memory_allocated() - after_vectors  # the block array, its scratch, one set of work vectors
    K = fc.TangentMatrix(force, format="bsr")
    K.set_constrained(mask)
    before = torch.cuda.memory_allocated()
    values = K(tangent)
    cg_k = {"batch": fc.ConjugateGradient(K, rtol=0.0, maxiter=args.iterations, check_every=args.iterations),
            "setup": fc.ConjugateGradient(K, maxiter=0), "whole": fc.ConjugateGradient(K, rtol=1e-8, maxiter=args.maxiter)}
    assert cg_k["setup"](values, b, out=x_out).status == "maxiter"
    matrix_bytes = torch.cuda.memory_allocated() - before  # the values, the assembly scratch, one set of work vectors
    grad = torch.empty(9 * n, dtype=torch.float64, device="cuda")
    row = {"points": n, "cells": op.n_cells, "nodes": n_nodes, "dofs": nd, "blocks": K.nnzb, "resources": A.resources,
           "bytes": {"tangent": 8 * 36 * n, "values": 8 * K.nnz, "assembly_scratch": 8 * K._scratch[0].numel(), "block_array": 8 * 9 * n_nodes,
                     "block_scratch": 8 * A._scratch[0].numel(), "saved_exactly": 8 * K.nnz + 8 * K._scratch[0].numel(),
                     "allocated_by_the_operator_route": operator_bytes, "allocated_by_the_matrix_route": matrix_bytes, "before_either": base}}
    # what the fused product computes is what the pair computes
    vm = torch.where(mask_dev, zero, v)
    pair = torch.where(mask_dev, v, force.tangent_action(tangent, op(vm, out=grad)))
    row["fused_equals_pair_on_the_bits"] = bool(torch.equal(A(tangent, v, out=y).view(torch.int64), pair.view(torch.int64)))
    row["fused_against_matvec_max_relative"] = float((y - solver.matvec(K, values, v)).abs().max() / y.abs().max())
    del pair, vm

    # ---- (a) one product -------------------------------------------------------------------------------------------------------
    products = trains({"fused": lambda: A(tangent, v, out=y), "pair": lambda: force.tangent_action(tangent, op(v, out=grad), out=y),
                       "matvec": lambda: solver.matvec(K, values, v, out=y)}, args.repeats)
    row["product"] = {name: spread(t) for name, t in products.items()}
    # ---- (b) one iteration, (c) the setup, (d) the whole solve: alternating ------------------------------------------------------
    its = args.iterations
    for name in ("batch", "setup", "whole"):
        for route, cg, first in (("operator", cg_a, tangent), ("matrix", cg_k, values)):
            cg[name](first, b, out=x_out)  # warm: the work vectors of this solver
    times = {(name, route): [] for name in ("batch", "setup", "whole") for route in ("operator", "matrix")}
    last = {}
    for name, repeats in (("batch", args.repeats), ("setup", args.repeats), ("whole", args.solve_repeats)):
        for _ in range(repeats):
            ms, res = timed(lambda: cg_a[name](tangent, b, out=x_out))
            times[name, "operator"].append(ms)
            last[name, "operator"] = res
            if name == "setup":  # the matrix route assembles first
                ms, res = timed(lambda: cg_k[name](K(tangent, out=values), b, out=x_out))
            else:
                ms, res = timed(lambda: cg_k[name](values, b, out=x_out))
            times[name, "matrix"].append(ms)
            last[name, "matrix"] = res
    for route in ("operator", "matrix"):
        res = last["whole", route]
        row[route] = {"iteration": {**spread([t / its for t in times["batch", route]]), "iterations_per_batch": its},
                      "setup": spread(times["setup", route]),
                      "solve": {**spread(times["whole", route]), "iterations": res.iterations, "status": res.status, "residual_norm": res.residual_norm}}
    row["assembly"] = spread(trains({"assembly": lambda: K(tangent, out=values)}, args.repeats, 1)["assembly"])
    row["diagonal_blocks"] = spread(trains({"blocks": lambda: A.diagonal_blocks(tangent, out=cg_a["setup"]._diagonal_blocks(0))}, args.repeats, 1)["blocks"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", nargs="+", choices=MESHES, default=list(MESHES))
    ap.add_argument("--cells-per-edge", type=int, default=108)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tangent_operator_bench.json"))
    args = ap.parse_args()
    assert args.solve_repeats >= 3, "at least three alternated repeats"

    import torch

    assert torch.cuda.is_available(), "tangent_operator_bench.py measures on the GPU"
    result = {"device": torch.cuda.get_device_name(0), "cells_per_edge": args.cells_per_edge, "repeats": args.repeats,
              "solve_repeats": args.solve_repeats, "rtol": 1e-8}
    for mesh in args.mesh:
        result[mesh] = measure(mesh, args, np.random.default_rng(1))
        torch.cuda.empty_cache()
        print(json.dumps({mesh: result[mesh]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
