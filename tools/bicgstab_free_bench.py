"""BiCGStab on the matrix-free tangent operator (fenics_constitutive_amd.MatrixFreeBiCGStab) against BiCGStab on the assembled
matrix, measured on the GPU.

    python tools/bicgstab_free_bench.py [--mesh hex8 tet_p2] [--cells-per-edge 108] [--repeats 5] [--solve-repeats 3]
                                        [--out profiles/bicgstab_free_bench.json]

One process; the two meshes of tools/tangent_operator_bench.py (the unit cube, 109^3 nodes, 3.9 M dofs at the default size: hexahedra
with 2 x 2 x 2 points and per-point inverse Jacobians, 1.0e7 points; 10-node tetrahedra with 4 points, 3.8 M points), the constraints
those of the tension test, the matrix block CSR, the tangent the UNSYMMETRIC one of tests/bicgstab_util.py (non-associated, b = 0.6,
b_flow = 0, at a seeded 30 % of the points).  Everything is built and warmed up outside the timed regions; by device events, the
routes ALTERNATING repeat by repeat, median (min - max); every comparison is with the matrix route of the same run:

(a) one product with one dot ("v") and with two ("t"): the operator's element kernel and the node-dots kernel against
    ``fcamd_bcg_product_kernel`` on the assembled values;
(b) one whole iteration: a solve with ``rtol = 0`` stopped after ``--iterations`` iterations in one batch, divided by their number (the
    call's setup is in it), with block-Jacobi and with the additive cycle, either route;
(c) the whole solve at ``rtol = 1e-8`` (at most ``--maxiter`` iterations), either route, with the additive cycle and with block-Jacobi:
    iterations, status, the true residual ``|b - A x| / |b|`` by the operator's product;
(d) the setup of a call (a solve with ``maxiter = 0``): the operator route's against the assembly followed by the matrix route's;
(e) the device bytes either route allocates (``torch.cuda.memory_allocated`` around its first use).
"""

from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "examples"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

import numpy as np  # noqa: E402
from bicgstab_bench import trains  # noqa: E402
from gradient_bench import spread  # noqa: E402
from multilevel_bench import ratios, timed  # noqa: E402
from tangent_operator_bench import MESHES, build  # noqa: E402

PRECONDITIONERS = ("additive", "block_jacobi")
ROUTES = ("operator", "matrix")


def measure(mesh: str, args, rng) -> dict:
    import torch
    from bicgstab_util import nonassociated_tangent

    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd import bicgstab, bicgstab_free, jit, solver
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
    tangent = to_device(nonassociated_tangent(n), "cuda")
    b = torch.where(mask_dev, zero, to_device(rng.normal(size=nd), "cuda"))
    vec, other = to_device(rng.normal(size=nd), "cuda"), to_device(rng.normal(size=nd), "cuda")
    x_out, y = torch.empty(nd, dtype=torch.float64, device="cuda"), torch.empty(nd, dtype=torch.float64, device="cuda")
    its = args.iterations
    kw = {"batch": dict(rtol=0.0, maxiter=its, check_every=its), "setup": dict(maxiter=0), "whole": dict(rtol=1e-8, maxiter=args.maxiter)}

    # ---- the operator route, first: the tables every route shares are counted with it -------------------------------------------
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    A = fc.TangentOperator(force)
    A.set_constrained(mask)
    pc_a = fc.MultilevelPreconditioner(A, cycle="additive", coarsest_nodes=args.coarsest_nodes)
    free = {(name, kind): fc.MatrixFreeBiCGStab(A, preconditioner="block_jacobi" if kind == "block_jacobi" else pc_a, **kw[name]) for name in kw for kind in PRECONDITIONERS}
    bytes_operator = {}
    for kind in reversed(PRECONDITIONERS):  # block-Jacobi first: the shared tables come with it
        before = torch.cuda.memory_allocated()
        assert free[("batch", kind)](tangent, b, out=x_out).status == "maxiter"
        torch.cuda.synchronize()
        bytes_operator[kind] = torch.cuda.memory_allocated() - before
    # ---- the matrix route ----------------------------------------------------------------------------------------------------------
    before = torch.cuda.memory_allocated()
    K = fc.TangentMatrix(force, format="bsr")
    K.set_constrained(mask)
    values = K(tangent)
    pc_k = fc.MultilevelPreconditioner(K, cycle="additive", coarsest_nodes=args.coarsest_nodes)
    assembled = {(name, kind): fc.BiCGStab(K, preconditioner="block_jacobi" if kind == "block_jacobi" else pc_k, **kw[name]) for name in kw for kind in PRECONDITIONERS}
    bytes_matrix = {}
    for kind in reversed(PRECONDITIONERS):
        assert assembled[("batch", kind)](values, b, out=x_out).status == "maxiter"
        torch.cuda.synchronize()
        bytes_matrix[kind] = torch.cuda.memory_allocated() - before
        before = torch.cuda.memory_allocated()
    row = {"points": n, "cells": op.n_cells, "nodes": n_nodes, "dofs": nd, "blocks": K.nnzb, "levels": pc_a.levels,
           "resources": free[("batch", "block_jacobi")].resources,
           "bytes": {"tangent": 8 * 36 * n, "values": 8 * K.nnz, "assembly_scratch": 8 * K._scratch[0].numel(),
                     "allocated_by_the_operator_route": bytes_operator, "allocated_by_the_matrix_route": bytes_matrix, "before_either": base}}
    for name in ("setup", "whole"):  # warm: the work vectors of every solver (the whole solves stopped early)
        for kind in PRECONDITIONERS:
            for s, first in ((free[(name, kind)], tangent), (assembled[(name, kind)], values)):
                s.maxiter, keep = min(s.maxiter, 3), s.maxiter
                s(first, b, out=x_out)
                s.maxiter = keep

    # ---- (a) one product ---------------------------------------------------------------------------------------------------------
    s = assembled[("batch", "block_jacobi")]
    control, r, rhat, p, v, t, yk, z, inv = s._workspace(0)
    control.upload(0.0, 0.0, 1)  # status "running": the product kernels honour it
    fcontrol = bicgstab_free._product(A).control(0)
    fcontrol.upload(0.0, 0.0, 1)

    def matrix_product(dots):
        pa = bicgstab.Params()
        pa.cg = s._op.args(0, values, control)
        pa.cg.va, pa.cg.q, pa.cg.vb, pa.cg.mode = vec.data_ptr(), t.data_ptr(), other.data_ptr(), dots
        return lambda: jit.launch(s._code, 0, s._op.blocks(0), pa, "bicgstab_free_bench product launch", kernel=bicgstab.PRODUCT_KERNEL)

    def free_product(dots):
        launch = bicgstab_free._product(A).launch
        return lambda: launch(0, tangent.data_ptr(), vec.data_ptr(), y.data_ptr(), other.data_ptr(), dots, fcontrol)

    times = trains({"matrix_v": matrix_product(0), "operator_v": free_product(0), "matrix_t": matrix_product(1), "operator_t": free_product(1),
                    "operator_cg": lambda: A(tangent, vec, out=y)}, args.repeats)
    for c in (control, fcontrol):
        c.download(0)
        assert int(c.ints[solver._STATUS]) == 0, "the timed products did not run"
    row["product"] = {name: spread(ms) for name, ms in times.items()}
    for dots in ("v", "t"):
        row["product"][f"operator_{dots}"]["times_the_matrix_product"] = ratios([x / c for x, c in zip(times[f"operator_{dots}"], times[f"matrix_{dots}"])])
    row["product"]["operator_t"]["times_operator_v"] = ratios([x / c for x, c in zip(times["operator_t"], times["operator_v"])])
    same = float((y - t).abs().max() / t.abs().max())
    row["product"]["operator_against_matrix_max_relative"] = same
    print(json.dumps({mesh: {"product": row["product"]}}), flush=True)

    # ---- (b) one iteration, (d) the setup, (c) the whole solve: alternating -----------------------------------------------------------
    times = {(name, route, kind): [] for name in kw for route in ROUTES for kind in PRECONDITIONERS}
    last = {}
    for name, repeats in (("batch", args.repeats), ("setup", args.repeats), ("whole", args.solve_repeats)):
        for _ in range(repeats):
            for kind in PRECONDITIONERS:
                ms, res = timed(lambda: free[(name, kind)](tangent, b, out=x_out))
                times[name, "operator", kind].append(ms)
                true = float(torch.linalg.vector_norm(b - A(tangent, x_out, out=y)) / torch.linalg.vector_norm(b)) if name == "whole" else None
                last[name, "operator", kind] = (res, true)
                if name == "setup":  # the matrix route assembles first
                    ms, res = timed(lambda: assembled[(name, kind)](K(tangent, out=values), b, out=x_out))
                else:
                    ms, res = timed(lambda: assembled[(name, kind)](values, b, out=x_out))
                times[name, "matrix", kind].append(ms)
                true = float(torch.linalg.vector_norm(b - A(tangent, x_out, out=y)) / torch.linalg.vector_norm(b)) if name == "whole" else None
                last[name, "matrix", kind] = (res, true)
                if name == "whole":
                    print(json.dumps({mesh: {kind: {route: [round(times[name, route, kind][-1], 1), last[name, route, kind][0].iterations, last[name, route, kind][0].status]
                                                    for route in ROUTES}}}), flush=True)
    for kind in PRECONDITIONERS:
        out = row[kind] = {}
        for route in ROUTES:
            res, true = last["whole", route, kind]
            out[route] = {"iteration": {**spread([x / its for x in times["batch", route, kind]]), "iterations_per_batch": its},
                          "setup": spread(times["setup", route, kind]),
                          "solve": {**spread(times["whole", route, kind]), "iterations": res.iterations, "status": res.status, "residual_norm": res.residual_norm,
                                    "rhs_norm": res.rhs_norm, "true_residual_over_rhs": true,
                                    "ms_per_iteration": round(float(np.median(times["whole", route, kind])) / max(res.iterations, 1), 3)}}
        for name, key in (("batch", "iteration"), ("setup", "setup"), ("whole", "solve")):
            out[f"{key}_operator_over_matrix"] = ratios([x / c for x, c in zip(times[name, "operator", kind], times[name, "matrix", kind])])
    row["assembly"] = spread(trains({"assembly": lambda: K(tangent, out=values)}, args.repeats, 1)["assembly"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", nargs="+", choices=MESHES, default=list(MESHES))
    ap.add_argument("--cells-per-edge", type=int, default=108)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--maxiter", type=int, default=4000)
    ap.add_argument("--coarsest-nodes", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bicgstab_free_bench.json"))
    args = ap.parse_args()
    assert args.solve_repeats >= 3, "at least three alternated repeats"

    import torch

    assert torch.cuda.is_available(), "bicgstab_free_bench.py measures on the GPU"
    result = {"device": torch.cuda.get_device_name(0), "cells_per_edge": args.cells_per_edge, "repeats": args.repeats,
              "solve_repeats": args.solve_repeats, "rtol": 1e-8, "maxiter": args.maxiter}
    for mesh in args.mesh:
        result[mesh] = measure(mesh, args, np.random.default_rng(1))
        torch.cuda.empty_cache()
        print(json.dumps({mesh: result[mesh]}), flush=True)
        if args.out:  # (after every mesh: a run cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
