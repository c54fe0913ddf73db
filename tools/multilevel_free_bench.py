"""The multilevel preconditioner of the matrix-free operator against the two routes the package had, measured on the GPU.

    python tools/multilevel_free_bench.py [--mesh hex8 tet_p2] [--cells-per-edge 108] [--repeats 5] [--solve-repeats 3]
                                          [--out profiles/multilevel_free_bench.json]

One process; the two meshes of tools/tangent_operator_bench.py (the unit cube with 109^3 nodes, 3.9 M dofs at the default size:
trilinear hexahedra with 2 x 2 x 2 points and per-point inverse Jacobians, and 10-node tetrahedra with 4 points).  The tangent is
that of linear elasticity, the constraints those of the tension test, the matrix block CSR, ``rtol = 1e-8``.  Five routes:

    operator + block-Jacobi                    ConjugateGradient(A)                                             (had)
    matrix + multilevel, each cycle            ConjugateGradient(K, preconditioner=MultilevelPreconditioner(K))  (had)
    operator + multilevel, each cycle          ConjugateGradient(A, preconditioner=MultilevelPreconditioner(A))  (new)

Everything is built and warmed up outside the timed regions; by device events, the routes ALTERNATING repeat by repeat, median
(min - max):

(a) the whole solve with its iteration count, and its time per iteration;
(b) one whole iteration: a solve with ``rtol = 0`` stopped after ``--iterations`` iterations in one batch, divided by their number;
(c) the setup of a call of the new route (``pc.setup(tangent)``) and its parts, each launched alone: the element matrices (the
    element kernel over every chunk), the first-level gather (over every chunk, on the element matrices the scratch holds), the
    diagonal blocks (the operator's two kernels); "the rest" is the difference -- the deeper Galerkin steps and the inverses.  Next
    to it the setup of the matrix route: the assembly of the values followed by ``pc.setup(values)``;
(d) ``torch.cuda.memory_allocated`` around the first use of every route (its objects' device tables, buffers and work vectors).
"""

from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
from bicgstab_bench import timed, trains  # noqa: E402
from gradient_bench import spread  # noqa: E402
from solver_bench import elastic_tangent  # noqa: E402
from tangent_operator_bench import MESHES, build  # noqa: E402

CYCLES = ("additive", "multiplicative")
ROUTES = ("operator block_jacobi",) + tuple(f"matrix {c}" for c in CYCLES) + tuple(f"operator {c}" for c in CYCLES)
PARTS = {"element_matrices": "MultilevelPreconditioner element launch", "first_level_gather": "MultilevelPreconditioner first Galerkin launch"}


@contextlib.contextmanager
def only(what: str):
    """inside: of the launches that go through ``jit.launch`` only those named ``what`` happen"""
    from fenics_constitutive_amd import jit

    real = jit.launch
    jit.launch = lambda code, device, blocks, args, name, kernel=None: real(code, device, blocks, args, name, kernel=kernel) if name == what else None
    try:
        yield
    finally:
        jit.launch = real


def measure(mesh: str, args, rng) -> dict:
    import torch

    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd import jit
    from fenics_constitutive_amd.gradient import BLOCKS_PER_CU
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
    tangent = to_device(elastic_tangent(210000.0, 0.3).reshape(-1), "cuda").repeat(n)
    b = torch.where(to_device(mask, "cuda"), zero, to_device(rng.normal(size=nd), "cuda"))
    x_out = torch.empty(nd, dtype=torch.float64, device="cuda")
    its = args.iterations
    row = {"points": n, "cells": op.n_cells, "nodes": n_nodes, "dofs": nd, "bytes": {"tangent": 8 * 36 * n, "before_any_route": torch.cuda.memory_allocated()}}

    # ---- the routes, each built and used once: (d) the device bytes of its first use ------------------------------------------------
    def first_use(make):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        made = make()
        torch.cuda.synchronize()
        return made, torch.cuda.memory_allocated() - before

    A = fc.TangentOperator(force)
    A.set_constrained(mask)
    K = fc.TangentMatrix(force, format="bsr")
    K.set_constrained(mask)
    pcs, whole, batch, first = {}, {}, {}, {}
    t0 = time.perf_counter()
    for cycle in CYCLES:
        pcs[f"operator {cycle}"] = fc.MultilevelPreconditioner(A, cycle=cycle, coarsest_nodes=args.coarsest_nodes)
    row["hierarchy_and_lists_host_s"] = round((time.perf_counter() - t0) / len(CYCLES), 2)
    for cycle in CYCLES:
        pcs[f"matrix {cycle}"] = fc.MultilevelPreconditioner(K, cycle=cycle, coarsest_nodes=args.coarsest_nodes)
    row["levels"] = pcs["operator additive"].levels
    row["resources"] = {k: v for k, v in pcs["operator additive"].resources.items() if k.startswith("free_")}
    row["chunks"] = len(pcs["operator additive"]._seam.chunks())

    def solvers(route):
        on, pc = route.split()
        target = A if on == "operator" else K
        pc = pc if pc == "block_jacobi" else pcs[route]
        return (fc.ConjugateGradient(target, preconditioner=pc, rtol=1e-8, maxiter=args.maxiter),
                fc.ConjugateGradient(target, preconditioner=pc, rtol=0.0, maxiter=its, check_every=its))

    values = None
    for route in ROUTES:  # the operator's routes first: the values of the matrix do not exist yet
        if route.startswith("matrix") and values is None:
            values, row["bytes"]["values_and_assembly_scratch"] = first_use(lambda: K(tangent))
        first[route] = tangent if route.startswith("operator") else values
        whole[route], batch[route] = solvers(route)

        def use():
            res = batch[route](first[route], b, out=x_out)
            assert res.status == "maxiter" and res.iterations == its, (route, res.status, res.iterations)
            whole[route].maxiter, keep = 3, whole[route].maxiter
            assert whole[route](first[route], b, out=x_out).iterations == 3
            whole[route].maxiter = keep

        _, row["bytes"][route] = first_use(use)
    print(json.dumps({mesh: {k: row[k] for k in ("levels", "chunks", "bytes", "hierarchy_and_lists_host_s")}}), flush=True)

    # ---- (c) the setup of a call and its parts ------------------------------------------------------------------------------------
    pc = pcs["operator additive"]
    on = pc._device(0)
    seam = pc._seam
    cap = BLOCKS_PER_CU * jit.num_cu(0)

    def part(what):
        def run():
            with only(what):
                seam.galerkin(pc, 0, tangent, cap)
        return run

    parts = {"whole": lambda: pc.setup(tangent), "diagonal_blocks": lambda: A.diagonal_blocks(tangent, out=on.blocks),
             **{name: part(what) for name, what in PARTS.items()},
             "matrix_route": lambda: pcs["matrix additive"].setup(K(tangent, out=values)), "assembly": lambda: K(tangent, out=values)}
    times = trains(parts, args.repeats, 1)
    row["setup"] = {name: spread(t) for name, t in times.items()}
    row["setup"]["the_rest_median_ms"] = round(row["setup"]["whole"]["median_ms"] - sum(row["setup"][k]["median_ms"] for k in ("diagonal_blocks", *PARTS)), 3)
    print(json.dumps({mesh: {"setup": row["setup"]}}), flush=True)

    # ---- (b) one whole iteration, (a) the whole solve: alternating ------------------------------------------------------------------
    per_iteration, solves, last = {r: [] for r in ROUTES}, {r: [] for r in ROUTES}, {}
    for _ in range(args.repeats):
        for route in ROUTES:
            ms, res = timed(lambda: batch[route](first[route], b, out=x_out))
            assert res.iterations == its and res.status == "maxiter", (route, res.iterations, res.status)
            per_iteration[route].append(ms / its)
    for rep in range(args.solve_repeats):
        for route in ROUTES:
            ms, res = timed(lambda: whole[route](first[route], b, out=x_out))
            solves[route].append(ms)
            last[route] = res
            print(json.dumps({"mesh": mesh, "repeat": rep, "route": route, "ms": round(ms, 1), "iterations": res.iterations, "status": res.status}), flush=True)
    for route in ROUTES:
        res = last[route]
        row[route] = {"iteration": {**spread(per_iteration[route]), "iterations_per_batch": its},
                      "solve": {**spread(solves[route]), "iterations": res.iterations, "status": res.status, "residual_norm": res.residual_norm,
                                "rhs_norm": res.rhs_norm, "ms_per_iteration": round(float(np.median(solves[route])) / max(res.iterations, 1), 3)}}
    for cycle in CYCLES:  # the new route's solve time over each route the package had, repeat by repeat
        new = solves[f"operator {cycle}"]
        row[f"operator {cycle}"]["time_over"] = {other: [round(x / y, 3) for x, y in zip(new, solves[other])] for other in ("operator block_jacobi", f"matrix {cycle}")}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", nargs="+", choices=MESHES, default=list(MESHES))
    ap.add_argument("--cells-per-edge", type=int, default=108)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--coarsest-nodes", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multilevel_free_bench.json"))
    args = ap.parse_args()
    assert args.solve_repeats >= 3, "at least three alternated repeats"

    import torch

    assert torch.cuda.is_available(), "multilevel_free_bench.py measures on the GPU"
    result = {"device": torch.cuda.get_device_name(0), "cells_per_edge": args.cells_per_edge, "repeats": args.repeats, "solve_repeats": args.solve_repeats,
              "rtol": 1e-8, "coarsest_nodes": args.coarsest_nodes}
    for mesh in args.mesh:
        result[mesh] = measure(mesh, args, np.random.default_rng(1))
        torch.cuda.empty_cache()
        print(json.dumps({mesh: result[mesh]}), flush=True)
        if args.out:  # (written after every mesh: a run cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
