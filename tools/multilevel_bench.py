"""The multilevel preconditioner (fenics_constitutive_amd.MultilevelPreconditioner) against block-Jacobi, measured on the GPU.

    python tools/multilevel_bench.py [--cells-per-edge 108] [--repeats 5] [--solve-repeats 3] [--out profiles/multilevel_bench.json]

One process, the cube of tools/solver_bench.py (trilinear hexahedra, 2 x 2 x 2 points, per-point inverse Jacobians; 108 cells per
edge: 1 295 029 nodes, 3.9 M dofs), the tangent that of linear elasticity, the constraints those of the tension test, block CSR.
Every solver is built once and warmed up (kernels loaded, vectors allocated) outside the timed regions; by device events, median
(min - max):

(a) the hierarchy: its levels and the host time of its construction (once per pattern);
(b) the setup of a call: the Galerkin values of the coarse levels and the inverses of every level;
(c) one application of each cycle with the setup done (the launches of ``z = M^-1 r`` alone) next to one matrix-vector product;
(d) one whole iteration: a solve with ``rtol = 0`` stopped after ``--iterations`` iterations in one batch, divided by their number
    (the call's setup is in it: the inverse kernel under block-Jacobi, (b) under a cycle);
(e) the whole solve at ``rtol = 1e-8`` with its iteration count: block-Jacobi, additive and multiplicative ALTERNATING, repeat by
    repeat, and the ratio of block-Jacobi's time to each cycle's, repeat by repeat (median and range).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
from force_bench import train  # noqa: E402
from gradient_bench import hex_mesh, spread  # noqa: E402
from solver_bench import elastic_tangent  # noqa: E402

SOLVERS = ("block_jacobi", "additive", "multiplicative")


def timed(fn):
    """(ms by device events around ``fn()``, what it returned)"""
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def ratios(xs):
    return {"each": [round(x, 3) for x in xs], "median": round(float(np.median(xs)), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells-per-edge", type=int, default=108)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--coarsest-nodes", type=int, default=64)
    ap.add_argument("--omega", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multilevel_bench.json"))
    args = ap.parse_args()
    assert args.solve_repeats >= 3, "at least three alternated repeats"

    import torch

    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd import solver
    from fenics_constitutive_amd.gradient import hex8_reference_gradients, integration_weights, inverse_jacobians
    from fenics_constitutive_amd.hostio import to_device

    assert torch.cuda.is_available(), "multilevel_bench.py measures on the GPU"
    m = args.cells_per_edge
    rng = np.random.default_rng(1)
    nodes, cells = hex_mesh(m, rng)
    ref = hex8_reference_gradients()
    x = nodes[cells]
    op = fc.DisplacementGradient(cells, ref, inverse_jacobians(x, ref), nodes.shape[0])
    force = fc.InternalForce(op, integration_weights(x, ref, np.ones(8)))
    del x
    n, n_nodes = op.n_points, op.n_nodes
    nd = 3 * n_nodes
    mask = np.zeros(nd, dtype=bool)
    mask[3 * np.flatnonzero((nodes[:, 2] < 1e-12) | (nodes[:, 2] > 1 - 1e-12)) + 2] = True
    origin = int(np.flatnonzero((np.abs(nodes) < 1e-12).all(axis=1))[0])
    xcorner = int(np.flatnonzero((np.abs(nodes - [1.0, 0.0, 0.0]) < 1e-12).all(axis=1))[0])
    mask[[3 * origin, 3 * origin + 1, 3 * xcorner + 1]] = True
    tangent = to_device(elastic_tangent(210000.0, 0.3).reshape(-1), "cuda").repeat(n)
    K = fc.TangentMatrix(force, format="bsr")
    K.set_constrained(mask)
    values = K(tangent)
    torch.cuda.synchronize()
    K._scratch.clear()  # (the element matrices of the assembly: not needed again)
    del tangent
    b = torch.where(to_device(mask, "cuda"), torch.zeros((), dtype=torch.float64, device="cuda"), to_device(rng.normal(size=nd), "cuda"))
    x_out = torch.empty(nd, dtype=torch.float64, device="cuda")
    result = {"points": n, "nodes": n_nodes, "dofs": nd, "blocks": K.nnzb, "format": "bsr", "repeats": args.repeats, "solve_repeats": args.solve_repeats,
              "device": torch.cuda.get_device_name(0), "omega": args.omega, "coarsest_nodes": args.coarsest_nodes, "rtol": 1e-8}

    # ---- (a) the hierarchy -----------------------------------------------------------------------------------------------------
    pcs = {}
    for cycle in SOLVERS[1:]:
        t0 = time.perf_counter()
        pcs[cycle] = fc.MultilevelPreconditioner(K, cycle=cycle, omega=args.omega, coarsest_nodes=args.coarsest_nodes)
        result.setdefault("hierarchy_host_s", round(time.perf_counter() - t0, 2))
    result["levels"] = pcs["additive"].levels
    result["resources"] = pcs["additive"].resources
    print(json.dumps({k: result[k] for k in ("levels", "hierarchy_host_s")}), flush=True)

    def cg(pc, **kw):
        return fc.ConjugateGradient(K, preconditioner=pc if pc == "block_jacobi" else pcs[pc], **kw)

    # ---- warm-up: every program loaded, every vector allocated -------------------------------------------------------------------
    # the solvers are built once, outside every timed region; their first call allocates the work vectors and loads the kernels
    its = args.iterations
    batch = {pc: cg(pc, rtol=0.0, maxiter=its, check_every=its) for pc in SOLVERS}
    whole = {pc: cg(pc, rtol=1e-8, maxiter=args.maxiter) for pc in SOLVERS}
    for pc in SOLVERS:
        res = batch[pc](values, b, out=x_out)
        assert res.status == "maxiter", (pc, res.status)
        whole[pc].maxiter, keep = 3, whole[pc].maxiter
        assert whole[pc](values, b, out=x_out).iterations == 3
        whole[pc].maxiter = keep

    # ---- (b) the setup, (c) one application -------------------------------------------------------------------------------------
    p = to_device(rng.normal(size=nd), "cuda")
    result["matvec"] = spread(train(lambda: solver.matvec(K, values, p, out=x_out), args.repeats, 5))
    for cycle, pc in pcs.items():
        row = {"setup": spread(train(lambda: pc.setup(values), args.repeats, 5))}
        control = pc._own_control(0)
        pc._setup(0, values, control)
        row["application"] = spread(train(lambda: pc._cycle(0, values, control, b.data_ptr(), x_out.data_ptr()), args.repeats, 5))
        row["application"]["times_the_matvec"] = round(row["application"]["median_ms"] / result["matvec"]["median_ms"], 2)
        result[cycle] = row
        print(json.dumps({cycle: row}), flush=True)
    result["block_jacobi"] = {}

    # ---- (d) one whole iteration -------------------------------------------------------------------------------------------------
    per_iteration = {pc: [] for pc in SOLVERS}
    for _ in range(args.repeats):
        for pc in SOLVERS:
            ms, res = timed(lambda: batch[pc](values, b, out=x_out))
            assert res.iterations == its and res.status == "maxiter", (pc, res.iterations, res.status)
            per_iteration[pc].append(ms / its)
    for pc in SOLVERS:
        result[pc]["iteration"] = {**spread(per_iteration[pc]), "iterations_per_batch": its}

    # ---- (e) the whole solve, alternating -----------------------------------------------------------------------------------------
    solves = {pc: [] for pc in SOLVERS}
    last = {}
    for rep in range(args.solve_repeats):
        for pc in SOLVERS:
            ms, res = timed(lambda: whole[pc](values, b, out=x_out))
            solves[pc].append(ms)
            last[pc] = res
            print(json.dumps({"repeat": rep, "solver": pc, "ms": round(ms, 1), "iterations": res.iterations, "status": res.status}), flush=True)
    for pc in SOLVERS:
        res = last[pc]
        result[pc]["solve"] = {**spread(solves[pc]), "iterations": res.iterations, "status": res.status, "residual_norm": res.residual_norm, "rhs_norm": res.rhs_norm,
                               "ms_per_iteration": round(float(np.median(solves[pc])) / max(res.iterations, 1), 3)}
    for pc in SOLVERS[1:]:
        result[pc]["speedup_over_block_jacobi"] = ratios([j / c for j, c in zip(solves["block_jacobi"], solves[pc])])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
