"""The rigid-body coarse space of the multilevel preconditioner against the translation hierarchy and block-Jacobi, measured on the GPU.

    python tools/rigid_body_bench.py [--cells-per-edge 108] [--repeats 5] [--solve-repeats 3] [--out profiles/rigid_body_bench.json]

One process, the cube of tools/multilevel_bench.py and tools/bicgstab_bench.py (trilinear hexahedra, 2 x 2 x 2 points, per-point
inverse Jacobians; 108 cells per edge: 1 295 029 nodes, 3.9 M dofs), the constraints those of the tension test, block CSR.  Under
conjugate gradients the values are those of linear elasticity, under BiCGStab the unsymmetric system of bicgstab_bench.py (the
non-associated tangent at 30 % of the points).  The contenders: block-Jacobi, and the additive and the multiplicative cycle over
the translation hierarchy and over the rigid-body one.  Everything is built once and warmed up (kernels loaded, vectors allocated)
outside the timed regions; by device events:

(a) the hierarchies: their levels, dofs per node and value memory (6 x 6 blocks hold four times the values of 3 x 3 ones), and the
    host time of their construction (once per pattern);
(b) the setup of a call: the Galerkin values of the coarse levels and the inverses of every level, median (min - max);
(c) the whole solve at ``rtol = 1e-8``: iterations, time per solve and per iteration, the contenders ALTERNATING repeat by repeat,
    and the ratio of each contender's time to the translation hierarchy's of the same cycle and to block-Jacobi's, repeat by repeat.

Every comparison is within this run.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
from force_bench import train  # noqa: E402
from gradient_bench import hex_mesh, spread  # noqa: E402
from multilevel_bench import ratios, timed  # noqa: E402
from solver_bench import elastic_tangent  # noqa: E402

CYCLES = ("additive", "multiplicative")
SPACES = ("translations", "rigid_body")
CONTENDERS = ("block_jacobi",) + tuple(f"{space}/{cycle}" for cycle in CYCLES for space in SPACES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells-per-edge", type=int, default=108)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--coarsest-nodes", type=int, default=64)
    ap.add_argument("--methods", default="cg,bicgstab")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rigid_body_bench.json"))
    args = ap.parse_args()
    assert args.solve_repeats >= 3, "at least three alternated repeats"

    import torch
    from bicgstab_util import nonassociated_tangent

    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd.gradient import hex8_reference_gradients, integration_weights, inverse_jacobians
    from fenics_constitutive_amd.hostio import to_device

    assert torch.cuda.is_available(), "rigid_body_bench.py measures on the GPU"
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
    K = fc.TangentMatrix(force, format="bsr")
    K.set_constrained(mask)
    methods = {"cg": fc.ConjugateGradient, "bicgstab": fc.BiCGStab}
    methods = {name: methods[name] for name in args.methods.split(",")}
    values = {}
    if "cg" in methods:
        values["cg"] = K(to_device(elastic_tangent(210000.0, 0.3).reshape(-1), "cuda").repeat(n)).clone()
    if "bicgstab" in methods:
        values["bicgstab"] = K(to_device(nonassociated_tangent(n), "cuda")).clone()
    torch.cuda.synchronize()
    K._scratch.clear()  # (the element matrices of the assembly: not needed again)
    b = to_device(np.where(mask, 0.0, rng.normal(size=nd)), "cuda")
    x_out = torch.empty(nd, dtype=torch.float64, device="cuda")
    result = {"points": n, "nodes": n_nodes, "dofs": nd, "blocks": K.nnzb, "format": "bsr", "repeats": args.repeats, "solve_repeats": args.solve_repeats,
              "device": torch.cuda.get_device_name(0), "coarsest_nodes": args.coarsest_nodes, "rtol": 1e-8}

    # ---- (a) the hierarchies ---------------------------------------------------------------------------------------------------
    pcs = {}
    for space in SPACES:
        extra = {"coarse_space": space, "coordinates": nodes} if space == "rigid_body" else {}
        for cycle in CYCLES:
            t0 = time.perf_counter()
            pcs[f"{space}/{cycle}"] = pc = fc.MultilevelPreconditioner(K, cycle=cycle, coarsest_nodes=args.coarsest_nodes, **extra)
            host_s = round(time.perf_counter() - t0, 2)
        dofs = [3] + [pc.coarse_dofs] * (len(pc.levels) - 1)
        result[space] = {"hierarchy_host_s": host_s, "coarse_dofs": pc.coarse_dofs,
                         "levels": [{**lv, "dofs_per_node": d, "value_bytes": 8 * d * d * lv["blocks"]} for lv, d in zip(pc.levels, dofs)]}
        result[space]["coarse_value_bytes"] = sum(lv["value_bytes"] for lv in result[space]["levels"][1:])
        print(json.dumps({space: result[space]}), flush=True)
    result["resources"] = pcs["rigid_body/additive"].resources

    # ---- (b) the setup of a call -----------------------------------------------------------------------------------------------
    first = values[next(iter(values))]
    for space in SPACES:
        pc = pcs[f"{space}/additive"]
        result[space]["setup"] = spread(train(lambda: pc.setup(first), args.repeats, 5))
        print(json.dumps({space: {"setup": result[space]["setup"]}}), flush=True)

    # ---- (c) the whole solves, alternating ---------------------------------------------------------------------------------------
    for name, cls in methods.items():
        whole = {c: cls(K, preconditioner="block_jacobi" if c == "block_jacobi" else pcs[c], rtol=1e-8, maxiter=args.maxiter) for c in CONTENDERS}
        for c, s in whole.items():  # warm-up: every program loaded, every vector allocated
            s.maxiter, keep = 3, s.maxiter
            assert s(values[name], b, out=x_out).iterations == 3, c
            s.maxiter = keep
        solves, last = {c: [] for c in CONTENDERS}, {}
        for rep in range(args.solve_repeats):
            for c in CONTENDERS:
                ms, res = timed(lambda: whole[c](values[name], b, out=x_out))
                solves[c].append(ms)
                last[c] = res
                print(json.dumps({"method": name, "repeat": rep, "contender": c, "ms": round(ms, 1), "iterations": res.iterations, "status": res.status}), flush=True)
        rows = {}
        for c in CONTENDERS:
            res = last[c]
            rows[c] = {**spread(solves[c]), "iterations": res.iterations, "status": res.status, "residual_norm": res.residual_norm, "rhs_norm": res.rhs_norm,
                       "ms_per_iteration": round(float(np.median(solves[c])) / max(res.iterations, 1), 3),
                       "time_over_block_jacobi": ratios([t / j for t, j in zip(solves[c], solves["block_jacobi"])])}
        for cycle in CYCLES:
            rows[f"rigid_body/{cycle}"]["time_over_translations"] = ratios([r / t for r, t in zip(solves[f"rigid_body/{cycle}"], solves[f"translations/{cycle}"])])
            rows[f"rigid_body/{cycle}"]["iterations_over_translations"] = round(rows[f"rigid_body/{cycle}"]["iterations"] / max(rows[f"translations/{cycle}"]["iterations"], 1), 3)
        result[name] = rows
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
