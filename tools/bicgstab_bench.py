"""The device BiCGStab (fenics_constitutive_amd.BiCGStab) against the conjugate gradients, measured on the GPU.

    python tools/bicgstab_bench.py [--cells-per-edge 108] [--repeats 5] [--solve-repeats 3] [--out profiles/bicgstab_bench.json]

One process, the cube of tools/multilevel_bench.py (trilinear hexahedra, 2 x 2 x 2 points, per-point inverse Jacobians; 108 cells
per edge: 1 295 029 nodes, 3.9 M dofs), the constraints those of the tension test, block CSR.  Two matrices over the one pattern:
the ELASTIC one (symmetric) and the UNSYMMETRIC one of tests/bicgstab_util.py (the non-associated tangent, b = 0.6, b_flow = 0, at a
seeded 30 % of the points).  Every solver is built once and warmed up outside the timed regions; by device events, ALTERNATING
repeat by repeat, median (min - max):

(a) the product kernel in both modes ("v": one fused dot; "t": two) next to the conjugate gradients' product (one fused dot), the
    elastic values;
(b) one whole iteration, the elastic values: a solve with ``rtol = 0`` stopped after ``--iterations`` iterations in one batch, divided
    by their number -- BiCGStab and the conjugate gradients, with block-Jacobi and with the additive cycle;
(c) the whole BiCGStab solve of the unsymmetric system at ``rtol = 1e-8`` with its iteration count and true residual, next to the
    status the conjugate gradients end with on it (capped at ``--cg-maxiter`` iterations).
"""

from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "examples"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

import numpy as np  # noqa: E402
from gradient_bench import hex_mesh, spread  # noqa: E402
from multilevel_bench import ratios, timed  # noqa: E402
from solver_bench import elastic_tangent  # noqa: E402

PRECONDITIONERS = ("block_jacobi", "additive")


def trains(fns: dict, repeats: int, launches: int = 5) -> dict:
    """ms per call of every ``fns[name]`` (asynchronous device work): trains of ``launches`` calls between device events, the
    functions alternating repeat by repeat"""
    import torch

    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            ms, _ = timed(lambda: [fn() for _ in range(launches)])
            times[name].append(ms / launches)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells-per-edge", type=int, default=108)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--cg-maxiter", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bicgstab_bench.json"))
    args = ap.parse_args()
    assert args.solve_repeats >= 3, "at least three alternated repeats"

    import torch
    from bicgstab_util import nonassociated_tangent

    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd import bicgstab, jit, solver
    from fenics_constitutive_amd.gradient import hex8_reference_gradients, integration_weights, inverse_jacobians
    from fenics_constitutive_amd.hostio import to_device

    assert torch.cuda.is_available(), "bicgstab_bench.py measures on the GPU"
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
    elastic = K(to_device(elastic_tangent(210000.0, 0.3).reshape(-1), "cuda").repeat(n)).clone()
    unsymmetric = K(to_device(nonassociated_tangent(n), "cuda")).clone()
    torch.cuda.synchronize()
    K._scratch.clear()  # (the element matrices of the assembly: not needed again)
    a = K.to_scipy(unsymmetric)
    d = a - a.T
    asym = float(np.sqrt((d.data**2).sum() / (a.data**2).sum()))  # |K - K^T|_F / |K|_F
    del d
    b_host = np.where(mask, 0.0, rng.normal(size=nd))
    b = to_device(b_host, "cuda")
    x_out = torch.empty(nd, dtype=torch.float64, device="cuda")
    pc = fc.MultilevelPreconditioner(K, cycle="additive")
    result = {"points": n, "nodes": n_nodes, "dofs": nd, "blocks": K.nnzb, "format": "bsr", "repeats": args.repeats, "solve_repeats": args.solve_repeats,
              "device": torch.cuda.get_device_name(0), "rtol": 1e-8, "asymmetry": round(asym, 4), "levels": pc.levels}

    def build(cls, kind, **kw):
        return cls(K, preconditioner="block_jacobi" if kind == "block_jacobi" else pc, **kw)

    # ---- warm-up: every program loaded, every vector allocated -------------------------------------------------------------------
    its = args.iterations
    classes = {"bicgstab": fc.BiCGStab, "cg": fc.ConjugateGradient}
    batch = {(name, kind): build(cls, kind, rtol=0.0, maxiter=its, check_every=its) for name, cls in classes.items() for kind in PRECONDITIONERS}
    whole = {kind: build(fc.BiCGStab, kind, rtol=1e-8, maxiter=args.maxiter) for kind in PRECONDITIONERS}
    cg_whole = build(fc.ConjugateGradient, "block_jacobi", rtol=1e-8, maxiter=args.cg_maxiter, check_every=64)
    for key, s in batch.items():
        res = s(elastic, b, out=x_out)
        assert res.status == "maxiter" and res.iterations == its, (key, res.status)
    for kind, s in whole.items():
        s.maxiter, keep = 3, s.maxiter
        assert s(unsymmetric, b, out=x_out).iterations == 3
        s.maxiter = keep
    result["resources"] = batch[("bicgstab", "block_jacobi")].resources
    result["resources_cg_product"] = {k: v for k, v in batch[("cg", "block_jacobi")].resources.items() if not isinstance(v, dict)}

    # ---- (a) the products ---------------------------------------------------------------------------------------------------------
    s = batch[("bicgstab", "block_jacobi")]
    control, r, rhat, p, v, t, y, z, inv = s._workspace(0)
    control.upload(0.0, 0.0, 1)  # status "running": the product kernel honours it
    vec, other = to_device(rng.normal(size=nd), "cuda"), to_device(rng.normal(size=nd), "cuda")

    def product(dots):
        pa = bicgstab.Params()
        pa.cg = s._op.args(0, elastic, control)
        pa.cg.va, pa.cg.q, pa.cg.vb, pa.cg.mode = vec.data_ptr(), t.data_ptr(), other.data_ptr(), dots
        return lambda: jit.launch(s._code, 0, s._op.blocks(0), pa, "bicgstab_bench product launch", kernel=bicgstab.PRODUCT_KERNEL)

    times = trains({"cg_product": lambda: solver.matvec(K, elastic, vec, out=x_out), "product_v": product(0), "product_t": product(1)}, args.repeats)
    control.download(0)
    assert int(control.ints[solver._STATUS]) == 0, "the timed products did not run"
    result["products"] = {name: spread(ms) for name, ms in times.items()}
    for name in ("product_v", "product_t"):
        result["products"][name]["times_the_cg_product"] = ratios([x / c for x, c in zip(times[name], times["cg_product"])])
    print(json.dumps({"products": result["products"]}), flush=True)

    # ---- (b) one whole iteration, the elastic values ------------------------------------------------------------------------------
    per_iteration = {key: [] for key in batch}
    for _ in range(args.repeats):
        for key, solve in batch.items():
            ms, res = timed(lambda: solve(elastic, b, out=x_out))
            assert res.iterations == its and res.status == "maxiter", (key, res.iterations, res.status)
            per_iteration[key].append(ms / its)
    result["iteration"] = {}
    for kind in PRECONDITIONERS:
        row = {name: spread(per_iteration[(name, kind)]) for name in classes}
        row["bicgstab_over_cg"] = ratios([x / c for x, c in zip(per_iteration[("bicgstab", kind)], per_iteration[("cg", kind)])])
        row["iterations_per_batch"] = its
        result["iteration"][kind] = row
    print(json.dumps({"iteration": result["iteration"]}), flush=True)

    # ---- (c) the whole solve of the unsymmetric system -----------------------------------------------------------------------------
    solves = {kind: [] for kind in PRECONDITIONERS}
    last = {}
    for rep in range(args.solve_repeats):
        for kind in PRECONDITIONERS:
            ms, res = timed(lambda: whole[kind](unsymmetric, b, out=x_out))
            solves[kind].append(ms)
            last[kind] = (res, float(np.linalg.norm(b_host - a @ x_out.cpu().numpy()) / np.linalg.norm(b_host)))
            print(json.dumps({"repeat": rep, "preconditioner": kind, "ms": round(ms, 1), "iterations": res.iterations, "status": res.status}), flush=True)
    result["solve"] = {}
    for kind in PRECONDITIONERS:
        res, true = last[kind]
        result["solve"][kind] = {**spread(solves[kind]), "iterations": res.iterations, "status": res.status, "residual_norm": res.residual_norm, "rhs_norm": res.rhs_norm,
                                 "true_residual_over_rhs": true, "ms_per_iteration": round(float(np.median(solves[kind])) / max(res.iterations, 1), 3)}
    ms, res = timed(lambda: cg_whole(unsymmetric, b, out=x_out))
    result["solve"]["cg_block_jacobi"] = {"status": res.status, "iterations": res.iterations, "maxiter": args.cg_maxiter, "ms": round(ms, 1), "residual_norm": res.residual_norm,
                                          "rhs_norm": res.rhs_norm, "true_residual_over_rhs": float(np.linalg.norm(b_host - a @ x_out.cpu().numpy()) / np.linalg.norm(b_host))}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
