"""The device solver (fenics_constitutive_amd.ConjugateGradient), measured on the GPU.

    python tools/solver_bench.py [--cells-per-edge 108] [--repeats 5] [--solve-repeats 3] [--out profiles/conjugate_gradient_bench.json]

One process, the mesh and operators of tools/matrix_bench.py (trilinear hexahedra, 2 x 2 x 2 points, per-point inverse Jacobians;
108 cells per edge: 10 077 696 points, 1 295 029 nodes), the tangent that of linear elasticity, the constraints those of the
tension test, both formats.  By device events, median (min - max) over ``--repeats``:

(a) the yardsticks of the same run: the gradient producer and the tangent action;
(b) one matrix-vector product ``solver.matvec`` against its byte model: 72 B of values and 4 B of column index per block (12 B
    in scalar CSR: an index per row of a block), 4 B of row pointer and three 24 B vector entries per node (p gathered, p and q
    of the fused dot);
(c) one whole iteration: a solve with ``rtol = 0`` stopped after ``--iterations`` iterations in one batch, divided by their number;
(d) a whole solve at ``rtol = 1e-8`` with its iteration count, block-Jacobi and plain (``--solve-repeats``);
(e) what the host route needs before it can start: the download of the values array.
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
from force_bench import train, with_model  # noqa: E402
from gradient_bench import hex_mesh, spread  # noqa: E402


def elastic_tangent(e_modulus: float, nu: float) -> np.ndarray:
    """the 6 x 6 Mandel tangent of isotropic linear elasticity"""
    lam, mu = e_modulus * nu / ((1 + nu) * (1 - 2 * nu)), e_modulus / (2 * (1 + nu))
    c = 2 * mu * np.eye(6)
    c[:3, :3] += lam
    return c


def timed_solve(cg, values, b, out, repeats):
    """(times in ms by device events around the whole call, the last result)"""
    import torch

    times, res = [], None
    for _ in range(repeats + 1):  # (the first call allocates the work vectors and loads the kernels)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = cg(values, b, out=out)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return times[1:], res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells-per-edge", type=int, default=108)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conjugate_gradient_bench.json"))
    args = ap.parse_args()

    import torch

    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd import solver
    from fenics_constitutive_amd.gradient import hex8_reference_gradients, integration_weights, inverse_jacobians
    from fenics_constitutive_amd.hostio import download, to_device

    assert torch.cuda.is_available(), "solver_bench.py measures on the GPU"
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
    # the constraints of the tension test: z at the bottom and the top face, x and y at the origin, y at the corner (1, 0, 0)
    mask = np.zeros(nd, dtype=bool)
    mask[3 * np.flatnonzero((nodes[:, 2] < 1e-12) | (nodes[:, 2] > 1 - 1e-12)) + 2] = True
    origin = int(np.flatnonzero((np.abs(nodes) < 1e-12).all(axis=1))[0])
    xcorner = int(np.flatnonzero((np.abs(nodes - [1.0, 0.0, 0.0]) < 1e-12).all(axis=1))[0])
    mask[[3 * origin, 3 * origin + 1, 3 * xcorner + 1]] = True
    tangent = to_device(elastic_tangent(210000.0, 0.3).reshape(-1), "cuda").repeat(n)
    du_dev = to_device(rng.normal(size=nd) / m, "cuda")
    grad = torch.empty(9 * n, dtype=torch.float64, device="cuda")
    f = torch.empty(nd, dtype=torch.float64, device="cuda")
    result = {"points": n, "nodes": n_nodes, "dofs": nd, "repeats": args.repeats, "launches_per_train": args.launches,
              "device": torch.cuda.get_device_name(0), "segments": -(-nd // solver.SEG), "slab_doubles": solver.SLAB}

    # ---- (a) the yardsticks ----------------------------------------------------------------------------------------------------
    node_bytes = 24 * cells.size + 4 * cells.size + 4 * n_nodes + 24 * n_nodes
    result["producer"] = with_model(train(lambda: op(du_dev, out=grad), args.repeats), 144 * n + 4 * cells.size + 24 * n_nodes, n)
    result["tangent_action"] = with_model(train(lambda: force.tangent_action(tangent, grad, out=f), args.repeats),
                                          (288 + 72 + 72 + 8) * n + 24 * cells.size + node_bytes, n)
    print(json.dumps({k: result[k] for k in ("producer", "tangent_action")}), flush=True)
    del grad, du_dev

    b = torch.where(to_device(mask, "cuda"), torch.zeros((), dtype=torch.float64, device="cuda"), to_device(rng.normal(size=nd), "cuda"))
    p = to_device(rng.normal(size=nd), "cuda")
    x_out = torch.empty(nd, dtype=torch.float64, device="cuda")
    for fmt in ("bsr", "csr"):
        K = fc.TangentMatrix(force, format=fmt)
        K.set_constrained(mask)
        values = K(tangent)
        torch.cuda.synchronize()
        K._scratch.clear()  # (TangentMatrix keeps its 256 MiB of element matrices per device and has no call that frees them: dropped here, before the solver's vectors are allocated, so that two formats do not hold two of them)
        row = {"blocks": K.nnzb}
        if fmt == "bsr":
            result["resources"] = fc.ConjugateGradient(K).resources
        # ---- (b) one product ---------------------------------------------------------------------------------------------------
        product_bytes = (76 if fmt == "bsr" else 72 + 4 * 3) * K.nnzb + 4 * n_nodes + 3 * 8 * nd
        row["matvec"] = with_model(train(lambda: solver.matvec(K, values, p, out=f), args.repeats, args.launches), product_bytes, n)
        row["matvec"]["model_bytes"] = product_bytes
        for name in ("tangent_action", "producer"):
            row["matvec"][f"times_the_{name}"] = round(row["matvec"]["median_ms"] / result[name]["median_ms"], 2)
        # ---- (c) one whole iteration ---------------------------------------------------------------------------------------------
        its = args.iterations
        times, res = timed_solve(fc.ConjugateGradient(K, rtol=0.0, maxiter=its, check_every=its), values, b, x_out, args.repeats)
        assert res.iterations == its and res.status == "maxiter", (res.iterations, res.status)
        row["iteration"] = {**spread([t / its for t in times]), "iterations_per_batch": its}
        print(json.dumps({fmt: row}), flush=True)
        # ---- (d) a whole solve ---------------------------------------------------------------------------------------------------
        for pc in ("block_jacobi", None):
            times, res = timed_solve(fc.ConjugateGradient(K, preconditioner=pc, rtol=1e-8, maxiter=args.maxiter), values, b, x_out, args.solve_repeats)
            row[f"solve_{pc or 'plain'}"] = {**spread(times), "iterations": res.iterations, "status": res.status, "residual_norm": res.residual_norm,
                                             "rhs_norm": res.rhs_norm, "ms_per_iteration": round(float(np.median(times)) / max(res.iterations, 1), 3)}
            print(json.dumps({fmt: {f"solve_{pc or 'plain'}": row[f"solve_{pc or 'plain'}"]}}), flush=True)
        # ---- (e) the values array coming down, for a solver on the host ----------------------------------------------------------
        if fmt == "csr":
            host_values = np.empty(K.nnz)
            times = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                download(host_values, values.reshape(-1))
                times.append((time.perf_counter() - t0) * 1e3)
            result["download_values"] = {**spread(times), "bytes": 8 * K.nnz}
            del host_values
        result[fmt] = row
        del values, K
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
