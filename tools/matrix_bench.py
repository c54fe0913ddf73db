"""The assembled tangent stiffness (fenics_constitutive_amd.TangentMatrix), measured on the GPU.

    python tools/matrix_bench.py [--cells-per-edge 108] [--host-cells-per-edge 48] [--repeats 5] [--out profiles/tangent_matrix_bench.json]

One process, the mesh of tools/force_bench.py (trilinear hexahedra, 2 x 2 x 2 points, per-point inverse Jacobians; 108 cells per
edge: 10 077 696 points).  By device events around trains of launches, median (min - max) over ``--repeats``:

(a) the yardsticks of the same run: the gradient producer and the tangent action;
(b) the whole call ``K(tangent, out=values)`` in both formats with the default ``scratch_bytes`` (chunked) and with a scratch that
    holds every element matrix (one chunk), and the two kernels apart (the same call with the other kernel's launch left out),
    each against its byte model --
      element kernel  tangent 288 + jinv 72 + weight 8 B/pt in, 576 B/pt of element matrices out
      gather kernel   576 B/pt in, 4 B per contribution (8 per point) and 16 B per block of tables in, 72 B per block out;
(c) on the host, what the device path replaces: the download of the 288 B/pt of tangent and ``fe_mini.Cube.stiffness``'s
    arithmetic (an einsum and a COO -> CSR conversion), at ``--host-cells-per-edge`` (the COO triplets of the full size do not fit
    a host's memory comfortably), timed, not compared on values.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells-per-edge", type=int, default=108)
    ap.add_argument("--host-cells-per-edge", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tangent_matrix_bench.json"))
    args = ap.parse_args()

    import fe_mini
    import torch

    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd import jit
    from fenics_constitutive_amd import matrix as matrix_module
    from fenics_constitutive_amd.gradient import hex8_reference_gradients, integration_weights, inverse_jacobians
    from fenics_constitutive_amd.hostio import download, to_device

    assert torch.cuda.is_available(), "matrix_bench.py measures on the GPU"
    m = args.cells_per_edge
    rng = np.random.default_rng(1)
    nodes, cells = hex_mesh(m, rng)
    ref = hex8_reference_gradients()
    x = nodes[cells]
    op = fc.DisplacementGradient(cells, ref, inverse_jacobians(x, ref), nodes.shape[0])
    force = fc.InternalForce(op, integration_weights(x, ref, np.ones(8)))
    del x
    n, n_nodes, n_cells = op.n_points, op.n_nodes, op.n_cells
    nd = 3 * n_nodes
    t0 = time.perf_counter()
    K = fc.TangentMatrix(force, format="bsr")
    symbolic_s = time.perf_counter() - t0
    whole = 8 * 576 * n_cells
    result = {"points": n, "cells": n_cells, "nodes": n_nodes, "blocks": K.nnzb, "contributions": int(K.contributions.size), "repeats": args.repeats,
              "launches_per_train": args.launches, "symbolic_phase_host_s": round(symbolic_s, 2), "resources": K.resources,
              "default_scratch_bytes": matrix_module.SCRATCH_BYTES, "chunks_at_default": len(K.chunks()), "unchunked_scratch_bytes": whole,
              "device": torch.cuda.get_device_name(0)}
    print(json.dumps({k: result[k] for k in ("points", "blocks", "contributions", "symbolic_phase_host_s", "chunks_at_default")}), flush=True)

    # ---- (a) the yardsticks ----------------------------------------------------------------------------------------------------
    du_dev = to_device(rng.normal(size=nd) / m, "cuda")
    grad = torch.empty(9 * n, dtype=torch.float64, device="cuda")
    tangent = torch.empty(36 * n, dtype=torch.float64, device="cuda").normal_(std=1e4)
    f = torch.empty(nd, dtype=torch.float64, device="cuda")
    node_bytes = 24 * cells.size + 4 * cells.size + 4 * n_nodes + 24 * n_nodes
    result["producer"] = with_model(train(lambda: op(du_dev, out=grad), args.repeats), 144 * n + 4 * cells.size + 24 * n_nodes, n)
    result["tangent_action"] = with_model(train(lambda: force.tangent_action(tangent, grad, out=f), args.repeats),
                                          (288 + 72 + 72 + 8) * n + 24 * cells.size + node_bytes, n)
    print(json.dumps({k: result[k] for k in ("producer", "tangent_action")}), flush=True)
    del grad, f, du_dev

    # ---- (b) the assembly ------------------------------------------------------------------------------------------------------
    element_bytes = (288 + 72 + 8) * n + 576 * n
    gather_bytes = 576 * n + 4 * K.contributions.size + (4 + 8 + 4) * K.nnzb + 72 * K.nnzb
    real_launch = jit.launch
    values = torch.empty(K.nnz, dtype=torch.float64, device="cuda")
    for fmt in matrix_module.FORMATS:
        for tag, scratch in (("default_scratch", None), ("one_chunk", whole)):
            k = K if (fmt == "bsr" and scratch is None) else fc.TangentMatrix(force, format=fmt, scratch_bytes=scratch)
            row = {"chunks": len(k.chunks())}
            row["call"] = with_model(train(lambda: k(tangent, out=values), args.repeats, args.launches), element_bytes + gather_bytes, n)
            for kernel, name, model in ((matrix_module.ELEMENT_KERNEL, "element_kernel", element_bytes), (matrix_module.GATHER_KERNEL, "gather_kernel", gather_bytes)):
                jit.launch = lambda code, dev, blocks, a, what, kernel=None, only=kernel: real_launch(code, dev, blocks, a, what, kernel=kernel) if (kernel or code.kernel) == only else None
                try:
                    row[name] = with_model(train(lambda: k(tangent, out=values), args.repeats, args.launches), model, n)
                finally:
                    jit.launch = real_launch
            for name in ("call", "element_kernel", "gather_kernel"):
                row[name]["times_the_tangent_action"] = round(row[name]["median_ms"] / result["tangent_action"]["median_ms"], 2)
            result[f"{fmt}_{tag}"] = row
            print(json.dumps({f"{fmt}_{tag}": row}), flush=True)
            if k is not K:
                k._scratch.clear()
                del k
    # the values array coming down, for a solver on the host
    host_values = np.empty(K.nnz)
    times = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        download(host_values, values)
        times.append((time.perf_counter() - t0) * 1e3)
    result["download_values"] = {**spread(times), "bytes": 8 * K.nnz}
    del host_values, values

    # ---- (c) what the device path replaces: the tangent down the link and assembled on the host ---------------------------------
    mh = args.host_cells_per_edge
    mesh = fe_mini.Cube(mh, mh, mh)
    nh = mesh.n_points
    tangent_host = np.empty(36 * nh)
    times_down, times_asm = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        download(tangent_host, tangent[: 36 * nh])
        times_down.append((time.perf_counter() - t0) * 1e3)
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        mesh.stiffness(tangent_host)
        times_asm.append((time.perf_counter() - t0) * 1e3)
    scale = n / nh
    result["host"] = {"cells_per_edge": mh, "points": nh, "download_tangent": spread(times_down), "cube_stiffness": spread(times_asm),
                      "scaled_to_the_device_size_ms": round(float(np.median(times_down) + np.median(times_asm)) * scale, 1)}
    print(json.dumps({"host": result["host"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
