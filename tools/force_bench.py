"""The force operator (fenics_constitutive_amd.InternalForce) and the matrix-free Newton iteration around it, measured on the GPU.

    python tools/force_bench.py [--cells-per-edge 108] [--repeats 5] [--out profiles/internal_force_bench.json]

One process, the mesh of tools/gradient_bench.py (trilinear hexahedra, 2 x 2 x 2 points, per-point inverse Jacobians; 108 cells per
edge: 10 077 696 points):

(a) the kernels alone, by device events around trains of launches: the gradient producer (the yardstick of the same run), the
    internal force (element + node kernel, and each of the two apart) and the tangent action, each against its byte model --
      element kernel  stress 48 + jinv 72 + weight 8 B/pt in (tangent action: tangent 288 + gradient 72 + jinv 72 + weight 8), fe out
      node kernel     fe in, 4 B per adjacency entry and per node, 24 B per node out
    (fe is 24 B per (cell, node): 24 B/pt for the hexahedron);
(b) one Newton iteration's residual, for LinearElasticityModel and VonMises3D (22 % plastic points): upload the nodal increment +
    producer + ResidentState.evaluate + force + download f, against evaluate_into(device gradient, stress=page-locked ndarray) and
    fe_mini.Cube.internal_force's arithmetic on the host (the regular box's B matrices, an einsum and np.add.at).
Every figure is taken ``--repeats`` times (each the best of three calls; the host assembly one call); the spread is the margin.
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
from gradient_bench import best_of, hex_mesh, make_law, scale_for_plastic_fraction, spread  # noqa: E402


def train(fn, repeats, launches=20):
    """ms per call of ``fn`` (asynchronous device work) from device events around trains of ``launches`` calls"""
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / launches)
    return times


def with_model(times, model_bytes, n):
    return {**spread(times), "model_bytes_per_point": round(model_bytes / n, 2),
            "achieved_GB_s": round(model_bytes / (float(np.median(times)) * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells-per-edge", type=int, default=108)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "internal_force_bench.json"))
    args = ap.parse_args()

    import fe_mini
    import torch

    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd import _capi
    from fenics_constitutive_amd.gradient import hex8_reference_gradients, integration_weights, inverse_jacobians
    from fenics_constitutive_amd.hostio import download, to_device, to_host
    from fenics_constitutive_amd.resident import ResidentState

    assert torch.cuda.is_available(), "force_bench.py measures on the GPU"
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
    du = rng.normal(size=nd) / m
    result = {"points": n, "cells": n_cells, "nodes": n_nodes, "repeats": args.repeats, "resources": force.resources,
              "producer_resources": op.resources, "device": torch.cuda.get_device_name(0)}

    # ---- (a) the kernels alone -------------------------------------------------------------------------------------------------
    du_dev = to_device(du, "cuda")
    grad = torch.empty(9 * n, dtype=torch.float64, device="cuda")
    stress = to_device(rng.normal(scale=100.0, size=6 * n), "cuda")
    tangent = torch.empty(36 * n, dtype=torch.float64, device="cuda").normal_(std=1e4)
    f = torch.empty(nd, dtype=torch.float64, device="cuda")
    node_bytes = 24 * cells.size + 4 * cells.size + 4 * n_nodes + 24 * n_nodes
    models = {"producer": 144 * n + 4 * cells.size + 24 * n_nodes,
              "internal_force": (48 + 72 + 8) * n + 24 * cells.size + node_bytes,
              "tangent_action": (288 + 72 + 72 + 8) * n + 24 * cells.size + node_bytes}
    calls = {"producer": lambda: op(du_dev, out=grad), "internal_force": lambda: force(stress, out=f),
             "tangent_action": lambda: force.tangent_action(tangent, grad, out=f)}
    for name in ("producer", "internal_force", "tangent_action"):
        result[name] = with_model(train(calls[name], args.repeats), models[name], n)
        print(json.dumps({name: result[name]}), flush=True)
    for name in ("internal_force", "tangent_action"):
        result[name]["times_the_producer"] = round(result[name]["median_ms"] / result["producer"]["median_ms"], 2)
    # the two kernels of the internal force apart: the same call with the other kernel's launch left out
    from fenics_constitutive_amd import force as force_module
    from fenics_constitutive_amd import jit

    real_launch = jit.launch
    for kernel, tag, model in ((force_module.ELEMENT_KERNEL, "element_kernel", (48 + 72 + 8) * n + 24 * cells.size), (force_module.NODE_KERNEL, "node_kernel", node_bytes)):
        jit.launch = lambda code, dev, blocks, a, what, kernel=None, only=kernel: real_launch(code, dev, blocks, a, what, kernel=kernel) if (kernel or code.kernel) == only else None
        try:
            result[tag] = with_model(train(calls["internal_force"], args.repeats), model, n)
        finally:
            jit.launch = real_launch
        print(json.dumps({tag: result[tag]}), flush=True)
    del tangent

    # ---- (b) the residual of one Newton iteration -------------------------------------------------------------------------------
    ctx = _capi.get_context(_capi.default_device())
    unit = fe_mini.Cube(1, 1, 1)
    b_matrices, weight = unit.B * m, unit.w / m**3  # the B matrices of fe_mini.Cube(m, m, m), without building its 24 x 24 index arrays
    cell_dofs = (3 * cells[:, :, None] + np.arange(3)[None, None, :]).reshape(n_cells, 24)

    def host_internal_force(s):  # fe_mini.Cube.internal_force
        fe = weight * np.einsum("qmd,eqm->ed", b_matrices, s.reshape(n_cells, 8, 6))
        out = np.zeros(nd)
        np.add.at(out, cell_dofs.ravel(), fe.ravel())
        return out

    g_unit = to_host(op(du_dev))
    scales = {"LinearElasticityModel": 1e-3, "VonMises3D": scale_for_plastic_fraction(g_unit, 0.22)}
    del g_unit
    result["newton_residual"] = {}
    f_host = np.zeros(nd)
    so = np.zeros(6 * n)
    for a in (f_host, so):
        ctx.register_host_buffer(a)
    for name, scale in scales.items():
        du_s = scale * du
        law = make_law(name)
        st = ResidentState(law, n, placement="torch")

        def host_call():
            st.evaluate_into(0.0, 1.0, op(du_s, out=grad), so)

        host_call()
        t_eval = [best_of(host_call) for _ in range(args.repeats)]
        plastic = int(law.last_stats.n_plastic) if name == "VonMises3D" else 0
        t_asm = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            f_ref = host_internal_force(so)
            t_asm.append((time.perf_counter() - t0) * 1e3)
        rs = ResidentState(make_law(name), n, placement="torch")

        def device_call():
            rs.evaluate(0.0, 1.0, op(du_s, out=grad))
            download(f_host, force(rs.stress, out=f))  # (synchronous: the clock stops after the vector has arrived)

        device_call()
        t_dev = [best_of(device_call) for _ in range(args.repeats)]
        scale_f = float(np.abs(f_ref).max())
        row = {"plastic_fraction": round(plastic / n, 4), "evaluate_into_stress_ndarray": spread(t_eval), "host_internal_force": spread(t_asm),
               "matrix_free": spread(t_dev), "host_total_median_ms": round(float(np.median(t_eval) + np.median(t_asm)), 3),
               "bytes_over_the_link_matrix_free": 2 * 8 * nd, "bytes_over_the_link_host": 8 * nd + 48 * n,
               # the host stand-in assembles with the regular box's B matrices, the device with the moved nodes' own: not the same numbers
               "largest_force_entry": scale_f}
        row["speedup"] = round(row["host_total_median_ms"] / row["matrix_free"]["median_ms"], 2)
        row["speedup_over_evaluate_into_alone"] = round(row["evaluate_into_stress_ndarray"]["median_ms"] / row["matrix_free"]["median_ms"], 2)
        result["newton_residual"][name] = row
        print(json.dumps({name: row}), flush=True)
        del st, rs
    for a in (f_host, so):
        ctx.unregister_host_buffer(a)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
