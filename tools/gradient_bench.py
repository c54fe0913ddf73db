"""The gradient producer (fenics_constitutive_amd.DisplacementGradient) and the host path behind it, measured on the GPU.

    python tools/gradient_bench.py [--cells-per-edge 108] [--repeats 5] [--parent-lib tools/_ab/libfcamd_<commit>.so] [--out FILE.json]

One process, the same buffers for every variant (trilinear hexahedra, 2 x 2 x 2 points, per-point inverse Jacobians; 108 cells per
edge: 10 077 696 points):

(a) the producer alone: ms per launch (device events around a train of launches) and the bytes/s it achieves against its model --
    72 B/pt of inverse Jacobians in, 72 B/pt of gradient out, and the gather amortised over the points (the dofmap once, every
    node's displacement once: the repeated reads of a node by its cells are cache hits by assumption -- the model says so);
(b) ResidentState.evaluate_into at that size for LinearElasticityModel and VonMises3D (22 % plastic points), page-locked arrays,
    default options: the ndarray gradient against "upload the nodal increment + producer + device gradient", the same gradient
    VALUES in both.  Every figure is taken ``--repeats`` times (each the best of three calls); the spread of the repeats is the
    margin of every comparison.

``--parent-lib``: the ndarray call also runs against that library (tools/build_at.sh <parent commit>) in fresh child processes
before and after this process's own measurements, and in one more such child on this tree's library -- child against child is the
comparison that shows whether a call without the flag slowed down (this process has other allocations alive).
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
LE_P = {"E": 42.0, "nu": 0.3}


def hex_mesh(m: int, rng):
    """(nodes [N][3], cells [C][8] int32) of m^3 trilinear hexahedra on the unit cube, the interior nodes moved a little (so that
    the inverse Jacobians differ from point to point)"""
    xs = np.linspace(0.0, 1.0, m + 1)
    nodes = np.stack(np.meshgrid(xs, xs, xs, indexing="ij"), axis=-1).reshape(-1, 3)
    nodes = nodes + rng.uniform(-0.1, 0.1, size=nodes.shape) / m * ((nodes > 0) & (nodes < 1))
    nid = np.arange((m + 1) ** 3).reshape(m + 1, m + 1, m + 1)
    corner = [nid[a: a + m, b: b + m, c: c + m] for a, b, c in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))]  # gradient.HEX8_SIGNS
    return nodes, np.ascontiguousarray(np.stack(corner, axis=-1).reshape(-1, 8), dtype=np.int32)


def spread(xs):
    return {"ms": [round(x, 3) for x in xs], "median_ms": round(float(np.median(xs)), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def best_of(fn, calls=3):
    b = None
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()  # (evaluate_into is synchronous: the clock stops after the device has finished)
        dt = (time.perf_counter() - t0) * 1e3
        b = dt if b is None else min(b, dt)
    return b


def make_law(name):
    import fenics_constitutive_amd as fc

    return fc.VonMises3D(VM_P) if name == "VonMises3D" else fc.LinearElasticityModel(LE_P, fc.StressStrainConstraint.FULL)


def scale_for_plastic_fraction(g, fraction):
    """factor on the gradient at which ``fraction`` of the points leave the elastic range of VM_P from a stress-free state"""
    e = g.reshape(-1, 3, 3)
    e = 0.5 * (e + e.transpose(0, 2, 1))
    e = e - np.trace(e, axis1=1, axis2=2)[:, None, None] / 3.0 * np.eye(3)[None]
    seq = np.sqrt(1.5) * 2.0 * VM_P["p_mu"] * np.sqrt((e * e).sum(axis=(1, 2)))
    return VM_P["p_y0"] / float(np.quantile(seq, 1.0 - fraction))


def measure_ndarray(name, n, g, so, to, repeats):
    """evaluate_into with the (page-locked) ndarray gradient: what the parent commit's call does, on this process's library"""
    from fenics_constitutive_amd.resident import ResidentState

    law = make_law(name)
    st = ResidentState(law, n, placement="torch")
    st.evaluate_into(0.0, 1.0, g, so, to)  # warm: code objects, the tangent's first full pass
    times = [best_of(lambda: st.evaluate_into(0.0, 1.0, g, so, to)) for _ in range(repeats)]
    return times, int(law.last_stats.n_plastic)


def worker(args):
    """child process (FCAMD_LIBRARY = the parent commit's library): the ndarray call only, on gradients read from --worker"""
    from fenics_constitutive_amd import _capi

    data = np.load(args.worker)
    ctx = _capi.get_context(_capi.default_device())
    out = {}
    for name in ("LinearElasticityModel", "VonMises3D"):
        g = np.ascontiguousarray(data[name])
        n = g.size // 9
        so, to = np.zeros(6 * n), np.zeros(36 * n)
        for x in (g, so, to):
            ctx.register_host_buffer(x)
        times, plastic = measure_ndarray(name, n, g, so, to, args.repeats)
        out[name] = {**spread(times), "plastic": plastic}
        for x in (g, so, to):
            ctx.unregister_host_buffer(x)
    print("WORKER " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells-per-edge", type=int, default=108)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    import torch

    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd import _capi
    from fenics_constitutive_amd.gradient import hex8_reference_gradients, inverse_jacobians
    from fenics_constitutive_amd.hostio import to_device, to_host
    from fenics_constitutive_amd.resident import ResidentState

    assert torch.cuda.is_available(), "gradient_bench.py measures on the GPU"
    rng = np.random.default_rng(1)
    nodes, cells = hex_mesh(args.cells_per_edge, rng)
    ref = hex8_reference_gradients()
    jinv = inverse_jacobians(nodes[cells], ref)
    op = fc.DisplacementGradient(cells, ref, jinv, nodes.shape[0])
    n, n_nodes, n_cells = op.n_points, op.n_nodes, op.n_cells
    du = rng.normal(size=3 * n_nodes) / args.cells_per_edge  # gradients of order one before scaling
    ctx = _capi.get_context(_capi.default_device())
    result = {"points": n, "cells": n_cells, "nodes": n_nodes, "repeats": args.repeats, "resources": op.resources,
              "device": torch.cuda.get_device_name(0)}

    # ---- (a) the producer alone ---------------------------------------------------------------------------------------------
    du_dev = to_device(du, "cuda")
    out = torch.empty(9 * n, dtype=torch.float64, device="cuda")
    for _ in range(3):
        op(du_dev, out=out)
    torch.cuda.synchronize()
    launches = 20
    times = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            op(du_dev, out=out)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / launches)
    model_bytes = 144 * n + 4 * cells.size + 24 * n_nodes
    result["producer"] = {**spread(times), "model_bytes": model_bytes, "model_bytes_per_point": round(model_bytes / n, 2),
                          "achieved_GB_s": round(model_bytes / (float(np.median(times)) * 1e-3) / 1e9, 1)}
    print(json.dumps({"producer": result["producer"]}), flush=True)

    # ---- the gradients of (b): the producer's own output, scaled ------------------------------------------------------------
    g_unit = to_host(op(du_dev))
    scales = {"LinearElasticityModel": 1e-3, "VonMises3D": scale_for_plastic_fraction(g_unit, 0.22)}
    del g_unit
    grads = {k: to_host(op(s * du)) for k, s in scales.items()}  # the very values the device-gradient calls will read
    if args.parent_lib:
        import tempfile

        shared = os.path.join(tempfile.mkdtemp(prefix="gradient_bench_"), "inputs.npz")
        np.savez(shared, **grads)

    from fenics_constitutive_amd import _build

    def parent_run(tag, lib=None):
        env = dict(os.environ, FCAMD_LIBRARY=os.path.abspath(lib or args.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", shared, "--repeats", str(args.repeats)], env=env,
                           capture_output=True, text=True, timeout=900)
        line = [x for x in r.stdout.splitlines() if x.startswith("WORKER ")]
        if r.returncode != 0 or not line:
            raise RuntimeError(f"parent-library worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        result[tag] = json.loads(line[0][len("WORKER "):])
        print(json.dumps({tag: result[tag]}), flush=True)

    if args.parent_lib:
        parent_run("parent_library_before")
        parent_run("this_library_child", _build.LIB)  # the same child on this tree's library: like against like

    # ---- (b) evaluate_into: ndarray gradient against increment upload + producer + device gradient ---------------------------
    result["evaluate_into"] = {}
    for name, scale in list(scales.items()):
        g = grads.pop(name)
        du_s = scale * du
        so, to = np.zeros(6 * n), np.zeros(36 * n)
        for x in (g, so, to):
            ctx.register_host_buffer(x)
        row = {}
        t_nd, plastic = measure_ndarray(name, n, g, so, to, args.repeats)
        s_nd, t_ref = so.copy(), to.copy()
        mode_nd = ctx.last_host_mode()
        law = make_law(name)
        st = ResidentState(law, n, placement="torch")

        def device_call():
            st.evaluate_into(0.0, 1.0, op(du_s, out=out), so, to)  # (op uploads the ndarray increment synchronously)

        so[:], to[:] = 0.0, 0.0
        device_call()
        t_dev = [best_of(device_call) for _ in range(args.repeats)]
        row = {"plastic_fraction": round(plastic / n, 4), "ndarray": spread(t_nd), "device_gradient": spread(t_dev),
               "ndarray_Mpts_s": round(n / np.median(t_nd) / 1e3, 1), "device_gradient_Mpts_s": round(n / np.median(t_dev) / 1e3, 1),
               "mode_ndarray": mode_nd, "mode_device_gradient": ctx.last_host_mode(),
               "same_bits": bool(np.array_equal(so.view(np.uint64), s_nd.view(np.uint64)) and np.array_equal(to.view(np.uint64), t_ref.view(np.uint64)))}
        result["evaluate_into"][name] = row
        print(json.dumps({name: row}), flush=True)
        del st
        for x in (g, so, to):
            ctx.unregister_host_buffer(x)

    if args.parent_lib:
        parent_run("parent_library_after")
        os.remove(shared)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
