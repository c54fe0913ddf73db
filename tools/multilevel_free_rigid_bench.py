"""The rigid-body coarse space on the matrix-free operator against the three combinations the package had, measured on the GPU.

    python tools/multilevel_free_rigid_bench.py [--mesh hex8 tet_p2] [--cells-per-edge 108] [--repeats 5] [--solve-repeats 3]
                                                [--out profiles/multilevel_free_rigid_bench.json]

One process PER MESH (with several meshes this process starts a fresh child for each and touches no GPU itself); the two meshes and
the settings of tools/multilevel_free_bench.py (the unit cube with 109^3 nodes, 3.9 M dofs at the default size: trilinear hexahedra
with 2 x 2 x 2 points, 1.0e7 points, and 10-node tetrahedra with 4 points, 3.8 M points; the constraints of the tension test, block
CSR, ``rtol = 1e-8``, ``coarsest_nodes = 64``, the default scratch).  Four contenders, everything built once and warmed up outside the
timed regions, device events, the contenders ALTERNATING repeat by repeat, median (min - max), every comparison within the run:

    operator + rigid body      ConjugateGradient(A, preconditioner=MultilevelPreconditioner(A, coarse_space="rigid_body", coordinates=X))   (new)
    operator + translations    ConjugateGradient(A, preconditioner=MultilevelPreconditioner(A))
    matrix + rigid body        ConjugateGradient(K, preconditioner=MultilevelPreconditioner(K, coarse_space="rigid_body", coordinates=X)), its assembly timed apart
    operator + block-Jacobi    ConjugateGradient(A)

(a) conjugate gradients on the elastic tangent, both cycles: the whole solve with its iterations, its time per iteration, and one
    iteration of a batch of ``--iterations`` with the call's setup in it;
(b) the additive cycle under ``MatrixFreeBiCGStab`` on the UNSYMMETRIC tangent of tests/bicgstab_util.py, rigid body against
    translations on the operator and against ``BiCGStab(K)`` with the rigid-body modes: status, iterations, residual, time;
(c) ``pc.setup(tangent)`` of the new route and of the translations, and alone, over all chunks, the new gather
    (fcamd_mfr_galerkin_kernel) against the translation gather (fcamd_mf_galerkin_kernel) and the element matrices they share; the
    matrix route's assembly and ``pc.setup(values)``;
(d) ``torch.cuda.memory_allocated`` around the first use of every contender.
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "examples"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

import numpy as np  # noqa: E402

CYCLES = ("additive", "multiplicative")
SPACES = ("operator rigid_body", "operator translations", "matrix rigid_body")
GATHERS = {"operator rigid_body": "MultilevelPreconditioner first rigid-body Galerkin launch", "operator translations": "MultilevelPreconditioner first Galerkin launch"}
ELEMENTS = "MultilevelPreconditioner element launch"


def measure(mesh: str, args, rng) -> dict:
    import torch
    from bicgstab_bench import timed, trains
    from bicgstab_util import nonassociated_tangent
    from gradient_bench import spread
    from multilevel_bench import ratios
    from multilevel_free_bench import only
    from solver_bench import elastic_tangent
    from tangent_operator_bench import build

    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd import jit
    from fenics_constitutive_amd.gradient import BLOCKS_PER_CU
    from fenics_constitutive_amd.hostio import to_device

    op, force, nodes = build(mesh, args.cells_per_edge, rng)
    nodes = np.ascontiguousarray(nodes, dtype=np.float64)
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
    x_out, y = torch.empty(nd, dtype=torch.float64, device="cuda"), torch.empty(nd, dtype=torch.float64, device="cuda")
    its = args.iterations
    row = {"points": n, "cells": op.n_cells, "nodes": n_nodes, "dofs": nd, "bytes": {"tangent": 8 * 36 * n, "before_any_contender": torch.cuda.memory_allocated()}}

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
    rigid = dict(coarse_space="rigid_body", coordinates=nodes)
    pcs, host = {}, {}
    for cycle in CYCLES:
        for space in SPACES:
            t0 = time.perf_counter()
            on, name = space.split()
            pcs[f"{space} {cycle}"] = fc.MultilevelPreconditioner(A if on == "operator" else K, cycle=cycle, coarsest_nodes=args.coarsest_nodes, **(rigid if name == "rigid_body" else {}))
            host[space] = round(time.perf_counter() - t0, 2)
    new = pcs["operator rigid_body additive"]
    row["hierarchy_and_lists_host_s"] = host
    row["levels"], row["coarse_dofs"], row["chunks"] = new.levels, new.coarse_dofs, len(new._seam.chunks())
    row["resources"] = {"free_rigid_galerkin": new.resources["free_rigid_galerkin"], "free_galerkin": pcs["operator translations additive"].resources["free_galerkin"]}
    routes = tuple(pcs) + ("operator block_jacobi",)

    # ---- (d) every contender built and used once ---------------------------------------------------------------------------------
    whole, batch, first = {}, {}, {}
    values = None
    for route in sorted(routes, key=lambda r: r.startswith("matrix")):  # the operator's first: the values of the matrix do not exist yet
        if route.startswith("matrix") and values is None:
            values, row["bytes"]["values_and_assembly_scratch"] = first_use(lambda: K(tangent))
        target = K if route.startswith("matrix") else A
        pc = pcs.get(route, "block_jacobi")
        first[route] = values if route.startswith("matrix") else tangent
        whole[route] = fc.ConjugateGradient(target, preconditioner=pc, rtol=1e-8, maxiter=args.maxiter)
        batch[route] = fc.ConjugateGradient(target, preconditioner=pc, rtol=0.0, maxiter=its, check_every=its)

        def use():
            res = batch[route](first[route], b, out=x_out)
            assert res.status == "maxiter" and res.iterations == its, (route, res.status, res.iterations)
            whole[route].maxiter, keep = 3, whole[route].maxiter
            assert whole[route](first[route], b, out=x_out).iterations == 3
            whole[route].maxiter = keep

        _, row["bytes"][route] = first_use(use)
    print(json.dumps({mesh: {k: row[k] for k in ("levels", "chunks", "bytes", "hierarchy_and_lists_host_s", "resources")}}), flush=True)

    # ---- (c) the setup of a call and the gathers alone -----------------------------------------------------------------------------
    cap = BLOCKS_PER_CU * jit.num_cu(0)

    def part(pc, what):
        def run():
            with only(what):
                pc._seam.galerkin(pc, 0, tangent, cap)
        return run

    plain, assembled = pcs["operator translations additive"], pcs["matrix rigid_body additive"]
    parts = {"setup operator rigid_body": lambda: new.setup(tangent), "setup operator translations": lambda: plain.setup(tangent),
             "gather operator rigid_body": part(new, GATHERS["operator rigid_body"]), "gather operator translations": part(plain, GATHERS["operator translations"]),
             "element_matrices": part(new, ELEMENTS), "diagonal_blocks": lambda: A.diagonal_blocks(tangent, out=new._device(0).blocks),
             "setup matrix rigid_body": lambda: assembled.setup(values), "assembly": lambda: K(tangent, out=values)}
    times = trains(parts, args.repeats, 1)
    row["setup"] = {name: spread(t) for name, t in times.items()}
    row["setup"]["gather_rigid_body_over_translations"] = ratios([x / c for x, c in zip(times["gather operator rigid_body"], times["gather operator translations"])])
    row["setup"]["setup_rigid_body_over_translations"] = ratios([x / c for x, c in zip(times["setup operator rigid_body"], times["setup operator translations"])])
    print(json.dumps({mesh: {"setup": row["setup"]}}), flush=True)

    # ---- (a) conjugate gradients: one iteration of a batch, the whole solve, alternating ----------------------------------------------
    per_iteration, solves, last = {r: [] for r in routes}, {r: [] for r in routes}, {}
    for _ in range(args.repeats):
        for route in routes:
            ms, res = timed(lambda: batch[route](first[route], b, out=x_out))
            assert res.iterations == its and res.status == "maxiter", (route, res.iterations, res.status)
            per_iteration[route].append(ms / its)
    for rep in range(args.solve_repeats):
        for route in routes:
            ms, res = timed(lambda: whole[route](first[route], b, out=x_out))
            solves[route].append(ms)
            last[route] = res
            print(json.dumps({"mesh": mesh, "repeat": rep, "route": route, "ms": round(ms, 1), "iterations": res.iterations, "status": res.status}), flush=True)
    row["conjugate_gradient"] = cg = {}
    for route in routes:
        res = last[route]
        cg[route] = {"iteration_in_a_batch_with_setup": {**spread(per_iteration[route]), "iterations_per_batch": its},
                     "solve": {**spread(solves[route]), "iterations": res.iterations, "status": res.status, "residual_norm": res.residual_norm, "rhs_norm": res.rhs_norm,
                               "ms_per_iteration": round(float(np.median(solves[route])) / max(res.iterations, 1), 3)}}
    for cycle in CYCLES:  # the new route over every other contender, repeat by repeat
        mine = f"operator rigid_body {cycle}"
        others = (f"operator translations {cycle}", f"matrix rigid_body {cycle}", "operator block_jacobi")
        cg[mine]["solve_time_over"] = {o: ratios([x / c for x, c in zip(solves[mine], solves[o])]) for o in others}
        cg[mine]["batch_iteration_over"] = {o: ratios([x / c for x, c in zip(per_iteration[mine], per_iteration[o])]) for o in others}
        cg[mine]["iterations_over"] = {o: round(last[mine].iterations / max(last[o].iterations, 1), 3) for o in others}
    del whole, batch

    # ---- (b) BiCGStab with the additive cycle on the unsymmetric tangent --------------------------------------------------------------
    unsymmetric = to_device(nonassociated_tangent(n), "cuda")
    K(unsymmetric, out=values)
    contenders = {"operator rigid_body": (fc.MatrixFreeBiCGStab(A, preconditioner=new, rtol=1e-8, maxiter=args.bicgstab_maxiter), unsymmetric),
                  "operator translations": (fc.MatrixFreeBiCGStab(A, preconditioner=plain, rtol=1e-8, maxiter=args.bicgstab_maxiter), unsymmetric),
                  "matrix rigid_body": (fc.BiCGStab(K, preconditioner=assembled, rtol=1e-8, maxiter=args.bicgstab_maxiter), values)}
    for s, t in contenders.values():  # warm: the work vectors
        s.maxiter, keep = 3, s.maxiter
        s(t, b, out=x_out)
        s.maxiter = keep
    ms_of, last = {name: [] for name in contenders}, {}
    for rep in range(args.solve_repeats):
        for name, (s, t) in contenders.items():
            ms, res = timed(lambda: s(t, b, out=x_out))
            true = float(torch.linalg.vector_norm(b - A(unsymmetric, x_out, out=y)) / torch.linalg.vector_norm(b))
            ms_of[name].append(ms)
            last[name] = (res, true)
            print(json.dumps({"mesh": mesh, "repeat": rep, "bicgstab": name, "ms": round(ms, 1), "iterations": res.iterations, "status": res.status}), flush=True)
    row["bicgstab_additive"] = {name: {**spread(ms_of[name]), "iterations": last[name][0].iterations, "status": last[name][0].status,
                                       "residual_norm": last[name][0].residual_norm, "rhs_norm": last[name][0].rhs_norm, "true_residual_over_rhs": last[name][1],
                                       "ms_per_iteration": round(float(np.median(ms_of[name])) / max(last[name][0].iterations, 1), 3)} for name in contenders}
    row["bicgstab_additive"]["rigid_body_over"] = {o: ratios([x / c for x, c in zip(ms_of["operator rigid_body"], ms_of[o])]) for o in ("operator translations", "matrix rigid_body")}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", nargs="+", choices=("hex8", "tet_p2"), default=["hex8", "tet_p2"])
    ap.add_argument("--cells-per-edge", type=int, default=108)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--bicgstab-maxiter", type=int, default=4000)
    ap.add_argument("--coarsest-nodes", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multilevel_free_rigid_bench.json"))
    args = ap.parse_args()
    assert args.solve_repeats >= 3, "at least three alternated repeats"
    if len(args.mesh) > 1:  # a fresh process per mesh; this one starts them and touches no GPU
        for mesh in args.mesh:
            command = [sys.executable, os.path.abspath(__file__), "--mesh", mesh] + [x for k, v in vars(args).items() if k != "mesh"
                                                                                    for x in ("--" + k.replace("_", "-"), str(v))]
            subprocess.run(command, check=True)
        return

    import torch

    assert torch.cuda.is_available(), "multilevel_free_rigid_bench.py measures on the GPU"
    result = {}
    if args.out and os.path.exists(args.out):  # (the other mesh's process wrote its part)
        with open(args.out) as fh:
            result = json.load(fh)
    result.update({"device": torch.cuda.get_device_name(0), "cells_per_edge": args.cells_per_edge, "repeats": args.repeats, "solve_repeats": args.solve_repeats,
                   "rtol": 1e-8, "coarsest_nodes": args.coarsest_nodes})
    mesh = args.mesh[0]
    result[mesh] = measure(mesh, args, np.random.default_rng(1))
    print(json.dumps({mesh: result[mesh]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
