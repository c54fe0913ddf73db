"""``UserLaw.evaluate_path`` against the same path as S launches of the existing stress-only kernel: the UserLaw
transcriptions of LinearElasticityModel, SpringMaxwellModel (FULL) and VonMises3D, S = 100 steps, a path shared by all points and a
path per point, strain control and ``(1, 2)`` stress control, on the SAME device buffers in interleaved rounds in one process.

The sequential run is the baseline: S ``evaluate_from`` calls (tangent=None) that read step k - 1's block of the stress record
and write step k's, the history ping-ponging between two sets of arrays, on gradients built beforehand.  Under stress control
it replays the strain increments the path launch recorded, strain-controlled: the same result, and a lower bound of a host Newton
loop, which would need several launches with a tangent per step.  Time from HIP events around the whole sequence and around the
one launch, median over the rounds.

    python tools/path_bench.py [n=1e4,1e6] [steps=100] [rounds=5]
One JSON line per law, n, path kind and control set."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchlib.workloads import LE_P, SLS_P, VM_P  # noqa: E402
from fenics_constitutive_amd import userlaw_sources as S  # noqa: E402

sizes = [int(float(x)) for x in (sys.argv[1] if len(sys.argv) > 1 else "1e4,1e6").split(",")]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda", 0)
os.environ.setdefault("FCAMD_SMALL_CALL_WARNING", "0")

# law -> (constructor, history dims, strain increment per step at amplitude one)
CASES = {
    "linear_elasticity": (lambda: S.linear_elasticity(LE_P), {}, 1e-5),
    "spring_maxwell": (lambda: S.spring_maxwell(SLS_P), {"strain_visco": 6, "strain": 6}, 1e-5),
    "von_mises_3d": (lambda: S.von_mises_3d(VM_P), {"eps_n": 6, "alpha": 1}, 2e-4),  # amplitudes 0.2 ... 2: yield between step 18 and never
}
SQ2 = 2 ** 0.5


def gradients(load):
    """[S, n, 6] Mandel increments -> [S, 9 n] symmetric gradients (tests/material_point.py: grad_from_mandel_strain)"""
    S_, n = load.shape[:2]
    g = torch.zeros(S_, n, 9, dtype=torch.float64, device=dev)
    g[:, :, 0], g[:, :, 4], g[:, :, 8] = load[:, :, 0], load[:, :, 1], load[:, :, 2]
    g[:, :, 1] = g[:, :, 3] = load[:, :, 3] / SQ2
    g[:, :, 2] = g[:, :, 6] = load[:, :, 4] / SQ2
    g[:, :, 5] = g[:, :, 7] = load[:, :, 5] / SQ2
    return g.reshape(S_, 9 * n)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


for kind, (make, hist_dim, de) in CASES.items():
    law = make()
    for n in sizes:
        zeros = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)  # noqa: E731
        amp = torch.linspace(0.2, 2.0, n, dtype=torch.float64, device=dev)
        base = torch.tensor([1.0, -0.3, -0.3, 0.2, 0.0, 0.0], dtype=torch.float64, device=dev) * de
        dts = np.ones(steps)
        for per_point in (False, True):
            for ctrl in ((), (1, 2)):
                load = (amp[None, :, None] * base[None, None, :]).expand(steps, n, 6).contiguous() if per_point \
                    else (base[None, :] * 1.1).expand(steps, 6).contiguous()
                if ctrl:
                    load[..., list(ctrl)] = 0.0
                stress_path, strain_path = zeros(steps, n * 6), zeros(steps, n * 6)
                stress0 = zeros(6 * n)
                hist = [{k: zeros(d * n) for k, d in hist_dim.items()} for _ in range(3)]  # the path's, and the ping-pong pair

                def path():
                    stress0.zero_()
                    for h in hist[0].values():
                        h.zero_()
                    return law.evaluate_path(0.0, dts, load, stress0, hist[0] or None, stress_controlled=ctrl,
                                             stress_path=stress_path, strain_path=strain_path if ctrl else None)

                failed = path()  # also records the strain increments the sequential run replays under stress control
                assert int((failed >= 0).sum()) == 0
                full = load if per_point else load[:, None, :].expand(steps, n, 6)
                grads = gradients(strain_path.reshape(steps, n, 6) if ctrl else full)
                reference = stress_path.clone()

                def sequential():
                    stress0.zero_()
                    for h in hist[1].values():
                        h.zero_()
                    for k in range(steps):
                        law.evaluate_from(float(k), 1.0, grads[k], stress_path[k - 1] if k else stress0, stress_path[k], None,
                                          hist[1 + k % 2] or None, hist[1 + (k + 1) % 2] or None)

                sequential()
                torch.cuda.synchronize()
                assert torch.equal(stress_path, reference), "the sequential run does not reproduce the path launch bit for bit"
                t = {"path": [], "sequential": []}
                for r in range(rounds):
                    t["sequential"].append(timed(sequential))
                    t["path"].append(timed(path))
                med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
                res = law.path_resources(ctrl)
                print(json.dumps({"law": kind, "n": n, "steps": steps, "load": "per_point" if per_point else "shared",
                                  "stress_controlled": list(ctrl), "path_ms": round(med["path"], 4),
                                  "sequential_ms": round(med["sequential"], 4), "speedup": round(med["sequential"] / med["path"], 3),
                                  "path_us_per_step": round(1e3 * med["path"] / steps, 3), "vgprs": res["vgprs"],
                                  "waves_per_simd": res["waves_per_simd"]}), flush=True)
                del grads, reference, stress_path, strain_path, load, hist, stress0
                torch.cuda.empty_cache()
