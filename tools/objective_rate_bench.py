"""Objective-rate wrapper (fenics_constitutive_amd.JaumannRate) against the laws it wraps, out of place
(``evaluate_from``: committed arrays in, trial arrays and the whole tangent out) on the SAME device buffers, in interleaved rounds
in one process.  Fused path: LinearElasticityModel, SpringMaxwellModel (FULL) and VonMises3D on the headline mix (benchlib.workloads
"von_mises_mixed": log-uniform strain scales), each against its unrotated userlaw_sources transcription (the same kernel without
the rotation) and the built-in law.  Array-level path: MisesPlasticityLinearHardening3D (comfe-rs) against the unwrapped law.
The synthetic gradients are full random matrices: every point has a finite spin.  Kernel time from HIP events around each call
(the array-level call is two launches), median over the rounds.

    python tools/objective_rate_bench.py [n=1e8] [rounds=7]
One JSON line per law and implementation, then one summary line per law."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from benchlib.workloads import LE_P, RS_P, SLS_P, VM_P, synth_inputs  # noqa: E402
from fenics_constitutive_amd import userlaw_sources as S  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda", 0)
os.environ.setdefault("FCAMD_SMALL_CALL_WARNING", "0")
FULL = fc.StressStrainConstraint.FULL
RS = {k: np.array([v]) for k, v in RS_P.items()}

# law -> (implementations, strain scales, the implementation the wrapper is compared with)
CASES = {
    "linear_elasticity": ({"jaumann": lambda: fc.JaumannRate(fc.LinearElasticityModel(LE_P, FULL)),
                           "unrotated": lambda: S.linear_elasticity(LE_P),
                           "builtin": lambda: fc.LinearElasticityModel(LE_P, FULL)}, 1e-3, "unrotated"),
    "spring_maxwell": ({"jaumann": lambda: fc.JaumannRate(fc.SpringMaxwellModel(SLS_P, FULL)),
                        "unrotated": lambda: S.spring_maxwell(SLS_P),
                        "builtin": lambda: fc.SpringMaxwellModel(SLS_P, FULL)}, 1e-3, "unrotated"),
    "von_mises_3d": ({"jaumann": lambda: fc.JaumannRate(fc.VonMises3D(VM_P)),
                      "unrotated": lambda: S.von_mises_3d(VM_P),
                      "builtin": lambda: fc.VonMises3D(VM_P)}, "loguniform", "unrotated"),
    "comfe_mises_plasticity": ({"jaumann": lambda: fc.JaumannRate(fc.MisesPlasticityLinearHardening3D(RS)),
                                "builtin": lambda: fc.MisesPlasticityLinearHardening3D(RS)}, "loguniform", "builtin"),
}

for kind, (makers, scale, base) in CASES.items():
    laws = {k: m() for k, m in makers.items()}
    grad, stress0, hist0 = synth_inputs(kind, scale, n, 7, dev)
    g = grad()
    stress = torch.empty_like(stress0)
    tangent = torch.empty(36 * n, dtype=torch.float64, device=dev)
    hist = None if hist0 is None else {k: torch.empty_like(v) for k, v in hist0.items()}
    times = {k: [] for k in laws}
    for r in range(rounds + 1):  # round 0: warm-up (module load, first touch)
        for name, law in laws.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            law.evaluate_from(0.0, 1.0, g, stress0, stress, tangent, hist0, hist)
            b.record()
            b.synchronize()
            if r:
                times[name].append(a.elapsed_time(b))
    med = {}
    for name, law in laws.items():
        ms = sorted(times[name])
        med[name] = ms[len(ms) // 2]
        extra = {}
        if isinstance(law, fc.JaumannRate):
            extra = {"path": law.path, "resources": law.resources}
        elif isinstance(law, fc.UserLaw):
            extra = {"resources": law.resources}
        print(json.dumps({"law": kind, "impl": name, "n": n, "ms_median": round(med[name], 4), "ms_min": round(ms[0], 4),
                          "ms_max": round(ms[-1], 4), **extra}), flush=True)
    print(json.dumps({"law": kind, f"jaumann_over_{base}": round(med["jaumann"] / med[base], 4),
                      "jaumann_over_builtin": round(med["jaumann"] / med["builtin"], 4)}), flush=True)
    del laws, g, grad, stress0, hist0, stress, tangent, hist
    torch.cuda.empty_cache()
