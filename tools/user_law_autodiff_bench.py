"""User laws in autodiff mode against their explicit forms and the built-in laws: LinearElasticityModel,
SpringMaxwellModel (FULL) and VonMises3D as built-in, explicit (userlaw_sources.*) and autodiff (userlaw_sources.*_AD) laws, out
of place (``evaluate_from``) on the SAME device buffers, with the tangent and with ``tangent=None``, in interleaved rounds in one
process.  VonMises3D on the headline mix (benchlib.workloads "von_mises_mixed").  Kernel time from HIP events around each
launch, median over the rounds.

    python tools/user_law_autodiff_bench.py [n=1e8] [rounds=7]
One JSON line per law, implementation and tangent mode, then one summary line per law."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from benchlib.workloads import LE_P, SLS_P, VM_P, synth_inputs  # noqa: E402
from fenics_constitutive_amd import userlaw_sources as S  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda", 0)
os.environ.setdefault("FCAMD_SMALL_CALL_WARNING", "0")
FULL = fc.StressStrainConstraint.FULL

# law -> (built-in, explicit, autodiff, strain scales)
CASES = {
    "linear_elasticity": (lambda: fc.LinearElasticityModel(LE_P, FULL), lambda: S.linear_elasticity(LE_P),
                          lambda: S.linear_elasticity_ad(LE_P), 1e-3),
    "spring_maxwell": (lambda: fc.SpringMaxwellModel(SLS_P, FULL), lambda: S.spring_maxwell(SLS_P),
                       lambda: S.spring_maxwell_ad(SLS_P), 1e-3),
    "von_mises_3d": (lambda: fc.VonMises3D(VM_P), lambda: S.von_mises_3d(VM_P), lambda: S.von_mises_3d_ad(VM_P), "loguniform"),
}

for kind, (make_builtin, make_explicit, make_ad, scale) in CASES.items():
    laws = {"builtin": make_builtin(), "explicit": make_explicit(), "autodiff": make_ad()}
    grad, stress0, hist0 = synth_inputs(kind, scale, n, 7, dev)
    g = grad()
    stress = torch.empty_like(stress0)
    tangent = torch.empty(36 * n, dtype=torch.float64, device=dev)
    hist = None if hist0 is None else {k: torch.empty_like(v) for k, v in hist0.items()}
    variants = [(name, mode) for name in laws for mode in ("tangent", "none")]
    times = {v: [] for v in variants}
    for r in range(rounds + 1):  # round 0: warm-up (module load, first touch)
        for name, mode in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            laws[name].evaluate_from(0.0, 1.0, g, stress0, stress, tangent if mode == "tangent" else None, hist0, hist)
            b.record()
            b.synchronize()
            if r:
                times[(name, mode)].append(a.elapsed_time(b))
    med = {}
    for name, mode in variants:
        ms = sorted(times[(name, mode)])
        med[(name, mode)] = ms[len(ms) // 2]
        extra = {"resources": laws[name].resources} if name != "builtin" and mode == "tangent" else {}
        print(json.dumps({"law": kind, "impl": name, "tangent": mode, "n": n, "ms_median": round(med[(name, mode)], 4),
                          "ms_min": round(ms[0], 4), **extra}), flush=True)
    print(json.dumps({"law": kind,
                      "autodiff_over_explicit": round(med[("autodiff", "tangent")] / med[("explicit", "tangent")], 4),
                      "autodiff_over_builtin": round(med[("autodiff", "tangent")] / med[("builtin", "tangent")], 4),
                      "autodiff_over_explicit_tangent_none": round(med[("autodiff", "none")] / med[("explicit", "none")], 4)}),
          flush=True)
    del laws, g, grad, stress0, hist0, stress, tangent, hist
    torch.cuda.empty_cache()
