"""User-defined laws against the built-in kernels: the UserLaw transcriptions of LinearElasticityModel,
SpringMaxwellModel (FULL) and VonMises3D (fenics_constitutive_amd.userlaw_sources) and the built-in laws, out of place
(``evaluate_from``: committed arrays in, trial arrays and the whole tangent out) on the SAME device buffers, in interleaved rounds
in one process.  VonMises3D on the headline mix (benchlib.workloads "von_mises_mixed": log-uniform strain scales, 22 % plastic).
Kernel time from HIP events around each launch, median over the rounds, next to the algorithmic bytes of the call.

    python tools/user_law_bench.py [n=1e8] [rounds=7]
One JSON line per law and implementation, then one summary line per law."""

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

# law -> (built-in, user law, strain scales, algorithmic bytes per point of evaluate_from: grad 72, stress 48 + 48, tangent 288,
# every history array read and written)
CASES = {
    "linear_elasticity": (lambda: fc.LinearElasticityModel(LE_P, FULL), lambda: S.linear_elasticity(LE_P), 1e-3, 456),
    "spring_maxwell": (lambda: fc.SpringMaxwellModel(SLS_P, FULL), lambda: S.spring_maxwell(SLS_P), 1e-3, 456 + 2 * 96),
    "von_mises_3d": (lambda: fc.VonMises3D(VM_P), lambda: S.von_mises_3d(VM_P), "loguniform", 456 + 2 * 56),
}

for kind, (make_builtin, make_user, scale, bytes_pt) in CASES.items():
    laws = {"builtin": make_builtin(), "user": make_user()}
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
    plastic = None
    if kind == "von_mises_3d":  # the share of plastic points of this mix: the built-in law's counters
        plastic = laws["builtin"].device_stats(0).n_plastic / n
    med = {}
    for name in laws:
        ms = sorted(times[name])
        med[name] = ms[len(ms) // 2]
        extra = {"resources": laws[name].resources} if name == "user" else {}
        print(json.dumps({"law": kind, "impl": name, "n": n, "ms_median": round(med[name], 4), "ms_min": round(ms[0], 4),
                          "algorithmic_bytes_per_point": bytes_pt, "ms_per_GB": round(med[name] / (bytes_pt * n / 1e9), 5),
                          "TB_s": round(bytes_pt * n / (med[name] * 1e-3) / 1e12, 3), "plastic_fraction": plastic, **extra}), flush=True)
    print(json.dumps({"law": kind, "user_over_builtin": round(med["user"] / med["builtin"], 4)}), flush=True)
    del laws, g, grad, stress0, hist0, stress, tangent, hist
    torch.cuda.empty_cache()
