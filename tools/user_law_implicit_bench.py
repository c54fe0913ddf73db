"""User laws in implicit mode against their autodiff forms and the built-in law: VonMises3D as built-in,
autodiff (userlaw_sources.von_mises_3d_ad) and implicit (von_mises_3d_implicit) law, and the Swift law as autodiff
(von_mises_swift_ad), implicit in one unknown (von_mises_swift_implicit) and as the general return mapping in eight
(von_mises_swift_general); out of place (``evaluate_from``) on the SAME device buffers, with the tangent and with
``tangent=None``, in interleaved rounds in one process, on the headline mix (benchlib.workloads "von_mises_mixed").  Kernel time
from HIP events around each launch, median over the rounds.

    python tools/user_law_implicit_bench.py [n=1e8] [rounds=7]
One JSON line per law, implementation and tangent mode, then one summary line per law."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from benchlib.workloads import VM_P, synth_inputs  # noqa: E402
from fenics_constitutive_amd import userlaw_sources as S  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda", 0)
os.environ.setdefault("FCAMD_SMALL_CALL_WARNING", "0")
SWIFT_P = {"p_ka": VM_P["p_ka"], "p_mu": VM_P["p_mu"], "K": 1500.0, "eps0": 1e-3, "m": 0.2}

# law -> {implementation: factory}; the first one is the yardstick of the summary line
CASES = {
    "von_mises_3d": {"autodiff": lambda: S.von_mises_3d_ad(VM_P), "builtin": lambda: fc.VonMises3D(VM_P),
                     "implicit": lambda: S.von_mises_3d_implicit(VM_P)},
    "von_mises_swift": {"autodiff": lambda: S.von_mises_swift_ad(SWIFT_P), "implicit": lambda: S.von_mises_swift_implicit(SWIFT_P),
                        "general": lambda: S.von_mises_swift_general(SWIFT_P)},
}

for kind, makers in CASES.items():
    laws = {name: make() for name, make in makers.items()}
    grad, stress0, hist0 = synth_inputs("von_mises_3d", "loguniform", n, 7, dev)
    g = grad()
    stress = torch.empty_like(stress0)
    tangent = torch.empty(36 * n, dtype=torch.float64, device=dev)
    hist = {k: torch.empty_like(v) for k, v in hist0.items()}
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
    plastic = float((hist["alpha"] != hist0["alpha"]).double().mean())
    med = {}
    for name, mode in variants:
        ms = sorted(times[(name, mode)])
        med[(name, mode)] = ms[len(ms) // 2]
        extra = {"resources": laws[name].resources} if name != "builtin" and mode == "tangent" else {}
        print(json.dumps({"law": kind, "impl": name, "tangent": mode, "n": n, "ms_median": round(med[(name, mode)], 4),
                          "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), **extra}), flush=True)
    print(json.dumps({"law": kind, "plastic_fraction": round(plastic, 4),
                      **{f"{name}_over_autodiff{'_tangent_none' if mode == 'none' else ''}": round(med[(name, mode)] / med[("autodiff", mode)], 4)
                         for name, mode in variants if name != "autodiff"}}), flush=True)
    del laws, g, grad, stress0, hist0, stress, tangent, hist
    torch.cuda.empty_cache()
