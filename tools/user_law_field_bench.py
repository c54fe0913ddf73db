"""What a per-point parameter field of a user law costs: von_mises_3d (explicit tangent) with 0, 1 (p_y0) and 5
fields and von_mises_swift_implicit with 0 and 1 (K) fields, out of place (``evaluate_from``) on the SAME device buffers, with the
tangent, in interleaved rounds in one process, on the headline mix (benchlib.workloads "von_mises_mixed").  Every field is
filled with the scalar it replaces, so all variants of a law do the same arithmetic on the same points and differ in the
8 bytes per point and field they stream, and in the registers their per-lane constants take.  Kernel time from HIP events
around each launch, median over the rounds.

The law with 0 fields is the yardstick.  Next to measured / yardstick the tool prints the byte-proportional estimate
(568 + 8 k) / 568 for k fields (568 bytes per point: gradient, committed and new stress and history, tangent), their ratio, and
the same ratio of the built-in field kernels (1.013 with one field, 1.022 with five; 2.6 % between rounds).

    python tools/user_law_field_bench.py [n=1e8] [rounds=7]
One JSON line per law and number of fields, then one summary line per law."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchlib.workloads import VM_P, synth_inputs  # noqa: E402
from fenics_constitutive_amd import userlaw_sources as S  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda", 0)
os.environ.setdefault("FCAMD_SMALL_CALL_WARNING", "0")
SWIFT_P = {"p_ka": VM_P["p_ka"], "p_mu": VM_P["p_mu"], "K": 1500.0, "eps0": 1e-3, "m": 0.2}
BYTES = 8 * (9 + 6 + 6 + 36 + 2 * 7)  # per point without fields
BUILTIN = {1: 1.013, 5: 1.022}  # measured / estimate of the built-in field kernels


def with_fields(p, names):
    """``p`` with the parameters ``names`` as constant device fields of their scalar"""
    return {k: (torch.full((n,), float(v), dtype=torch.float64, device=dev) if k in names else v) for k, v in p.items()}


# law -> (factory, parameters, the field sets measured; the first, without fields, is the yardstick)
CASES = {
    "von_mises_3d": (S.von_mises_3d, VM_P, [(), ("p_y0",), tuple(VM_P)]),
    "von_mises_swift_implicit": (S.von_mises_swift_implicit, SWIFT_P, [(), ("K",)]),
}

for kind, (make, p, field_sets) in CASES.items():
    laws = {len(names): make(with_fields(p, names)) for names in field_sets}
    grad, stress0, hist0 = synth_inputs("von_mises_3d", "loguniform", n, 7, dev)
    g = grad()
    stress = torch.empty_like(stress0)
    tangent = torch.empty(36 * n, dtype=torch.float64, device=dev)
    hist = {k: torch.empty_like(v) for k, v in hist0.items()}
    times = {k: [] for k in laws}
    for r in range(rounds + 1):  # round 0: warm-up (module load, field upload, first touch)
        for k, law in laws.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            law.evaluate_from(0.0, 1.0, g, stress0, stress, tangent, hist0, hist)
            b.record()
            b.synchronize()
            if r:
                times[k].append(a.elapsed_time(b))
    plastic = float((hist["alpha"] != hist0["alpha"]).double().mean())
    med = {}
    for k, law in laws.items():
        ms = sorted(times[k])
        med[k] = ms[len(ms) // 2]
        print(json.dumps({"law": kind, "fields": k, "field_names": list(law.field_names), "n": n, "ms_median": round(med[k], 4),
                          "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "gb_per_s": round((BYTES + 8 * k) * n / med[k] / 1e6, 1),
                          "resources": law.resources}), flush=True)
    summary = {"law": kind, "plastic_fraction": round(plastic, 4)}
    for k in laws:
        if k:
            estimate = (BYTES + 8 * k) / BYTES
            summary[f"fields_{k}"] = {"measured_over_0_fields": round(med[k] / med[0], 4), "estimate": round(estimate, 4),
                                      "measured_over_estimate": round(med[k] / med[0] / estimate, 4),
                                      "builtin_measured_over_estimate": BUILTIN.get(k)}
    print(json.dumps(summary), flush=True)
    del laws, g, grad, stress0, hist0, stress, tangent, hist
    torch.cuda.empty_cache()
