"""The 1-D / 2-D wrappers around user laws: the fused kernel (csrc/jit/user_law_wrapped.hip) against the generic path of
wrappers.py (``fused = False``: convert kernels around a full 3-D evaluate, and an array-level Newton loop around that for the
stress wrappers) on the SAME law and device buffers.  LinearElasticityModel, SpringMaxwellModel and VonMises3D as
explicit and autodiff transcriptions (userlaw_sources) under the four wrappers; where a built-in fused wrapper exists
(LinearElasticityModel, VonMises3D) it is timed too.  ``w.evaluate`` on tensors, in place, from the same committed state every time
(restored outside the timed region); the results of the paths are compared first.  Time from HIP events around each call (the
generic stress wrappers synchronise with the host inside theirs), medians over interleaved rounds in one process.

    python tools/user_law_wrapper_bench.py [n=1e4,1e7] [rounds=7]
One JSON line per law, wrapper and size."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from benchlib.workloads import LE_P, SLS_P, VM_P  # noqa: E402
from fenics_constitutive_amd import userlaw_sources as S  # noqa: E402

sizes = [int(float(x)) for x in (sys.argv[1] if len(sys.argv) > 1 else "1e4,1e7").split(",")]
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda", 0)
os.environ.setdefault("FCAMD_SMALL_CALL_WARNING", "0")
FULL = fc.StressStrainConstraint.FULL
WRAPPERS = {"uniaxial_strain": fc.UniaxialStrainFrom3D, "plane_strain": fc.PlaneStrainFrom3D,
            "plane_stress": fc.PlaneStressFrom3D, "uniaxial_stress": fc.UniaxialStressFrom3D}
# law -> (explicit, autodiff, built-in with a fused wrapper or None, history dims)
LAWS = {
    "linear_elasticity": (lambda: S.linear_elasticity(LE_P), lambda: S.linear_elasticity_ad(LE_P),
                          lambda: fc.LinearElasticityModel(LE_P, FULL), None),
    "spring_maxwell": (lambda: S.spring_maxwell(SLS_P), lambda: S.spring_maxwell_ad(SLS_P), None, {"strain_visco": 6, "strain": 6}),
    "von_mises_3d": (lambda: S.von_mises_3d(VM_P), lambda: S.von_mises_3d_ad(VM_P), lambda: fc.VonMises3D(VM_P), {"eps_n": 6, "alpha": 1}),
}


def inputs(kind, wname, n, seed=7):
    """(gradient, committed mapped stress, committed history) on the device: strains of 1e-4 to 1e-2 per point, so that part of the
    VonMises3D points yield"""
    rng = np.random.default_rng(seed)
    d = 1 if wname.startswith("uniaxial") else 4
    g = rng.normal(size=(n, d)) * 10 ** rng.uniform(-4, -2, size=(n, 1)) * (1.0 if kind == "von_mises_3d" else 0.1)
    s = rng.normal(scale=30.0 if kind == "von_mises_3d" else 0.01, size=(n, d))
    if wname == "plane_stress":
        s[:, 2] = 0.0
    if wname == "uniaxial_stress":
        # the committed stress pulls the way the increment does.  The wrappers' criterion is relative to |sigma|_2, so a point whose
        # axial stress nearly cancels (some of 1e7 random ones would) cannot meet it under either path, and one such point keeps
        # the generic path's array-level loop at its 50 rounds for all
        s = np.abs(s) * np.sign(g)
    hd = LAWS[kind][3]
    h = None if hd is None else {k: (rng.uniform(0, 0.02, size=n * v) if k == "alpha" else rng.normal(scale=1e-3, size=n * v)) for k, v in hd.items()}
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(dev)  # noqa: E731
    return up(g), up(s), None if h is None else {k: up(v) for k, v in h.items()}


class Variant:
    def __init__(self, w, s0, h0, d):
        self.w, self.s0, self.h0 = w, s0, h0
        n = s0.numel() // d
        self.s, self.t = torch.empty_like(s0), torch.empty(d * d * n, dtype=torch.float64, device=dev)
        self.h = None if h0 is None else {k: torch.empty_like(v) for k, v in h0.items()}

    def run(self, g):
        """one call from the committed state and a zero cache; returns the milliseconds of the call"""
        self.s.copy_(self.s0)
        for k in (self.h or {}):
            self.h[k].copy_(self.h0[k])
        if self.w.stress_3d is not None:
            self.w.stress_3d.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self.w.evaluate(0.0, 1.0, g, self.s, self.t, self.h)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


for n in sizes:
    for kind, (make_explicit, make_ad, make_builtin, _) in LAWS.items():
        for wname, W in WRAPPERS.items():
            d = 1 if wname.startswith("uniaxial") else 4
            g, s0, h0 = inputs(kind, wname, n)
            variants = {}
            for mode, make in (("explicit", make_explicit), ("autodiff", make_ad)):
                variants[mode + ".fused"] = Variant(W(make()), s0, h0, d)
                variants[mode + ".generic"] = Variant(W(make()), s0, h0, d)
                variants[mode + ".generic"].w.fused = False
            if make_builtin is not None:
                variants["builtin.fused"] = Variant(W(make_builtin()), s0, h0, d)
            times = {k: [] for k in variants}
            for r in range(rounds + 1):  # round 0: warm-up (compilation, module load, first touch) and the comparison
                for k, v in variants.items():
                    ms = v.run(g)
                    if r:
                        times[k].append(ms)
                if r == 0:
                    diff = {}
                    for mode in ("explicit", "autodiff"):
                        a, b = variants[mode + ".fused"], variants[mode + ".generic"]
                        diff[mode] = max(rel(a.s, b.s), rel(a.t, b.t), rel(a.w.stress_3d, b.w.stress_3d),
                                         *[rel(a.h[k], b.h[k]) for k in (a.h or {})])
                        assert diff[mode] <= (1e-10 if "stress" in wname else 0.0), (kind, wname, mode, diff[mode])
                        assert a.w.model.device_stats(0) == 0
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            line = {"law": kind, "wrapper": wname, "n": n, "ms_median": {k: round(v, 4) for k, v in med.items()},
                    "fused_vs_generic_max_rel_diff": diff}
            for mode in ("explicit", "autodiff"):
                line[mode + "_generic_over_fused"] = round(med[mode + ".generic"] / med[mode + ".fused"], 2)
                law = variants[mode + ".fused"].w.model
                r_ = law.wrapped_resources(variants[mode + ".fused"].w.constraint)
                line[mode + "_resources"] = {k: r_[k] for k in ("vgprs", "scratch_bytes", "rung_waves_per_simd")}
            if "builtin.fused" in med:
                line["explicit_fused_over_builtin_fused"] = round(med["explicit.fused"] / med["builtin.fused"], 2)
            print(json.dumps(line), flush=True)
            del variants, g, s0, h0
            torch.cuda.empty_cache()
