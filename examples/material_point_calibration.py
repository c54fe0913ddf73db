#!/usr/bin/env python3
"""Calibrating a law at the material point: a few thousand Swift-hardening parameter sets (yield stress K (eps0 + alpha)^m,
``userlaw_sources.VON_MISES_SWIFT_AD``) given as per-point fields, every set driven through the same uniaxial-stress tension test
-- 100 increments of eps_xx, every other stress component held at zero -- in ONE launch (``UserLaw.evaluate_path``), and the set
whose stress-strain curve is closest to a synthetic "experiment" picked.  The experiment is the curve of a hidden parameter set,
computed by a one-point law of its own, with a little noise on it.

    python examples/material_point_calibration.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("FCAMD_SMALL_CALL_WARNING", "0")
from fenics_constitutive_amd import userlaw_sources as S  # noqa: E402
from fenics_constitutive_amd.hostio import to_host  # noqa: E402

ELASTIC = {"p_ka": 175000.0, "p_mu": 80769.0}
UNIAXIAL_STRESS = (1, 2, 3, 4, 5)  # every component but sigma_xx is stress-controlled, with target zero
STEPS, EPS_MAX = 100, 0.03

# the candidates: a grid of 16 x 12 x 16 = 3072 parameter sets
K, eps0, m = (g.reshape(-1) for g in np.meshgrid(np.linspace(1500.0, 2500.0, 16), np.linspace(0.005, 0.02, 12),
                                                   np.linspace(0.1, 0.3, 16), indexing="ij"))
n = K.size
hidden = int(np.random.default_rng(7).integers(n))  # the set behind the experiment
truth = {"K": float(K[hidden]), "eps0": float(eps0[hidden]), "m": float(m[hidden])}

# the experiment: one path for all points, eps_xx in equal increments; the targets of the controlled components are zero
load = np.zeros((STEPS, 6))
load[:, 0] = EPS_MAX / STEPS
del_t = np.ones(STEPS)
dev = torch.device("cuda", 0)
zeros = lambda k: torch.zeros(k, dtype=torch.float64, device=dev)  # noqa: E731


def tension_curve(law, points):
    """sigma_xx after every step of the tension test, [STEPS, points], and the lateral strain the test found"""
    stress, history = zeros(6 * points), {"eps_n": zeros(6 * points), "alpha": zeros(points)}
    stress_path, strain_path = zeros(STEPS * points * 6), zeros(STEPS * points * 6)
    failed = law.evaluate_path(0.0, del_t, torch.from_numpy(load).to(dev), stress, history, stress_controlled=UNIAXIAL_STRESS,
                               stress_path=stress_path, strain_path=strain_path, check=True)
    assert int((failed >= 0).sum()) == 0
    return to_host(stress_path).reshape(STEPS, points, 6)[:, :, 0], to_host(strain_path).reshape(STEPS, points, 6)


one = S.von_mises_swift_ad(dict(ELASTIC, **truth))
experiment, _ = tension_curve(one, 1)
experiment = experiment[:, 0] * (1.0 + 2e-4 * np.random.default_rng(1).standard_normal(STEPS))  # measurement noise

law = S.von_mises_swift_ad(dict(ELASTIC, K=K, eps0=eps0, m=m))
res = law.path_resources(UNIAXIAL_STRESS)
print(f"{n} parameter sets as fields {law.field_names}; path kernel: {res['vgprs']} VGPRs, {res['scratch_bytes']} B scratch, "
      f"{res['waves_per_simd']} waves per SIMD")
start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
tension_curve(law, n)  # the first call loads the code object
start.record()
curves, strains = tension_curve(law, n)
stop.record()
stop.synchronize()
print(f"{STEPS} increments of uniaxial stress for {n} sets in one launch: {start.elapsed_time(stop):.2f} ms with the records' download")

misfit = np.sqrt(np.mean((curves - experiment[:, None]) ** 2, axis=0))
best = int(np.argmin(misfit))
print(f"hidden     K = {truth['K']:8.2f}  eps0 = {truth['eps0']:.5f}  m = {truth['m']:.4f}")
print(f"recovered  K = {K[best]:8.2f}  eps0 = {eps0[best]:.5f}  m = {m[best]:.4f}   (rms misfit {misfit[best]:.3f} MPa; "
      f"runner-up {np.partition(misfit, 1)[1]:.3f} MPa)")
# uniaxial stress found the lateral contraction: between the elastic nu = 0.3 and the plastic 0.5
nu_eff = -strains[-1, best, 1] / strains[-1, best, 0]
print(f"lateral contraction ratio of the last increment: {nu_eff:.4f}")
assert best == hidden and 0.3 < nu_eff < 0.5, (best, hidden, nu_eff)
print("OK")
