#!/usr/bin/env python3
"""A plasticity law the engine does not ship, with the tangent for free: von Mises plasticity with Swift hardening
(yield stress K (eps0 + alpha)^m), written as a ``UserLaw`` in autodiff mode.  The user writes only the stress and history
update, as a template over the scalar type (``userlaw_sources.VON_MISES_SWIFT_AD``); the package differentiates it in forward
mode (dual numbers) inside the kernel.  A few increments of uniaxial straining on device tensors, stress and tangent out.

    python examples/user_law_autodiff.py [n_points]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("FCAMD_SMALL_CALL_WARNING", "0")
import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import userlaw_sources as S  # noqa: E402
from fenics_constitutive_amd.hostio import to_host  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
params = {"p_ka": 175000.0, "p_mu": 80769.0, "K": 1500.0, "eps0": 1e-3, "m": 0.2}
law = fc.UserLaw(S.VON_MISES_SWIFT_AD, dict(params, max_iter=50.0), {"eps_n": 6, "alpha": 1}, name="swift", tangent="autodiff")
print(f"compiled {law.name}: {law.resources}")

dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
scale = torch.from_numpy(rng.uniform(0.5, 1.5, n)).to(dev)  # every point strains at its own rate
stress = torch.zeros(6 * n, dtype=torch.float64, device=dev)
tangent = torch.empty(36 * n, dtype=torch.float64, device=dev)
hist = {"eps_n": torch.zeros(6 * n, dtype=torch.float64, device=dev), "alpha": torch.zeros(n, dtype=torch.float64, device=dev)}
for step in range(5):
    grad = torch.zeros(n, 9, dtype=torch.float64, device=dev)
    grad[:, 0] = 2e-3 * scale  # eps_xx increment; lateral strains held at zero
    law.evaluate(0.0, 1.0, grad.reshape(-1), stress, tangent, hist, check=True)
    s, a, t = to_host(stress).reshape(n, 6), to_host(hist["alpha"]), to_host(tangent).reshape(n, 6, 6)
    print(f"step {step}: sigma_xx mean {s[:, 0].mean():10.2f}  alpha max {a.max():.3e}  D_xx range [{t[:, 0, 0].min():.4g}, "
          f"{t[:, 0, 0].max():.4g}]")
assert np.isfinite(t).all() and (a > 0).all()
