#!/usr/bin/env python3
"""Simple shear with the Jaumann rate: linear elasticity wrapped in ``fc.JaumannRate`` is sheared to gamma = 2 pi in equal
increments of the displacement gradient on the current configuration, G = d_gamma e1 (x) e2.  Without the rotation the shear
stress grows without bound (mu gamma); with it the stress follows Dienes' solution sigma_11 = -sigma_22 = mu (1 - cos gamma),
sigma_12 = mu sin gamma, the error falling with the square of the step.

    python examples/simple_shear_jaumann.py [n_points] [steps]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("FCAMD_SMALL_CALL_WARNING", "0")
import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd.hostio import to_host  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 400
E, nu = 42.0, 0.3
mu = E / (2 * (1 + nu))
dev = torch.device("cuda", 0)
law = fc.JaumannRate(fc.LinearElasticityModel({"E": E, "nu": nu}, fc.StressStrainConstraint.FULL))
print(f"path: {law.path}, kernel resources: {law.resources}")

gamma = 2 * np.pi
grad = torch.zeros(n, 9, dtype=torch.float64, device=dev)
grad[:, 1] = gamma / steps  # G[0][1]: row-major
grad = grad.reshape(-1)
stress = torch.zeros(6 * n, dtype=torch.float64, device=dev)
for k in range(1, steps + 1):
    law.evaluate(0.0, 1.0, grad, stress, None, None)
    if k % (steps // 4) == 0:
        g = k * gamma / steps
        s = to_host(stress).reshape(n, 6)[0]
        print(f"gamma {g:6.3f}: sigma_11 {s[0]:9.5f} (Dienes {mu * (1 - np.cos(g)):9.5f})  sigma_22 {s[1]:9.5f}  "
              f"sigma_12 {s[3] / np.sqrt(2):9.5f} (Dienes {mu * np.sin(g):9.5f})")
s = to_host(stress).reshape(n, 6)
err = np.abs(s[:, 3] / np.sqrt(2) - mu * np.sin(gamma)).max()
print(f"max |sigma_12 - mu sin(2 pi)| over {n} points: {err:.3e} (mu = {mu:.4f})")
assert err < 1e-3 * mu
