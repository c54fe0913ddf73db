#!/usr/bin/env python3
"""A plasticity law stated the way it is written down: von Mises plasticity with Swift hardening (yield stress
K (eps0 + alpha)^m) as a general return mapping in eight local unknowns -- plastic strain increment, hardening increment and
plastic multiplier -- with the flow rule, the hardening rule and the yield condition as the residual
(``userlaw_sources.VON_MISES_SWIFT_GENERAL``).  The user writes the residual and the update from its solution; the package takes
the Jacobian by dual numbers, runs Newton's method per point, solves the 8 x 8 systems in registers and forms the consistent
tangent by the implicit-function theorem.  A few increments of uniaxial straining on device tensors, against the same law
reduced by hand to one unknown.

    python examples/user_law_implicit.py [n_points]
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
hist_dim = {"eps_n": 6, "alpha": 1}
general = fc.UserLaw(S.VON_MISES_SWIFT_GENERAL, params, hist_dim, name="swift_general", tangent="implicit", unknowns=8,
                     newton={"max_iter": 25, "tol": 1e-13})
reduced = fc.UserLaw(S.VON_MISES_SWIFT_IMPLICIT, params, hist_dim, name="swift_reduced", tangent="implicit", unknowns=1,
                     newton={"max_iter": 25, "tol": 1e-13})
for law in (general, reduced):
    print(f"compiled {law.name}: {law.unknowns} unknowns, newton {law.newton}, {law.resources}")

dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
scale = torch.from_numpy(rng.uniform(0.5, 1.5, n)).to(dev)  # every point strains at its own rate
state = {}
for law in (general, reduced):
    state[law.name] = (torch.zeros(6 * n, dtype=torch.float64, device=dev), torch.empty(36 * n, dtype=torch.float64, device=dev),
                       {"eps_n": torch.zeros(6 * n, dtype=torch.float64, device=dev), "alpha": torch.zeros(n, dtype=torch.float64, device=dev)})
for step in range(5):
    grad = torch.zeros(n, 9, dtype=torch.float64, device=dev)
    grad[:, 0] = 2e-3 * scale  # eps_xx increment; lateral strains held at zero
    for law in (general, reduced):
        stress, tangent, hist = state[law.name]
        law.evaluate(0.0, 1.0, grad.reshape(-1), stress, tangent, hist, check=True)
    s, a, t = (to_host(x) for x in (state["swift_general"][0], state["swift_general"][2]["alpha"], state["swift_general"][1]))
    s1, t1 = to_host(state["swift_reduced"][0]), to_host(state["swift_reduced"][1])
    print(f"step {step}: sigma_xx mean {s.reshape(n, 6)[:, 0].mean():10.2f}  alpha max {a.max():.3e}  "
          f"general against reduced: stress {np.abs(s - s1).max() / np.abs(s1).max():.1e}, tangent {np.abs(t - t1).max() / np.abs(t1).max():.1e}")
    assert np.abs(s - s1).max() <= 1e-9 * np.abs(s1).max() and np.abs(t - t1).max() <= 1e-6 * np.abs(t1).max()
assert np.isfinite(t).all() and (a > 0).all()
