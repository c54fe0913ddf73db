#!/usr/bin/env python3
"""A heterogeneous material with a law of one's own: von Mises plasticity with Swift hardening (yield stress
K (eps0 + alpha)^m, ``userlaw_sources.VON_MISES_SWIFT_IMPLICIT``: the residual in, Newton and the consistent tangent out) whose
strength coefficient K is a log-normal random field, one value per quadrature point.  The source is the one of the homogeneous
law: ``K`` moves from ``parameters`` to ``fields`` and ``p.K`` is then the value of the lane's own point.  A few increments of
uniaxial straining on device tensors, with the stress statistics of every step and, as a check, a few points against the
homogeneous law with their K.

    python examples/user_law_fields.py [n_points]
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

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
rng = np.random.default_rng(0)
K = 1500.0 * np.exp(0.25 * rng.standard_normal(n))  # median 1500, about 25 % scatter
scalars = {"p_ka": 175000.0, "p_mu": 80769.0, "eps0": 1e-3, "m": 0.2}
hist_dim = {"eps_n": 6, "alpha": 1}
newton = {"max_iter": 25, "tol": 1e-13}
law = fc.UserLaw(S.VON_MISES_SWIFT_IMPLICIT, scalars, hist_dim, name="swift_random_K", tangent="implicit", unknowns=1, newton=newton,
                 fields={"K": K})
print(f"compiled {law.name}: fields {law.field_names} over {law.field_points} points, scalars {sorted(law.parameters)}, {law.resources}")

dev = torch.device("cuda", 0)
zeros = lambda m: torch.zeros(m, dtype=torch.float64, device=dev)  # noqa: E731
stress, tangent, hist = zeros(6 * n), torch.empty(36 * n, dtype=torch.float64, device=dev), {"eps_n": zeros(6 * n), "alpha": zeros(n)}
probe = np.unique(np.linspace(0, n - 1, 5).astype(int))  # a few points, each run again as a homogeneous law with its own K
probe_state = {i: (zeros(6), torch.empty(36, dtype=torch.float64, device=dev), {"eps_n": zeros(6), "alpha": zeros(1)}) for i in probe}
probe_law = {i: fc.UserLaw(S.VON_MISES_SWIFT_IMPLICIT, dict(scalars, K=float(K[i])), hist_dim, name="swift_one_K", tangent="implicit",
                           unknowns=1, newton=newton) for i in probe}  # one code object: the values are kernel arguments
grad = torch.zeros(n, 9, dtype=torch.float64, device=dev)
grad[:, 0] = 2e-3  # eps_xx increment; lateral strains held at zero
for step in range(5):
    law.evaluate(0.0, 1.0, grad.reshape(-1), stress, tangent, hist, check=True)
    s, a = to_host(stress).reshape(n, 6), to_host(hist["alpha"])
    print(f"step {step}: sigma_xx mean {s[:, 0].mean():9.2f}  std {s[:, 0].std():8.2f}  min {s[:, 0].min():9.2f}  max {s[:, 0].max():9.2f}"
          f"  plastic points {int((a > 0).sum())}  alpha max {a.max():.3e}")
    for i in probe:
        si, ti, hi = probe_state[i]
        probe_law[i].evaluate(0.0, 1.0, grad[i].clone(), si, ti, hi, check=True)
        assert np.array_equal(to_host(si), s[i]), (i, to_host(si), s[i])
assert np.isfinite(to_host(tangent)).all() and (a > 0).all()
# a stronger point carries more stress once every point yields
assert np.corrcoef(K, s[:, 0])[0, 1] > 0.99
