#!/usr/bin/env python3
"""A law of one's own in a 2-D and in a 1-D problem: von Mises plasticity with Swift hardening (yield stress K (eps0 + alpha)^m),
written as a ``UserLaw`` in autodiff mode, under ``PlaneStressFrom3D`` and under ``UniaxialStressFrom3D``.

User laws are 3-D; the wrappers run one as a single kernel compiled from the law's own source: per point it pads the 2-D / 1-D
gradient, solves the out-of-plane strain increments that make the constrained stresses vanish (a Newton iteration in registers
on the law's own tangent entries, here dual-number partials), and writes the mapped stress and the condensed tangent.  Only the
wrapper's cached 3-D stress exists next to the low-dimensional arrays.

    python examples/user_law_plane_stress.py [n_points]
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
params = {"p_ka": 175000.0, "p_mu": 80769.0, "K": 1500.0, "eps0": 1e-3, "m": 0.2, "max_iter": 50.0}
history_dim = {"eps_n": 6, "alpha": 1}
dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
scale = torch.from_numpy(rng.uniform(0.5, 1.5, n)).to(dev)  # every point strains at its own rate


def zeros(k):
    return torch.zeros(k * n, dtype=torch.float64, device=dev)


def new_law():
    return fc.UserLaw(S.VON_MISES_SWIFT_AD, params, history_dim, name="swift", tangent="autodiff")


# --- plane stress: biaxial stretching with some shear -----------------------------------------------------------------------------
law = new_law()
w = fc.PlaneStressFrom3D(law)
print(f"plane stress kernel: {law.wrapped_resources(w.constraint)}")
stress, tangent = zeros(4), zeros(16)
hist = {"eps_n": zeros(6), "alpha": zeros(1)}
for step in range(5):
    grad = torch.zeros(n, 4, dtype=torch.float64, device=dev)  # row-major 2x2 displacement-gradient increment
    grad[:, 0] = 2e-3 * scale
    grad[:, 3] = -5e-4 * scale
    grad[:, 1] = grad[:, 2] = 3e-4 * scale
    w.evaluate(0.0, 1.0, grad.reshape(-1), stress, tangent, hist)
    assert law.device_stats(0) == 0  # neither the law's own Newton iteration nor the wrapper's failed anywhere
    s, a, t = to_host(stress).reshape(n, 4), to_host(hist["alpha"]), to_host(tangent).reshape(n, 4, 4)
    s3 = to_host(w.stress_3d).reshape(n, 6)
    print(f"plane stress   step {step}: sigma_xx mean {s[:, 0].mean():9.2f}  alpha max {a.max():.3e}  "
          f"|sigma_zz| / |sigma| max {np.max(np.abs(s3[:, 2]) / np.linalg.norm(s3, axis=1)):.1e}  C_xxxx mean {t[:, 0, 0].mean():.5g}")
assert np.all(s[:, 2] == 0.0) and np.all(t[:, 2, :] == 0.0) and np.all(t[:, :, 2] == 0.0)
assert np.isfinite(t).all() and (a > 0).all()
assert w.grad_del_u_3d is None and w.tangent_3d is None  # no 3-D gradient or tangent array was ever made

# --- uniaxial stress: a tension test ---------------------------------------------------------------------------------------------
law = new_law()
w = fc.UniaxialStressFrom3D(law)
print(f"uniaxial stress kernel: {law.wrapped_resources(w.constraint)}")
stress, tangent = zeros(1), zeros(1)
hist = {"eps_n": zeros(6), "alpha": zeros(1)}
young = 9.0 * params["p_ka"] * params["p_mu"] / (3.0 * params["p_ka"] + params["p_mu"])
for step in range(5):
    w.evaluate(0.0, 1.0, 2e-3 * scale, stress, tangent, hist)
    assert law.device_stats(0) == 0
    s, a, t = to_host(stress), to_host(hist["alpha"]), to_host(tangent)
    print(f"uniaxial stress step {step}: sigma_xx mean {s.mean():9.2f}  alpha max {a.max():.3e}  "
          f"d sigma / d eps in [{t.min():.5g}, {t.max():.5g}]  (Young's modulus {young:.5g})")
# in the plastic range the uniaxial stress is the yield stress and the tangent the elastoplastic modulus, far below Young's
yield_stress = params["K"] * (params["eps0"] + a) ** params["m"]
assert np.max(np.abs(s - yield_stress)) <= 1e-6 * yield_stress.max()
assert (t < 0.2 * young).all() and (t > 0).all()
print("OK")
