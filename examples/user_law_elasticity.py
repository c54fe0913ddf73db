#!/usr/bin/env python3
"""A constitutive law of one's own on the GPU: linear elasticity written as a ``UserLaw`` point function -- the counterpart of the
reference's C++ elasticity tutorial (docs/custom_models/) -- evaluated on NumPy arrays and on device tensors and compared with the
built-in ``LinearElasticityModel``.

The point function below is all the user writes.  The package compiles it for gfx950 at run time (hiprtc) inside a kernel
template that does the memory work: coalesced 16-byte streams, the transposition through LDS, the ragged last tile.  Written
with the library's helpers (``le_entries``, ``row_times_matrix_fma``) it reproduces the built-in kernel bit for bit.

    python examples/user_law_elasticity.py [n_points]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("FCAMD_SMALL_CALL_WARNING", "0")
import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402

SOURCE = r"""
// sigma += eps @ D, tangent = D: UserParams holds E and nu (generated from the parameters dict)
__device__ int fcamd_user_point(const UserParams& p, double t, double del_t, const double (&grad)[9], const double (&eps)[6],
                                double (&sigma)[6], double (&D)[36], UserHistory& h) {
    fcamd_elastic_matrix(le_entries(p.E, p.nu), D);
    double ds[6];
    row_times_matrix_fma(eps, D, ds);
    for (int i = 0; i < 6; ++i) sigma[i] = sigma[i] + ds[i];
    return 0;  // converged
}
"""

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_003
params = {"E": 42.0, "nu": 0.3}
law = fc.UserLaw(SOURCE, params, history_dim=None, name="my_elasticity")
builtin = fc.LinearElasticityModel(params, fc.StressStrainConstraint.FULL)
print(f"compiled {law.name}: {law.resources}")

rng = np.random.default_rng(0)
grad = rng.normal(scale=1e-3, size=9 * n)
stress0 = rng.normal(size=6 * n)

# NumPy arrays: synchronous, in place
s_user, t_user = stress0.copy(), np.zeros(36 * n)
law.evaluate(0.0, 1.0, grad, s_user, t_user, None)
s_ref, t_ref = stress0.copy(), np.zeros(36 * n)
builtin.evaluate(0.0, 1.0, grad, s_ref, t_ref, None)
print("ndarray: stress bit-identical:", np.array_equal(s_user, s_ref), " tangent bit-identical:", np.array_equal(t_user, t_ref))

# device tensors: asynchronous on torch's current stream
g = to_device(grad, "cuda")
s_dev, t_dev = to_device(stress0, "cuda"), torch.empty(36 * n, dtype=torch.float64, device="cuda")
law.evaluate(0.0, 1.0, g, s_dev, t_dev, None, check=True)
print("tensor:  stress bit-identical:", np.array_equal(to_host(s_dev), s_ref), " tangent bit-identical:",
      np.array_equal(to_host(t_dev), t_ref))
assert np.array_equal(s_user, s_ref) and np.array_equal(to_host(t_dev), t_ref)
