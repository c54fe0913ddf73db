"""NumPy model of PlaneStressFrom3D / UniaxialStressFrom3D around the oracle's 3-D laws (oracle/numpy_oracle.py).

The rule of the fused kernel (kernels/stress_wrapped.h) and of the generic path (wrappers.py), point by point:
the committed 3-D stress row is the cached one with the mapped components from the caller; the unknown strain
increments (plane stress: d_eps_zz; uniaxial stress: d_eps_yy, d_eps_zz) start from the elastic condensation
C^e_bb d = -(sigma0_b + C^e_ba d_eps_a); every iteration evaluates the 3-D law from the committed stress and history;
a point is converged when |sigma_b|_inf <= 1e-12 |sigma|_2 or sigma_b == 0, otherwise d <- d - C_bb^-1 sigma_b with
that iterate's tangent; a point's increment is frozen once converged, so the last evaluation holds every point's
converging iterate.  Outputs: the mapped stress (plane-stress zz exactly 0), the Schur complement
C_aa - C_ab C_bb^-1 C_ba in the low-dimensional layout, the history and the cached 3-D stress row.
"""

from __future__ import annotations

import numpy as np

from oracle import numpy_oracle as O

RTOL = 1e-12
MAX_ITER = 50

VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
RS_P = {"mu": 80769.0, "kappa": 175000.0, "y_0": 1200.0, "h": 200.0}
DP_P = {"mu": 80769.0, "kappa": 175000.0, "a": 100.0, "b": 0.05, "b_flow": 0.02}
DPH_P = {"mu": 80769.0, "kappa": 175000.0, "a": 100.0, "b": 0.05, "d": 40.0, "b_flow": 0.02}
LE_P = {"E": 42.0, "nu": 0.3}


def isotropic(kappa, mu):
    xioi = np.zeros((6, 6))
    xioi[:3, :3] = 1.0
    return kappa * xioi + 2.0 * mu * (np.eye(6) - xioi / 3.0)


# law name -> (oracle function, parameters, history dims, elastic tangent or None, extra keyword arguments)
LAWS = {
    "le": (O.linear_elasticity, LE_P, None, O.elastic_tangent_full(LE_P["E"], LE_P["nu"]), {}),
    "vm": (O.von_mises_3d, VM_P, {"eps_n": 6, "alpha": 1}, isotropic(VM_P["p_ka"], VM_P["p_mu"]), {}),
    "comfe_mises": (O.comfe_mises_plasticity, RS_P, {"history": 7}, isotropic(RS_P["kappa"], RS_P["mu"]), {}),
    "dp": (O.comfe_drucker_prager, DP_P, {"history": 7}, isotropic(DP_P["kappa"], DP_P["mu"]), {"hyperbolic": False}),
    "dp_hyper": (O.comfe_drucker_prager, DPH_P, {"history": 7}, isotropic(DPH_P["kappa"], DPH_P["mu"]), {"hyperbolic": True}),
}

FREE = {"PLANE_STRESS": ((2,), (8,)), "UNIAXIAL_STRESS": ((1, 2), (4, 8))}


def solve_bb(c, r):
    """C_bb^-1 r per point with the kernel's closed forms: c (n, k, k), r (n, k)"""
    if c.shape[1] == 1:
        return r / c[:, 0]
    c11, c12, c21, c22 = c[:, 0, 0], c[:, 0, 1], c[:, 1, 0], c[:, 1, 1]
    det = c11 * c22 - c12 * c21
    r1, r2 = r[:, 0], r[:, 1]
    return np.stack(((c22 * r1 - c12 * r2) / det, (c11 * r2 - c21 * r1) / det), axis=1)


def condense(constraint, s3, t3):
    """(mapped stress, condensed tangent) of 3-D rows s3 (n, 6) and tangents t3 (n, 6, 6)"""
    n = s3.shape[0]
    if constraint == "PLANE_STRESS":
        c = t3[:, :4, :4]
        u = c[:, :, 2] / c[:, 2, 2][:, None]
        ct = c - u[:, :, None] * c[:, 2, None, :]
        ct[:, 2, :] = 0.0
        ct[:, :, 2] = 0.0
        s = s3[:, :4].copy()
        s[:, 2] = 0.0
        return s.reshape(-1), ct.reshape(-1)
    c11, c12, c21, c22, c10, c20 = t3[:, 1, 1], t3[:, 1, 2], t3[:, 2, 1], t3[:, 2, 2], t3[:, 1, 0], t3[:, 2, 0]
    det = c11 * c22 - c12 * c21
    y1, y2 = (c22 * c10 - c12 * c20) / det, (c11 * c20 - c21 * c10) / det
    return s3[:, 0].copy(), (t3[:, 0, 0] - (t3[:, 0, 1] * y1 + t3[:, 0, 2] * y2)).reshape(n)


class StressFrom3DOracle:
    """The stress wrappers around a NumPy 3-D law, behind the model interface of tests/material_point.py."""

    def __init__(self, constraint: str, law: str, fn=None, params=None, history_dim=None, elastic=None, **kw):
        if fn is None:
            fn, params, history_dim, elastic, kw = LAWS[law]
        self.constraint_name = constraint
        self.fn, self.params, self.history_dim, self.elastic, self.kw = fn, params, history_dim, elastic, kw
        self.stress_3d = None
        self.evaluations = None  # per point: law evaluations of the last call
        self.failed = None

    def evaluate(self, t, del_t, grad, stress, tangent, history):
        ps = self.constraint_name == "PLANE_STRESS"
        sd = 4 if ps else 1
        n = stress.size // sd
        g3 = np.zeros((n, 9))
        if ps:
            g3[:, [0, 1, 3, 4]] = grad.reshape(n, 4)
        else:
            g3[:, 0] = grad.reshape(n)
        if self.stress_3d is None or self.stress_3d.shape[0] != n:
            self.stress_3d = np.zeros((n, 6))
        s0 = self.stress_3d.copy()
        s0[:, :sd] = stress.reshape(n, sd)
        h0 = None if history is None else {k: v.copy() for k, v in history.items()}
        b, gb = FREE[self.constraint_name]
        b, gb = list(b), list(gb)
        if self.elastic is None:
            delta = np.zeros((n, len(b)))
        else:
            ce = self.elastic
            rhs = s0[:, b] + g3[:, 0:1] * ce[b, 0]
            if ps:
                rhs = rhs + g3[:, 4:5] * ce[b, 1]
            delta = -solve_bb(np.broadcast_to(ce[np.ix_(b, b)], (n, len(b), len(b))), rhs)
        done = np.zeros(n, dtype=bool)
        failed = np.zeros(n, dtype=bool)
        evals = np.zeros(n, dtype=np.int64)
        s3, t3 = np.zeros((n, 6)), np.zeros((n, 36))
        h = None if h0 is None else {k: v.copy() for k, v in h0.items()}
        for it in range(1, MAX_ITER + 1):
            g3[:, gb] = delta
            s3[:] = s0
            if h0 is not None:
                for k in h:
                    h[k][:] = h0[k]
            self.fn(self.params, t, del_t, g3.reshape(-1), s3.reshape(-1), t3.reshape(-1), h, **self.kw)
            evals[~done] += 1
            r = s3[:, b]
            conv = np.all(r == 0, axis=1) | (np.max(np.abs(r), axis=1) <= RTOL * np.linalg.norm(s3, axis=1))
            done |= conv
            if done.all():
                break
            if it == MAX_ITER:
                failed |= ~done
                break
            with np.errstate(divide="ignore", invalid="ignore"):
                nd = delta - solve_bb(t3.reshape(n, 6, 6)[:, b][:, :, b], r)
            bad = ~done & ~np.all(np.isfinite(nd), axis=1)
            failed |= bad
            done |= bad
            delta = np.where(done[:, None], delta, nd)
        self.evaluations, self.failed = evals, failed
        self.stress_3d = s3.copy()
        s_lo, t_lo = condense(self.constraint_name, s3, t3.reshape(n, 6, 6))
        stress[:] = s_lo
        tangent[:] = t_lo
        if history is not None:
            for k in history:
                history[k][:] = h[k]


def fused_recipe(constraint: str, lname: str, n: int):
    """The inputs of tests/test_gpu_wrappers.py::test_fused_wrapper_equals_map_evaluate_map for the stress wrappers:
    (initial stress, initial history, [gradient of each of four calls with growing plastic sets])."""
    rng = np.random.default_rng(n)
    gd2, sd = (4, 4) if constraint == "PLANE_STRESS" else (1, 1)
    s0 = rng.normal(scale=30.0, size=sd * n)
    dp = lname.startswith("dp")
    if dp:  # compressive prestress: the regime where the reference's Newton iteration converges
        s0.reshape(n, sd)[:, : min(sd, 3)] -= 1000.0 if sd == 4 else 100.0
    if sd == 4:
        s0.reshape(n, 4)[:, 2] = 0.0  # a plane-stress state (the wrapper holds sigma_zz at 0 anyway)
    if lname == "le":
        h0 = None
    elif lname == "vm":
        h0 = {"eps_n": rng.normal(scale=1e-3, size=6 * n), "alpha": rng.uniform(0, 0.02, size=n)}
    else:
        hh = rng.normal(scale=1e-3, size=7 * n)
        hh.reshape(-1, 7)[:, 0] = rng.uniform(0, 0.02, size=n)
        h0 = {"history": hh}
    grads = []
    for call in range(4):
        hi = ((-2.9 if gd2 == 4 else -3.6) if dp else -2.0) + 0.1 * call
        g = rng.normal(size=gd2 * n) * np.repeat(10 ** rng.uniform(-4, hi, size=n), gd2)
        if dp and gd2 == 4:  # mostly isochoric in-plane increments keep the classic surface off its tip
            gv = g.reshape(n, 4)
            tr = gv[:, 0] + gv[:, 3]
            gv[:, 0] -= 0.475 * tr
            gv[:, 3] -= 0.475 * tr
        grads.append(g)
    return s0, h0, grads
