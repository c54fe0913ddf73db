"""NumPy model of ``UserLaw.evaluate_path`` around any law's in-place ``evaluate``, and the reference's
material-point scenarios (material_point_cases.py) written as load paths.

``drive_path`` is ``MaterialPoints.increment`` over a whole path with a stopping rule per point instead of the maximum over all
points: a point that has converged keeps its strain increment while the others iterate on, so its last evaluation repeats its
result, and a point whose control loop does not converge keeps its committed state, records NaN from that step on and takes no
further part.  The law's own return code is not visible through ``evaluate``; only control failures are modelled.
"""

from __future__ import annotations

import numpy as np

import material_point_cases as cases
from material_point import grad_from_mandel_strain


def path_times(t0, del_t) -> np.ndarray:
    """t_k of every step, accumulated sequentially in double as ``MaterialPoints.time`` is"""
    out, t = np.empty(len(del_t)), float(t0)
    for k, dt in enumerate(del_t):
        out[k] = t
        t += float(dt)
    return out


def drive_path(law, t0, del_t, load, stress, history, stress_controlled=(), max_iter=25, tol=1e-10, stress_path=None, strain_path=None):
    """The algorithm of one step, per point, for every step; ``stress`` [6 n] and ``history`` (dict or None) are updated in place
    and the first failed step of every point (-1: completed) is returned."""
    n, S = stress.size // 6, len(del_t)
    ctrl = list(stress_controlled)
    load = np.broadcast_to(load[:, None, :], (S, n, 6)) if load.ndim == 2 else load
    failed = np.full(n, -1, dtype=np.int32)
    times = path_times(t0, del_t)
    tangent = np.zeros(36 * n)
    for k in range(S):
        de = np.array(load[k], dtype=np.float64)
        target = de[:, ctrl].copy()
        de[:, ctrl] = 0.0
        active = failed < 0
        control_failed = np.zeros(n, dtype=bool)
        it = 0
        while True:
            st = stress.copy()  # every evaluation starts from the step's committed state
            ht = None if history is None else {name: h.copy() for name, h in history.items()}
            law.evaluate(times[k], float(del_t[k]), grad_from_mandel_strain(de, "FULL"), st, tangent, ht)
            if not ctrl:
                break
            r = st.reshape(n, 6)[:, ctrl] - target
            with np.errstate(invalid="ignore"):
                conv = np.max(np.abs(r), axis=1) <= tol  # False for a NaN
            step = active & ~control_failed & ~conv & (it < max_iter)  # a singular J has ended the point's loop
            control_failed |= active & ~conv & ~step
            if not step.any():
                break
            J = tangent.reshape(n, 6, 6)[:, ctrl][:, :, ctrl]
            for p in np.nonzero(step)[0]:
                try:
                    de[p, ctrl] -= np.linalg.solve(J[p], r[p])
                except np.linalg.LinAlgError:
                    control_failed[p] = True
            it += 1
        commit = active & ~control_failed
        failed[active & control_failed] = k
        stress.reshape(n, 6)[commit] = st.reshape(n, 6)[commit]
        if history is not None:
            for name, h in history.items():
                h.reshape(n, -1)[commit] = ht[name].reshape(n, -1)[commit]
        for rec, val in ((stress_path, st.reshape(n, 6)), (strain_path, de)):
            if rec is not None:
                rec.reshape(S, n, 6)[k] = np.where(commit[:, None], val, np.nan)
    return failed


# --- the reference's material-point scenarios as load paths: (del_t [S], load [S, n, 6], stress_controlled) -----------------------

def uniaxial_stress_path(n=8):
    """material_point_cases.uniaxial_stress_3d: 100 increments of eps_xx, sigma_yy = sigma_zz = 0"""
    amp = 0.05 * cases._amplitudes(n)
    cur = np.linspace(0, 1, 101)[1:, None] * amp[None, :]
    return _strain_path(cur)


def cyclic_strain_path(n=4):
    """material_point_cases.uniaxial_cyclic_strain_3d: one sine cycle of eps_xx, sigma_yy = sigma_zz = 0"""
    amp = 0.05 * cases._amplitudes(n, 0.8, 1.0)
    cur = np.sin(np.linspace(np.pi, -np.pi, 101))[:, None] * amp[None, :]
    return _strain_path(cur)


def _strain_path(cur):
    S, n = cur.shape
    load = np.zeros((S, n, 6))
    prev = np.zeros(n)
    for k in range(S):  # the increments as the scenarios form them: cur - prev
        load[k, :, 0] = cur[k] - prev
        prev = cur[k]
    return np.ones(S), load, (1, 2)


def sls_del_t():
    """the time increments of the relaxation and creep scenarios: 1e-8, then 2.0 while time < 20 tau"""
    dts, t = [1e-8], 1e-8
    while t < 20 * cases.SLS["tau"]:
        dts.append(2.0)
        t += 2.0
    return np.array(dts)


def relaxation_path(n=5):
    """material_point_cases.relaxation, FULL: eps_xx = d in the first step, then held; sigma_yy = sigma_zz = 0"""
    dts = sls_del_t()
    load = np.zeros((len(dts), n, 6))
    load[0, :, 0] = 0.01 * cases._amplitudes(n)
    return dts, load, (1, 2)


def creep_path(n=5):
    """material_point_cases.creep, FULL: the traction sigma_xx = f held, sigma_yy = sigma_zz = 0, no shear strain"""
    dts = sls_del_t()
    load = np.zeros((len(dts), n, 6))
    load[:, :, 0] = 0.1 * cases._amplitudes(n)
    return dts, load, (0, 1, 2)


def load_curve(stress_path):
    """the scenarios' load curve: sigma_xx after every step behind the zero start"""
    return np.vstack([np.zeros((1, stress_path.shape[1])), stress_path[:, :, 0]])


#: golden key -> (path, curve from (stress_path, strain_path) as [S, n, 6]).  The creep curve is the history's total strain_xx,
#: the running sum of the applied increments
SCENARIOS = {
    "uniaxial_stress_3d.load": ("von_mises_3d", uniaxial_stress_path, 8, lambda s, e: load_curve(s)),
    "uniaxial_cyclic_strain_3d.load": ("von_mises_3d", cyclic_strain_path, 4, lambda s, e: load_curve(s)),
    "relaxation.spring_maxwell.FULL": ("spring_maxwell", relaxation_path, 5, lambda s, e: s[:, :, 0]),
    "creep.spring_maxwell.FULL": ("spring_maxwell", creep_path, 5, lambda s, e: np.cumsum(e[:, :, 0], axis=0)),
}
HISTORY = {"von_mises_3d": {"eps_n": 6, "alpha": 1}, "spring_maxwell": {"strain_visco": 6, "strain": 6}}
PARAMS = {"von_mises_3d": cases.VM, "spring_maxwell": cases.SLS}
