"""Helpers of the per-point parameter field tests of user laws (test_user_law_fields.py, test_gpu_user_law_fields.py): the laws and
their parameter sets, the scattered groups, the gradients of the three load steps and the CPU ports that say which points are
plastic in the last step."""

import numpy as np

from fenics_constitutive_amd import userlaw_sources as S
from fenics_constitutive_amd.userlaw import FACTOR_PY
from objective_rate_util import rotate_state
from oracle import numpy_oracle as O
from swift_law_util import swift_evaluate

SIZES = [1, 63, 64, 65, 1000, 70_003]
N_MAX = max(SIZES)
STEPS = 3
VM_H = {"eps_n": 6, "alpha": 1}
SLS_H = {"strain_visco": 6, "strain": 6}

# family -> four parameter sets; the first is the one of the constant-field tests
GROUPS = {
    "le": [{"E": 210000.0, "nu": 0.3}, {"E": 70000.0, "nu": 0.33}, {"E": 30000.0, "nu": 0.2}, {"E": 1000.0, "nu": 0.45}],
    "sls": [{"E0": 42.0, "E1": 10.0, "tau": 10.0, "nu": 0.2}, {"E0": 70000.0, "E1": 3000.0, "tau": 0.5, "nu": 0.33},
            {"E0": 300.0, "E1": 900.0, "tau": 2.0, "nu": 0.1}, {"E0": 1000.0, "E1": 10.0, "tau": 100.0, "nu": 0.45}],
    "vm": [{"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 250.0, "p_y00": 2500.0, "p_w": 200.0},
           {"p_ka": 68000.0, "p_mu": 26000.0, "p_y0": 120.0, "p_y00": 400.0, "p_w": 50.0},
           {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 600.0, "p_y00": 900.0, "p_w": 10.0},
           {"p_ka": 16700.0, "p_mu": 12500.0, "p_y0": 30.0, "p_y00": 60.0, "p_w": 500.0}],
    "swift": [{"p_ka": 175000.0, "p_mu": 80769.0, "K": 1500.0, "eps0": 1e-3, "m": 0.2},
              {"p_ka": 68000.0, "p_mu": 26000.0, "K": 500.0, "eps0": 2e-3, "m": 0.1},
              {"p_ka": 175000.0, "p_mu": 80769.0, "K": 3000.0, "eps0": 5e-3, "m": 0.3},
              {"p_ka": 16700.0, "p_mu": 12500.0, "K": 200.0, "eps0": 1e-3, "m": 0.15}],
}
# law (a helper of userlaw_sources) -> (family, history)
LAWS = {
    "linear_elasticity": ("le", None), "spring_maxwell": ("sls", SLS_H), "von_mises_3d": ("vm", VM_H),
    "linear_elasticity_ad": ("le", None), "spring_maxwell_ad": ("sls", SLS_H), "von_mises_3d_ad": ("vm", VM_H),
    "von_mises_3d_implicit": ("vm", VM_H), "von_mises_swift_implicit": ("swift", VM_H), "von_mises_swift_general": ("swift", VM_H),
}
PLASTIC_FAMILIES = ("vm", "swift")
_laws = {}


def _key(v):
    return ("field", v.tobytes()) if isinstance(v, np.ndarray) else float(v)


def make(name, p, **kw):
    """one instance per (helper, parameters, keywords) for the session; the code objects are shared anyway"""
    key = (name, tuple((k, _key(v)) for k, v in p.items()), tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _laws:
        _laws[key] = getattr(S, name)(p, **kw)
    return _laws[key]


def scalars(name, gi=0):
    return dict(GROUPS[LAWS[name][0]][gi])


def constant_fields(p, n, names=None):
    """``p`` with the parameters ``names`` (default: all) as fields filled with their scalar"""
    return {k: (np.full(n, float(v)) if (names is None or k in names) and not isinstance(v, np.ndarray) else v) for k, v in p.items()}


def group_of(n):
    """every tile mixes the four groups and the pattern shifts from tile to tile"""
    i = np.arange(n)
    return (i + i // 64) % 4


def group_fields(family, n, names=None):
    """the four sets of ``family`` scattered by ``group_of``; ``names``: the parameters that are fields (the others: set 0's)"""
    sets, group = GROUPS[family], group_of(n)
    return {k: (np.array([s[k] for s in sets])[group] if names is None or k in names else v) for k, v in sets[0].items()}


def lognormal_fields(family, n, names=None, seed=7):
    """continuous fields over two decades among scalars; ``names`` default: the stiffness and the yield parameter (VonMises3D:
    p_mu and p_y0 as in test_gpu_point_fields.py; Swift: p_mu and K)"""
    rng = np.random.default_rng(seed)
    p = dict(GROUPS[family][0])
    for k in names or (("p_mu", "p_y0") if family == "vm" else ("p_mu", "K")):
        p[k] = (p[k] * 10 ** rng.uniform(-1.0, 1.0, size=N_MAX))[:n].copy()
    return p


_grads = {}


def grads(n, spin=0.0):
    """the gradients of the three load steps, [9 n] each: the first n points of one set of N_MAX, so a point's state does not
    depend on n.  Points 4 k .. 4 k + 3 are elastic (k % 3 == 0: 1e-6), mixed (k % 3 == 1: log-uniform magnitudes) or plastic in
    every parameter set (k % 3 == 2), which gives every group of ``group_of`` all three kinds among the first 63 points.
    ``spin``: the standard deviation of an antisymmetric part added to every gradient (0: as drawn)"""
    if spin not in _grads:
        rng = np.random.default_rng(2024)
        kind = (np.arange(N_MAX) // 4) % 3
        scale = np.where(kind == 0, 1e-6, np.where(kind == 1, 10 ** rng.uniform(-4.0, -2.5, size=N_MAX),
                                                    10 ** rng.uniform(-2.5, -2.1, size=N_MAX)))
        gs = []
        for _ in range(STEPS):
            g = rng.normal(size=(N_MAX, 9)) * scale[:, None]
            if spin:
                w = rng.normal(scale=spin, size=(N_MAX, 3))
                g[:, 1] += w[:, 0]; g[:, 3] -= w[:, 0]
                g[:, 2] += w[:, 1]; g[:, 6] -= w[:, 1]
                g[:, 5] += w[:, 2]; g[:, 7] -= w[:, 2]
            gs.append(g)
        _grads[spin] = gs
    return [g[:n].reshape(-1).copy() for g in _grads[spin]]


def symmetric(gs):
    """the symmetric parts of the gradients: no spin, the same strain"""
    out = []
    for g in gs:
        G = g.reshape(-1, 3, 3)
        out.append((0.5 * (G + G.transpose(0, 2, 1))).reshape(-1))
    return out


def mandel(g):
    g = g.reshape(-1, 9)
    return np.stack([g[:, 0], g[:, 4], g[:, 8], FACTOR_PY * (g[:, 1] + g[:, 3]), FACTOR_PY * (g[:, 2] + g[:, 6]),
                     FACTOR_PY * (g[:, 5] + g[:, 7])], axis=1)


def point_params(p, i):
    return {k: (float(v[i]) if isinstance(v, np.ndarray) else float(v)) for k, v in p.items()}


def port_steps(family, p, gs, rows=None, max_iter_last=50, rotate=False):
    """the CPU port of the plastic families over the load steps ``gs`` from a zero state, for the points ``rows`` (default: all):
    ``oracle.numpy_oracle`` (VonMises3D) or ``swift_law_util`` (Swift).  ``p``: scalars, or per-point arrays over all points of
    ``gs`` -- then the port runs point by point.  Returns (stress [m, 6], tangent [m, 36] (VonMises3D) or None, eps_n [m, 6],
    alpha [m], plastic [m]: alpha changed in the last step, status [m] of the last step (Swift; ``max_iter_last`` Newton steps)).
    ``rotate``: the committed stress and eps_n turn with the Hughes-Winget rotation of the step's gradient first (JaumannRate)"""
    n = gs[0].size // 9
    rows = np.arange(n) if rows is None else np.asarray(rows)
    m = rows.size
    fields = any(isinstance(v, np.ndarray) for v in p.values())
    s, t, e, a = np.zeros((m, 6)), np.zeros((m, 36)), np.zeros((m, 6)), np.zeros(m)
    status = np.zeros(m, dtype=np.int64)
    for step, g in enumerate(gs):
        g = g.reshape(n, 9)[rows]
        a_prev = a.copy()
        last = step == len(gs) - 1
        if rotate:
            sr, hr = rotate_state(g.reshape(-1), s.reshape(-1), {"eps_n": e.reshape(-1)}, {"eps_n": [0]})
            s, e = sr.reshape(m, 6), hr["eps_n"].reshape(m, 6)
        if family == "vm":
            if fields:
                for j, i in enumerate(rows):
                    sj, tj, hj = s[j].copy(), t[j].copy(), {"eps_n": e[j].copy(), "alpha": a[j:j + 1].copy()}
                    O.von_mises_3d(point_params(p, i), 0.0, 1.0, g[j].copy(), sj, tj, hj)
                    s[j], t[j], e[j], a[j] = sj, tj, hj["eps_n"], hj["alpha"][0]
            else:
                sf, tf, h = s.reshape(-1), t.reshape(-1), {"eps_n": e.reshape(-1), "alpha": a}
                O.von_mises_3d(p, 0.0, 1.0, g.reshape(-1), sf, tf, h)
        else:
            eps = mandel(g)
            mi = max_iter_last if last else 50
            if fields:
                for j, i in enumerate(rows):
                    sj, ej, aj, st = swift_evaluate(point_params(p, i), eps[j:j + 1], s[j:j + 1], e[j:j + 1], a[j:j + 1], max_iter=mi)
                    s[j], e[j], a[j], status[j] = sj[0], ej[0], aj[0], st[0]
            else:
                s, e, a, status = swift_evaluate(p, eps, s, e, a, max_iter=mi)
            t = None
    return s, t, e, a, a != a_prev, status


def plastic_of(family, alpha_before, alpha_after):
    """the points whose accumulated plastic strain changed in the last step (the GPU tests' side of the condition)"""
    return np.asarray(alpha_after) != np.asarray(alpha_before)


def assert_mixed(plastic, group=None, what=""):
    """at least one elastic and one plastic point, in every group when ``group`` is given"""
    plastic = np.asarray(plastic)
    for gi in ([None] if group is None else range(4)):
        sel = plastic if gi is None else plastic[group == gi]
        assert sel.any() and (~sel).any(), f"{what} group {gi}: {int(sel.sum())} plastic of {sel.size} points"
