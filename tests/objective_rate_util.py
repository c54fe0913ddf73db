"""NumPy oracle of the objective-rate rotation (fenics_constitutive_amd.JaumannRate, csrc/jit/rotation.h): the Hughes-Winget
rotation of an increment gradient and R S R^T of Mandel 6-vectors [xx, yy, zz, r xy, r xz, r yz], r = sqrt(2)
(the order of the reference's strain_from_grad_u, models/utils.py:199-204)."""

import numpy as np

R2 = np.sqrt(2.0)
PAIRS = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]


def hughes_winget(G):
    """R = (I - W / 2)^-1 (I + W / 2), W = (G - G^T) / 2, G row-major 3x3"""
    G = np.asarray(G, dtype=np.float64).reshape(3, 3)
    A = 0.25 * (G - G.T)
    eye = np.eye(3)
    return np.linalg.solve(eye - A, eye + A)


def hughes_winget_closed(G):
    """the closed form I + 2 / (1 + |a|^2) (A + A^2), a the axial vector of A = W / 2"""
    G = np.asarray(G, dtype=np.float64).reshape(3, 3)
    A = 0.25 * (G - G.T)
    a = np.array([A[2, 1], A[0, 2], A[1, 0]])
    return np.eye(3) + 2.0 / (1.0 + a @ a) * (A + A @ A)


def to_tensor(v):
    v = np.asarray(v, dtype=np.float64)
    T = np.empty((3, 3))
    for m, (i, j) in enumerate(PAIRS):
        T[i, j] = T[j, i] = v[m] if i == j else v[m] / R2
    return T


def to_mandel(T):
    return np.array([T[i, j] if i == j else R2 * T[i, j] for i, j in PAIRS])


def rotate(R, v):
    """Mandel(R S R^T)"""
    return to_mandel(R @ to_tensor(v) @ R.T)


def rotate_state(grad, stress, history, blocks):
    """the rotated committed state of n points: ``grad`` [9 n], ``stress`` [6 n], ``history`` {name: [dim n]}, ``blocks``
    {name: [offsets]}; new arrays"""
    n = grad.size // 9
    g = grad.reshape(n, 9)
    s = stress.reshape(n, 6).copy()
    h = {k: v.reshape(n, -1).copy() for k, v in (history or {}).items()}
    for p in range(n):
        R = hughes_winget(g[p])
        s[p] = rotate(R, s[p])
        for name, offs in blocks.items():
            for o in offs:
                h[name][p, o:o + 6] = rotate(R, h[name][p, o:o + 6])
    return s.reshape(-1), {k: v.reshape(-1) for k, v in h.items()}
