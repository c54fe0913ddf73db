"""NumPy port of userlaw_sources.VON_MISES_SWIFT_AD (von Mises plasticity with Swift hardening, sigma_y = K (eps0 + alpha)^m):
stress, history and the non-convergence flags of a batch of points, point by point in the source's expression order."""

import numpy as np

SWIFT_P = {"p_ka": 175000.0, "p_mu": 80769.0, "K": 1500.0, "eps0": 1e-3, "m": 0.2}


def swift_evaluate(p, eps, sigma, eps_n, alpha, max_iter=50):
    """``eps`` (n, 6) Mandel strain increments, ``sigma`` (n, 6), ``eps_n`` (n, 6), ``alpha`` (n,): the committed state.
    Returns (sigma, eps_n, alpha, status) of the trial state."""
    mu, s23 = p["p_mu"], np.sqrt(2.0 / 3.0)
    n = eps.shape[0]
    s_out, e_out, a_out = sigma.copy(), eps_n.copy(), alpha.copy()
    status = np.zeros(n, dtype=np.int64)
    I = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    for q in range(n):
        e, s = eps[q], sigma[q]
        tr_eps = (e[0] + e[1]) + e[2]
        tr_sig = (s[0] + s[1]) + s[2]
        del_sigtr = 2.0 * mu * (e - tr_eps * I / 3.0)
        sigtr = (s - tr_sig * I / 3.0) + del_sigtr
        sq = sigtr[0] * sigtr[0]
        for i in range(1, 6):
            sq = sq + sigtr[i] * sigtr[i]
        sigtrn = np.sqrt(sq)
        a0 = p["eps0"] + alpha[q]
        phitr = sigtrn - s23 * (p["K"] * a0 ** p["m"])
        xn = np.zeros(6)
        g = 0.0
        if phitr > 0.0:
            xn = sigtr / sigtrn
            it = 0
            while True:
                a = a0 + s23 * g
                sy = p["K"] * a ** p["m"]
                r = (sigtrn - 2.0 * mu * g) - s23 * sy
                done = abs(r) <= 1e-10 * sy
                if not done and it >= max_iter:
                    status[q] = 1
                    break
                dr = -2.0 * mu - 2.0 / 3.0 * p["m"] * (sy / a)
                g = g - r / dr
                if done:
                    break
                it += 1
        e_out[q] = eps_n[q] + g * xn
        s_out[q] = s + ((p["p_ka"] * tr_eps * I + del_sigtr) - 2.0 * mu * g * xn)
        a_out[q] = alpha[q] + s23 * g
    return s_out, e_out, a_out, status
