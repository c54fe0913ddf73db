"""Three built-in laws written as ``UserLaw`` point functions: starting points for laws of one's own, and the yardsticks of the
user-law kernel template (tests/test_gpu_user_law.py, tools/user_law_bench.py).

* ``LINEAR_ELASTICITY``: LinearElasticityModel (FULL) with the library's ``le_entries`` and the ascending-k FMA product -- bit for
  bit the built-in kernel's stress and tangent.
* ``SPRING_MAXWELL``: SpringMaxwellModel (FULL), the reference's NumPy expression order (models/spring_maxwell_model.py:56-88).
* ``VON_MISES_3D``: VonMises3D, the reference's per-point return mapping and Newton stopping rule
  (models/mises_plasticity_isotropic_hardening.py:74-175); a point whose Newton iteration exceeds 100 steps returns 1.

The same three in autodiff form (``tangent="autodiff"``: stress and history only, the tangent by forward-mode automatic
differentiation; contract in ``csrc/jit/user_law_ad.h``), each in the expression order of its explicit form, so stress and
history are bit-identical to it: ``LINEAR_ELASTICITY_AD``, ``SPRING_MAXWELL_AD``, ``VON_MISES_3D_AD``.  And one law the engine
does not ship, in autodiff form only:

* ``VON_MISES_SWIFT_AD``: von Mises plasticity with Swift hardening, yield stress ``K (eps0 + alpha)^m``, radial return with a
  per-point Newton iteration on the plastic multiplier; a point that has not converged after ``max_iter`` steps returns 1.

And three laws in implicit form (``tangent="implicit"``: the residual and the update from its solution; Jacobian, Newton loop,
dense solve and consistent tangent are the kernel template's; contract in ``csrc/jit/user_law_implicit.h``):

* ``VON_MISES_3D_IMPLICIT``: VonMises3D's hardening, one unknown (the plastic multiplier), the yield residual divided by the
  yield stress.
* ``VON_MISES_SWIFT_IMPLICIT``: the Swift law, one unknown, the residual divided by sigma_y.
* ``VON_MISES_SWIFT_GENERAL``: the Swift law as a general return mapping in eight unknowns ``(d eps_p[6], d alpha, d gamma)``:
  flow rule, hardening rule and yield condition as they are written down, nothing reduced by hand.

Every helper constructor takes a NumPy array or a tensor for any of its parameters and hands it to ``UserLaw(fields=...)``: a
per-point parameter field.  Scalars go where they always went, and a call with scalars only builds the program it always built.
"""

from __future__ import annotations

from .interfaces import StressStrainConstraint
from .userlaw import UserLaw

__all__ = ["LINEAR_ELASTICITY", "SPRING_MAXWELL", "VON_MISES_3D", "linear_elasticity", "spring_maxwell", "von_mises_3d",
           "LINEAR_ELASTICITY_AD", "SPRING_MAXWELL_AD", "VON_MISES_3D_AD", "VON_MISES_SWIFT_AD", "linear_elasticity_ad",
           "spring_maxwell_ad", "von_mises_3d_ad", "von_mises_swift_ad", "VON_MISES_3D_IMPLICIT", "VON_MISES_SWIFT_IMPLICIT",
           "VON_MISES_SWIFT_GENERAL", "von_mises_3d_implicit", "von_mises_swift_implicit", "von_mises_swift_general"]

LINEAR_ELASTICITY = r"""
// sigma += eps @ D ; tangent = D
__device__ int fcamd_user_point(const UserParams& p, double t, double del_t, const double (&grad)[9], const double (&eps)[6],
                                double (&sigma)[6], double (&D)[36], UserHistory& h) {
    fcamd_elastic_matrix(le_entries(p.E, p.nu), D);
    double ds[6];
    row_times_matrix_fma(eps, D, ds);
    for (int i = 0; i < 6; ++i) sigma[i] = sigma[i] + ds[i];
    return 0;
}
"""

SPRING_MAXWELL = r"""
// "x @ M" of the NumPy law: row_times_matrix_fma (the ascending-k FMA chain of the built-in kernels)
__device__ int fcamd_user_point(const UserParams& p, double t, double del_t, const double (&grad)[9], const double (&eps)[6],
                                double (&sigma)[6], double (&D)[36], UserHistory& h) {
    double D0[36], D1[36], D01[36];
    fcamd_elastic_matrix(le_entries(p.E0, p.nu), D0);
    fcamd_elastic_matrix(le_entries(p.E1, p.nu), D1);
    for (int i = 0; i < 36; ++i) D01[i] = D0[i] + D1[i];
    const double mu1 = p.E1 / (2.0 * (1.0 + p.nu));
    const double factor = 1.0 / del_t + 1.0 / p.tau;
    const double c = 1.0 / (p.tau * 2.0 * mu1);
    double x[6], y[6], ds[6], dev_v[6];
    for (int i = 0; i < 6; ++i) x[i] = c * (h.strain[i] + eps[i]);
    row_times_matrix_fma(x, D1, y);
    for (int i = 0; i < 6; ++i) dev_v[i] = 1.0 / factor * (y[i] - 1.0 / p.tau * h.strain_visco[i]);
    row_times_matrix_fma(eps, D01, ds);
    for (int i = 0; i < 6; ++i) sigma[i] = sigma[i] + (ds[i] - 2.0 * mu1 * dev_v[i]);
    const double r = 1.0 - 1.0 / (p.tau * factor);
    for (int i = 0; i < 36; ++i) D[i] = D0[i] + r * D1[i];
    for (int i = 0; i < 6; ++i) {
        h.strain_visco[i] = h.strain_visco[i] + dev_v[i];
        h.strain[i] = h.strain[i] + eps[i];
    }
    return 0;
}
"""

VON_MISES_3D = r"""
__device__ int fcamd_user_point(const UserParams& p, double t, double del_t, const double (&grad)[9], const double (&eps)[6],
                                double (&sigma)[6], double (&D)[36], UserHistory& h) {
    const double mu = p.p_mu, s23 = sqrt(2.0 / 3.0), dy = p.p_y00 - p.p_y0;
    const double tr_eps = (eps[0] + eps[1]) + eps[2];
    const double tr_sig = (sigma[0] + sigma[1]) + sigma[2];
    double del_sigtr[6], sigtr[6];
    for (int i = 0; i < 6; ++i) {
        const double I = i < 3 ? 1.0 : 0.0;
        del_sigtr[i] = 2.0 * mu * (eps[i] - tr_eps * I / 3.0);
        sigtr[i] = (sigma[i] - tr_sig * I / 3.0) + del_sigtr[i];
    }
    double sq = sigtr[0] * sigtr[0];
    for (int i = 1; i < 6; ++i) sq = sq + sigtr[i] * sigtr[i];
    const double sigtrn = sqrt(sq);
    const double a_n = h.alpha[0];
    const double phitr = sigtrn - s23 * (p.p_y0 + dy * (1.0 - exp(-p.p_w * a_n)));
    double xn[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double g1 = 0.0, xc1 = 0.0, xc2 = 0.0;
    int status = 0;
    if (phitr > 0.0) {
        double g0 = 1.0, xr = 1.0;
        int it = 0;
        for (int i = 0; i < 6; ++i) xn[i] = sigtr[i] / sigtrn;
        while (fabs(xr) > 1e-12 && fabs(g1 - g0) > 1e-8 * fabs(g1)) {
            g0 = g1;
            ++it;
            const double ex = exp(-p.p_w * (a_n + s23 * g0));
            xr = sigtrn - 2.0 * mu * g0 - s23 * (p.p_y0 + dy * (1.0 - ex));
            const double xg = -2.0 * mu - 2.0 / 3.0 * dy * p.p_w * ex;
            g1 = g0 - xr / xg;
            if (it > 100) {
                status = 1;
                break;
            }
        }
        const double xg = -2.0 * mu - 2.0 / 3.0 * dy * p.p_w * exp(-p.p_w * (a_n + s23 * g1));
        xc1 = -1.0 / xg;
        xc2 = g1 / sigtrn;
    }
    for (int i = 0; i < 6; ++i) {
        const double I = i < 3 ? 1.0 : 0.0;
        h.eps_n[i] = h.eps_n[i] + g1 * xn[i];
        sigma[i] = sigma[i] + ((p.p_ka * tr_eps * I + del_sigtr[i]) - 2.0 * mu * g1 * xn[i]);
    }
    h.alpha[0] = h.alpha[0] + s23 * g1;
    const double B = 2.0 * mu * (1.0 - 2.0 * mu * xc2);
    const double Cc = 4.0 * mu * mu * (xc2 - xc1);
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            const double ioi = (i < 3 && j < 3) ? 1.0 : 0.0;
            const double pp = (i == j ? 1.0 : 0.0) - 1.0 / 3.0 * ioi;
            D[6 * i + j] = (p.p_ka * ioi + B * pp) + Cc * (xn[i] * xn[j]);
        }
    return status;
}
"""

LINEAR_ELASTICITY_AD = r"""
// sigma += eps @ D: the ascending-k FMA chain; its derivative with a unit seed in eps_j is exactly row j of D
template <class T>
__device__ int fcamd_user_stress(const UserParams& p, double t, double del_t, const T (&eps)[6], T (&sigma)[6], UserHistoryT<T>& h) {
    double D[36];
    fcamd_elastic_matrix(le_entries(p.E, p.nu), D);
    T ds[6];
    row_times_matrix_fma(eps, D, ds);
    for (int i = 0; i < 6; ++i) sigma[i] = sigma[i] + ds[i];
    return 0;
}
"""

SPRING_MAXWELL_AD = r"""
template <class T>
__device__ int fcamd_user_stress(const UserParams& p, double t, double del_t, const T (&eps)[6], T (&sigma)[6], UserHistoryT<T>& h) {
    double D0[36], D1[36], D01[36];
    fcamd_elastic_matrix(le_entries(p.E0, p.nu), D0);
    fcamd_elastic_matrix(le_entries(p.E1, p.nu), D1);
    for (int i = 0; i < 36; ++i) D01[i] = D0[i] + D1[i];
    const double mu1 = p.E1 / (2.0 * (1.0 + p.nu));
    const double factor = 1.0 / del_t + 1.0 / p.tau;
    const double c = 1.0 / (p.tau * 2.0 * mu1);
    T x[6], y[6], ds[6], dev_v[6];
    for (int i = 0; i < 6; ++i) x[i] = c * (h.strain[i] + eps[i]);
    row_times_matrix_fma(x, D1, y);
    for (int i = 0; i < 6; ++i) dev_v[i] = 1.0 / factor * (y[i] - 1.0 / p.tau * h.strain_visco[i]);
    row_times_matrix_fma(eps, D01, ds);
    for (int i = 0; i < 6; ++i) sigma[i] = sigma[i] + (ds[i] - 2.0 * mu1 * dev_v[i]);
    for (int i = 0; i < 6; ++i) {
        h.strain_visco[i] = h.strain_visco[i] + dev_v[i];
        h.strain[i] = h.strain[i] + eps[i];
    }
    return 0;
}
"""

VON_MISES_3D_AD = r"""
// the return mapping of VON_MISES_3D without its tangent block: the Newton loop is differentiated through its iterations
template <class T>
__device__ int fcamd_user_stress(const UserParams& p, double t, double del_t, const T (&eps)[6], T (&sigma)[6], UserHistoryT<T>& h) {
    const double mu = p.p_mu, s23 = sqrt(2.0 / 3.0), dy = p.p_y00 - p.p_y0;
    const T tr_eps = (eps[0] + eps[1]) + eps[2];
    const T tr_sig = (sigma[0] + sigma[1]) + sigma[2];
    T del_sigtr[6], sigtr[6];
    for (int i = 0; i < 6; ++i) {
        const double I = i < 3 ? 1.0 : 0.0;
        del_sigtr[i] = 2.0 * mu * (eps[i] - tr_eps * I / 3.0);
        sigtr[i] = (sigma[i] - tr_sig * I / 3.0) + del_sigtr[i];
    }
    T sq = sigtr[0] * sigtr[0];
    for (int i = 1; i < 6; ++i) sq = sq + sigtr[i] * sigtr[i];
    const T sigtrn = sqrt(sq);
    const T a_n = h.alpha[0];
    const T phitr = sigtrn - s23 * (p.p_y0 + dy * (1.0 - exp(-p.p_w * a_n)));
    T xn[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    T g1 = 0.0;
    int status = 0;
    if (phitr > 0.0) {
        T g0 = 1.0, xr = 1.0;
        int it = 0;
        for (int i = 0; i < 6; ++i) xn[i] = sigtr[i] / sigtrn;
        while (fabs(xr) > 1e-12 && fabs(g1 - g0) > 1e-8 * fabs(g1)) {
            g0 = g1;
            ++it;
            const T ex = exp(-p.p_w * (a_n + s23 * g0));
            xr = sigtrn - 2.0 * mu * g0 - s23 * (p.p_y0 + dy * (1.0 - ex));
            const T xg = -2.0 * mu - 2.0 / 3.0 * dy * p.p_w * ex;
            g1 = g0 - xr / xg;
            if (it > 100) {
                status = 1;
                break;
            }
        }
    }
    for (int i = 0; i < 6; ++i) {
        const double I = i < 3 ? 1.0 : 0.0;
        h.eps_n[i] = h.eps_n[i] + g1 * xn[i];
        sigma[i] = sigma[i] + ((p.p_ka * tr_eps * I + del_sigtr[i]) - 2.0 * mu * g1 * xn[i]);
    }
    h.alpha[0] = h.alpha[0] + s23 * g1;
    return status;
}
"""

VON_MISES_SWIFT_AD = r"""
// von Mises plasticity with Swift hardening, sigma_y = K (eps0 + alpha)^m: radial return, Newton on the plastic multiplier g
// of r(g) = |s_tr| - 2 mu g - sqrt(2/3) sigma_y(alpha_n + sqrt(2/3) g).  Converged when |r| <= 1e-10 sigma_y, after which one
// more Newton step is taken (its derivative is then the implicit one to rounding); more than max_iter steps: status 1.
template <class T>
__device__ int fcamd_user_stress(const UserParams& p, double t, double del_t, const T (&eps)[6], T (&sigma)[6], UserHistoryT<T>& h) {
    const double mu = p.p_mu, s23 = sqrt(2.0 / 3.0);
    const T tr_eps = (eps[0] + eps[1]) + eps[2];
    const T tr_sig = (sigma[0] + sigma[1]) + sigma[2];
    T del_sigtr[6], sigtr[6];
    for (int i = 0; i < 6; ++i) {
        const double I = i < 3 ? 1.0 : 0.0;
        del_sigtr[i] = 2.0 * mu * (eps[i] - tr_eps * I / 3.0);
        sigtr[i] = (sigma[i] - tr_sig * I / 3.0) + del_sigtr[i];
    }
    T sq = sigtr[0] * sigtr[0];
    for (int i = 1; i < 6; ++i) sq = sq + sigtr[i] * sigtr[i];
    const T sigtrn = sqrt(sq);
    const T a0 = p.eps0 + h.alpha[0];
    const T phitr = sigtrn - s23 * (p.K * pow(a0, p.m));
    T xn[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    T g = 0.0;
    int status = 0;
    if (phitr > 0.0) {
        for (int i = 0; i < 6; ++i) xn[i] = sigtr[i] / sigtrn;
        for (int it = 0;; ++it) {
            const T a = a0 + s23 * g;
            const T sy = p.K * pow(a, p.m);
            const T r = (sigtrn - 2.0 * mu * g) - s23 * sy;
            const bool done = fabs(r) <= 1e-10 * sy;
            if (!done && it >= p.max_iter) {
                status = 1;
                break;
            }
            const T dr = -2.0 * mu - 2.0 / 3.0 * p.m * (sy / a);
            g = g - r / dr;
            if (done) break;
        }
    }
    for (int i = 0; i < 6; ++i) {
        const double I = i < 3 ? 1.0 : 0.0;
        h.eps_n[i] = h.eps_n[i] + g * xn[i];
        sigma[i] = sigma[i] + ((p.p_ka * tr_eps * I + del_sigtr[i]) - 2.0 * mu * g * xn[i]);
    }
    h.alpha[0] = h.alpha[0] + s23 * g;
    return status;
}
"""

# The deviatoric trial stress of the three implicit laws, its norm and the elastic predictor: the expressions of the _AD sources.
_IMPLICIT_TRIAL = r"""
template <class T>
__device__ __forceinline__ void trial_state(double ka, double mu, const T (&eps)[6], const double (&sigma_n)[6], T& tr_eps,
                                            T (&del_sigtr)[6], T (&sigtr)[6], T& sigtrn) {
    tr_eps = (eps[0] + eps[1]) + eps[2];
    const double tr_sig = (sigma_n[0] + sigma_n[1]) + sigma_n[2];
    for (int i = 0; i < 6; ++i) {
        const double I = i < 3 ? 1.0 : 0.0;
        del_sigtr[i] = 2.0 * mu * (eps[i] - tr_eps * I / 3.0);
        sigtr[i] = (sigma_n[i] - tr_sig * I / 3.0) + del_sigtr[i];
    }
    T sq = sigtr[0] * sigtr[0];
    for (int i = 1; i < 6; ++i) sq = sq + sigtr[i] * sigtr[i];
    sigtrn = sqrt(sq);
}
"""

# Radial return in one unknown g, the plastic multiplier: what start, residual and update share.  YIELD(a) is the yield stress at
# the accumulated plastic strain a.
_RADIAL_RETURN = r"""
// r(g) = (|s_tr| - 2 mu g - sqrt(2/3) sigma_y(alpha_n + sqrt(2/3) g)) / sigma_y; elastic (code 0, g = 0) while r(0) <= 0
template <class T>
__device__ int fcamd_user_start(const UserParams& p, double t, double del_t, const T (&eps)[6], const double (&sigma_n)[6],
                                const UserHistoryT<double>& h_n, T (&x)[1]) {
    T tr_eps, del_sigtr[6], sigtr[6], sigtrn;
    trial_state(p.p_ka, p.p_mu, eps, sigma_n, tr_eps, del_sigtr, sigtr, sigtrn);
    x[0] = 0.0;
    return sigtrn - sqrt(2.0 / 3.0) * yield_stress(p, h_n.alpha[0]) > 0.0 ? 1 : 0;
}

template <class T>
__device__ void fcamd_user_residual(const UserParams& p, double t, double del_t, const T (&eps)[6], const double (&sigma_n)[6],
                                    const UserHistoryT<double>& h_n, const T (&x)[1], T (&r)[1]) {
    const double s23 = sqrt(2.0 / 3.0);
    T tr_eps, del_sigtr[6], sigtr[6], sigtrn;
    trial_state(p.p_ka, p.p_mu, eps, sigma_n, tr_eps, del_sigtr, sigtr, sigtrn);
    const T sy = yield_stress(p, h_n.alpha[0] + s23 * x[0]);
    r[0] = ((sigtrn - 2.0 * p.p_mu * x[0]) - s23 * sy) / sy;
}

template <class T>
__device__ void fcamd_user_update(const UserParams& p, double t, double del_t, const T (&eps)[6], const T (&x)[1], T (&sigma)[6],
                                  UserHistoryT<T>& h) {
    const double s23 = sqrt(2.0 / 3.0);
    double sigma_n[6];
    for (int i = 0; i < 6; ++i) sigma_n[i] = fcamd_value(sigma[i]);
    T tr_eps, del_sigtr[6], sigtr[6], sigtrn;
    trial_state(p.p_ka, p.p_mu, eps, sigma_n, tr_eps, del_sigtr, sigtr, sigtrn);
    const T g = x[0];
    for (int i = 0; i < 6; ++i) {
        const double I = i < 3 ? 1.0 : 0.0;
        T gn = 0.0;  // g times the flow direction; a zero trial deviator has none
        if (sigtrn > 0.0) gn = g * (sigtr[i] / sigtrn);
        h.eps_n[i] = h.eps_n[i] + gn;
        sigma[i] = sigma[i] + ((p.p_ka * tr_eps * I + del_sigtr[i]) - 2.0 * p.p_mu * gn);
    }
    h.alpha[0] = h.alpha[0] + s23 * g;
}
"""

VON_MISES_3D_IMPLICIT = _IMPLICIT_TRIAL + r"""
// VonMises3D: sigma_y = y0 + (y00 - y0) (1 - exp(-w alpha))
template <class T>
__device__ __forceinline__ T yield_stress(const UserParams& p, const T& a) {
    return p.p_y0 + (p.p_y00 - p.p_y0) * (1.0 - exp(-p.p_w * a));
}
""" + _RADIAL_RETURN

VON_MISES_SWIFT_IMPLICIT = _IMPLICIT_TRIAL + r"""
// Swift hardening: sigma_y = K (eps0 + alpha)^m
template <class T>
__device__ __forceinline__ T yield_stress(const UserParams& p, const T& a) {
    return p.K * pow(p.eps0 + a, p.m);
}
""" + _RADIAL_RETURN

VON_MISES_SWIFT_GENERAL = _IMPLICIT_TRIAL + r"""
// von Mises plasticity with Swift hardening as a general return mapping: x = (d eps_p[6], d alpha, d gamma) and
//   r[0..5] = d eps_p - d gamma s / |s|                       flow rule
//   r[6]    = d alpha - sqrt(2/3) d gamma                     hardening rule
//   r[7]    = (|s| - sqrt(2/3) sigma_y(alpha_n + d alpha)) / (2 mu)     yield condition
// with s the deviator of sigma_n + C : (eps - d eps_p).  Nothing is reduced by hand; the 8 x 8 Jacobian is the engine's.
template <class T>
__device__ __forceinline__ T yield_stress(const UserParams& p, const T& a) {
    return p.K * pow(p.eps0 + a, p.m);
}

template <class T>
__device__ int fcamd_user_start(const UserParams& p, double t, double del_t, const T (&eps)[6], const double (&sigma_n)[6],
                                const UserHistoryT<double>& h_n, T (&x)[8]) {
    T tr_eps, del_sigtr[6], sigtr[6], sigtrn;
    trial_state(p.p_ka, p.p_mu, eps, sigma_n, tr_eps, del_sigtr, sigtr, sigtrn);
    for (int i = 0; i < 8; ++i) x[i] = 0.0;
    return sigtrn - sqrt(2.0 / 3.0) * yield_stress(p, h_n.alpha[0]) > 0.0 ? 1 : 0;
}

template <class T>
__device__ void fcamd_user_residual(const UserParams& p, double t, double del_t, const T (&eps)[6], const double (&sigma_n)[6],
                                    const UserHistoryT<double>& h_n, const T (&x)[8], T (&r)[8]) {
    const double s23 = sqrt(2.0 / 3.0);
    T tr_eps, del_sigtr[6], sigtr[6], sigtrn;
    trial_state(p.p_ka, p.p_mu, eps, sigma_n, tr_eps, del_sigtr, sigtr, sigtrn);
    const T tr_p = (x[0] + x[1]) + x[2];
    T s[6];
    for (int i = 0; i < 6; ++i) s[i] = sigtr[i] - 2.0 * p.p_mu * (x[i] - tr_p * (i < 3 ? 1.0 : 0.0) / 3.0);
    T sq = s[0] * s[0];
    for (int i = 1; i < 6; ++i) sq = sq + s[i] * s[i];
    const T sn = sqrt(sq);
    for (int i = 0; i < 6; ++i) r[i] = x[i] - x[7] * (s[i] / sn);
    r[6] = x[6] - s23 * x[7];
    r[7] = (sn - s23 * yield_stress(p, h_n.alpha[0] + x[6])) / (2.0 * p.p_mu);
}

template <class T>
__device__ void fcamd_user_update(const UserParams& p, double t, double del_t, const T (&eps)[6], const T (&x)[8], T (&sigma)[6],
                                  UserHistoryT<T>& h) {
    const T tr_eps = (eps[0] + eps[1]) + eps[2];
    for (int i = 0; i < 6; ++i) {
        const double I = i < 3 ? 1.0 : 0.0;
        const T del_sigtr = 2.0 * p.p_mu * (eps[i] - tr_eps * I / 3.0);
        h.eps_n[i] = h.eps_n[i] + x[i];
        sigma[i] = sigma[i] + ((p.p_ka * tr_eps * I + del_sigtr) - 2.0 * p.p_mu * x[i]);
    }
    h.alpha[0] = h.alpha[0] + x[6];
}
"""

FULL = StressStrainConstraint.FULL
_VM = ("p_ka", "p_mu", "p_y0", "p_y00", "p_w")
_SWIFT = ("p_ka", "p_mu", "K", "eps0", "m")


def _split(parameters, names) -> dict:
    """``{"parameters": ..., "fields": ...}`` of UserLaw for the law's parameter ``names``: a value that is a NumPy array or a tensor
    is a per-point field, the rest are the scalars they always were"""
    from .device import _is_torch

    import numpy as np

    is_field = {k: isinstance(parameters[k], np.ndarray) or _is_torch(parameters[k]) for k in names}
    return {"parameters": {k: parameters[k] for k in names if not is_field[k]},
            "fields": {k: parameters[k] for k in names if is_field[k]} or None}


def linear_elasticity(parameters) -> UserLaw:
    """``parameters``: {"E", "nu"}"""
    return UserLaw(LINEAR_ELASTICITY, history_dim=None, constraint=FULL, name="linear_elasticity", **_split(parameters, ("E", "nu")))


def spring_maxwell(parameters) -> UserLaw:
    """``parameters``: {"E0", "E1", "tau", "nu"}"""
    return UserLaw(SPRING_MAXWELL, history_dim={"strain_visco": 6, "strain": 6}, constraint=FULL, name="spring_maxwell",
                   **_split(parameters, ("E0", "E1", "tau", "nu")))


def von_mises_3d(parameters) -> UserLaw:
    """``parameters``: {"p_ka", "p_mu", "p_y0", "p_y00", "p_w"}"""
    return UserLaw(VON_MISES_3D, history_dim={"eps_n": 6, "alpha": 1}, constraint=FULL, name="von_mises_3d",
                   **_split(parameters, _VM))


def linear_elasticity_ad(parameters) -> UserLaw:
    """``parameters``: {"E", "nu"}"""
    return UserLaw(LINEAR_ELASTICITY_AD, history_dim=None, constraint=FULL, name="linear_elasticity_ad", tangent="autodiff",
                   **_split(parameters, ("E", "nu")))


def spring_maxwell_ad(parameters) -> UserLaw:
    """``parameters``: {"E0", "E1", "tau", "nu"}"""
    return UserLaw(SPRING_MAXWELL_AD, history_dim={"strain_visco": 6, "strain": 6}, constraint=FULL, name="spring_maxwell_ad",
                   tangent="autodiff", **_split(parameters, ("E0", "E1", "tau", "nu")))


def von_mises_3d_ad(parameters) -> UserLaw:
    """``parameters``: {"p_ka", "p_mu", "p_y0", "p_y00", "p_w"}"""
    return UserLaw(VON_MISES_3D_AD, history_dim={"eps_n": 6, "alpha": 1}, constraint=FULL, name="von_mises_3d_ad",
                   tangent="autodiff", **_split(parameters, _VM))


def von_mises_swift_ad(parameters) -> UserLaw:
    """``parameters``: {"p_ka", "p_mu", "K", "eps0", "m"} and optionally "max_iter" (Newton steps; default 50)"""
    p = _split(parameters, _SWIFT)
    p["parameters"]["max_iter"] = float(parameters.get("max_iter", 50))  # a step count: uniform
    return UserLaw(VON_MISES_SWIFT_AD, history_dim={"eps_n": 6, "alpha": 1}, constraint=FULL, name="von_mises_swift_ad",
                   tangent="autodiff", **p)


def von_mises_3d_implicit(parameters, newton=None) -> UserLaw:
    """``parameters``: {"p_ka", "p_mu", "p_y0", "p_y00", "p_w"}; ``newton``: {"max_iter", "tol"} (default 50, 1e-12: the residual
    is relative to the yield stress)"""
    return UserLaw(VON_MISES_3D_IMPLICIT, history_dim={"eps_n": 6, "alpha": 1}, constraint=FULL, name="von_mises_3d_implicit",
                   tangent="implicit", unknowns=1, newton={"max_iter": 50, "tol": 1e-12} if newton is None else newton,
                   **_split(parameters, _VM))


def von_mises_swift_implicit(parameters, newton=None) -> UserLaw:
    """``parameters``: {"p_ka", "p_mu", "K", "eps0", "m"}; ``newton``: {"max_iter", "tol"} (default 50, 1e-13)"""
    return UserLaw(VON_MISES_SWIFT_IMPLICIT, history_dim={"eps_n": 6, "alpha": 1}, constraint=FULL, name="von_mises_swift_implicit",
                   tangent="implicit", unknowns=1, newton={"max_iter": 50, "tol": 1e-13} if newton is None else newton,
                   **_split(parameters, _SWIFT))


def von_mises_swift_general(parameters, newton=None) -> UserLaw:
    """``parameters``: {"p_ka", "p_mu", "K", "eps0", "m"}; ``newton``: {"max_iter", "tol"} (default 50, 1e-13)"""
    return UserLaw(VON_MISES_SWIFT_GENERAL, history_dim={"eps_n": 6, "alpha": 1}, constraint=FULL, name="von_mises_swift_general",
                   tangent="implicit", unknowns=8, newton={"max_iter": 50, "tol": 1e-13} if newton is None else newton,
                   **_split(parameters, _SWIFT))
