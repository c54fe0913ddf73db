// The implicit contract of user-defined laws (UserLaw(..., tangent="implicit", unknowns=N), userlaw.py).  The user states the law
// as a residual r(x; eps, committed state) = 0 in N local unknowns x and as the state update from the solution; the kernel
// template user_law_implicit.hip provides the Jacobian (dual numbers, user_law_ad.h), the per-lane Newton loop, the dense solve
// below and the consistent tangent by the implicit-function theorem, dx / deps = -J^-1 dr / deps.  Nothing is differentiated
// through iterations.
//
//   struct UserParams { double p_mu, K; };                                      // generated, as in user_law_api.h
//   template <class T> struct UserHistoryT { T eps_n[6]; T alpha[1]; };         // generated: one array per history field
//   #define FCAMD_USER_UNKNOWNS 8                                               // generated: N
//
// The source defines three function templates over T (double, or fcamd::Dual<K> with the rules of user_law_ad.h).  The committed
// state is passed as doubles: it is never differentiated.
//
//   template <class T> __device__ int  fcamd_user_start(const UserParams& p, double t, double del_t, const T (&eps)[6],
//                                                       const double (&sigma_n)[6], const UserHistoryT<double>& h_n, T (&x)[N]);
//   template <class T> __device__ void fcamd_user_residual(const UserParams& p, double t, double del_t, const T (&eps)[6],
//                                                          const double (&sigma_n)[6], const UserHistoryT<double>& h_n,
//                                                          const T (&x)[N], T (&r)[N]);
//   template <class T> __device__ void fcamd_user_update(const UserParams& p, double t, double del_t, const T (&eps)[6],
//                                                        const T (&x)[N], T (&sigma)[6],      // in: committed, out: new
//                                                        UserHistoryT<T>& h);                 // in: committed, out: new
//
// start sets x and returns a code:
//   0      x is the solution as given (the elastic branch); nothing is solved, and dx / deps is what start<Dual> computes;
//   1      solve from here;
//   other  the point counts as not converged; update still runs on the x given.
// The residual is scaled by the user: a point is converged when |r_i| <= tol for every i (tol and max_iter: the law's `newton`
// dict, kernel arguments).  One lane, in this order: evaluate r; if converged, stop; else if max_iter steps have been taken, the
// point is not converged; else the Newton step x -= J^-1 r, J = dr / dx.  A pivot that is zero or not finite makes the point not
// converged; a NaN residual never passes the test.  The tangent of a point that did not converge is unspecified.  A lane that
// has finished keeps its x: no result depends on the other points of the wave.
//
// Stress, history and the count of a launch with a tangent are bit-identical to those of a launch without (-ffp-contract=off:
// the value part of every Dual operation is the double operation, and a partial does not depend on K).
#pragma once
#include "user_law_ad.h"

namespace fcamd {

// A X = B for M right-hand sides, in place (A: N x N row-major, destroyed; B: N x M row-major, X on return): LU with partial
// pivoting, eliminated and substituted in registers.  Every index is a constant of the unrolled loops and the row exchanges are
// compare-and-select, so nothing is addressed dynamically (no scratch).  False when a pivot is zero or not finite (X is then
// meaningless).  The pivots' reciprocals are formed once (one division per row).
template <int N, int M>
__device__ __forceinline__ bool dense_solve(double (&A)[N * N], double (&B)[N * M]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        // the largest |A[i][k]|, i >= k, into row k: one pass of exchanges with the rows below (a NaN never wins a comparison)
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const bool swap = __builtin_fabs(A[N * i + k]) > __builtin_fabs(A[N * k + k]);
#pragma unroll
            for (int j = k; j < N; ++j) {
                const double u = A[N * k + j], v = A[N * i + j];
                A[N * k + j] = swap ? v : u;
                A[N * i + j] = swap ? u : v;
            }
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const double u = B[M * k + m], v = B[M * i + m];
                B[M * k + m] = swap ? v : u;
                B[M * i + m] = swap ? u : v;
            }
        }
        const double piv = __builtin_fabs(A[N * k + k]);
        ok = ok && piv > 0.0 && piv < __builtin_inf();
        const double inv = 1.0 / A[N * k + k];
        A[N * k + k] = inv;
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const double f = -(A[N * i + k] * inv);
#pragma unroll
            for (int j = k + 1; j < N; ++j) A[N * i + j] = __builtin_fma(f, A[N * k + j], A[N * i + j]);
#pragma unroll
            for (int m = 0; m < M; ++m) B[M * i + m] = __builtin_fma(f, B[M * k + m], B[M * i + m]);
        }
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            double acc = B[M * i + m];
#pragma unroll
            for (int j = i + 1; j < N; ++j) acc = __builtin_fma(-A[N * i + j], B[M * j + m], acc);
            B[M * i + m] = acc * A[N * i + i];
        }
    }
    return ok;
}

}  // namespace fcamd
