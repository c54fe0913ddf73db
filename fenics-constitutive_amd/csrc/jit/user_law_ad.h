// The autodiff contract of user-defined laws (UserLaw(..., tangent="autodiff"), userlaw.py).  The user writes the stress and
// history update ONCE, as a function template over the scalar type; the kernel template user_law_ad.hip instantiates it with
// T = double for stress-only launches and with T = fcamd::Dual<K> (one value, K partials) for launches that also write the
// tangent, seeding K columns of the strain increment per pass:
//
//   struct UserParams { double E, nu; };                                        // generated, as in user_law_api.h
//   template <class T> struct UserHistoryT { T eps_n[6]; T alpha[1]; };         // generated: one array per history field
//
//   template <class T>
//   __device__ int fcamd_user_stress(const UserParams& p, double t, double del_t,
//                                    const T (&eps)[6],      // Mandel strain increment (bit-identical to user_law_api.h's eps)
//                                    T (&sigma)[6],          // in: committed stress, out: new stress
//                                    UserHistoryT<T>& h);    // in: committed history, out: trial history
//   // return 0 = converged; any other value counts the point as not converged
//
// The tangent is D[6 i + j] = d sigma_i / d eps_j (row-major, Mandel), the derivative of the code as written: a Newton loop is
// differentiated through its iterations.  t, del_t and the parameters are constants; the displacement gradient is not passed.
//
// Dual<K> rules:
//  * the value part of every operation is the same IEEE operation as the double code (the program is compiled with
//    -ffp-contract=off): stress, history and return code of a tangent launch are bit-identical to those of T = double;
//  * comparisons compare values only; fcamd_value(x) is the double of x for both T (branch conditions, loop tests);
//  * sqrt: a partial that is zero stays zero, also at a zero value -- a zero deviatoric trial stress gives the finite elastic
//    tangent instead of 0 / 0;
//  * write `T x = 0.0;` for a local that may become a Dual, `double` for constants.
#pragma once
#include "user_law_api.h"

namespace fcamd {

template <int K>
struct Dual {
    double v;
    double d[K];

    __device__ __forceinline__ Dual() = default;
    // a constant: zero partials
    __device__ __forceinline__ Dual(double x) : v(x) {
#pragma unroll
        for (int k = 0; k < K; ++k) d[k] = 0.0;
    }

    // --- arithmetic: Dual x Dual, Dual x double, double x Dual ---------------------------------------------------------------
    friend __device__ __forceinline__ Dual operator+(const Dual& a, const Dual& b) {
        Dual r;
        r.v = a.v + b.v;
#pragma unroll
        for (int k = 0; k < K; ++k) r.d[k] = a.d[k] + b.d[k];
        return r;
    }
    friend __device__ __forceinline__ Dual operator+(const Dual& a, double b) {
        Dual r = a;
        r.v = a.v + b;
        return r;
    }
    friend __device__ __forceinline__ Dual operator+(double a, const Dual& b) {
        Dual r = b;
        r.v = a + b.v;
        return r;
    }
    friend __device__ __forceinline__ Dual operator-(const Dual& a) {
        Dual r;
        r.v = -a.v;
#pragma unroll
        for (int k = 0; k < K; ++k) r.d[k] = -a.d[k];
        return r;
    }
    friend __device__ __forceinline__ Dual operator-(const Dual& a, const Dual& b) {
        Dual r;
        r.v = a.v - b.v;
#pragma unroll
        for (int k = 0; k < K; ++k) r.d[k] = a.d[k] - b.d[k];
        return r;
    }
    friend __device__ __forceinline__ Dual operator-(const Dual& a, double b) {
        Dual r = a;
        r.v = a.v - b;
        return r;
    }
    friend __device__ __forceinline__ Dual operator-(double a, const Dual& b) {
        Dual r;
        r.v = a - b.v;
#pragma unroll
        for (int k = 0; k < K; ++k) r.d[k] = -b.d[k];
        return r;
    }
    friend __device__ __forceinline__ Dual operator*(const Dual& a, const Dual& b) {
        Dual r;
        r.v = a.v * b.v;
#pragma unroll
        for (int k = 0; k < K; ++k) r.d[k] = __builtin_fma(a.d[k], b.v, a.v * b.d[k]);
        return r;
    }
    friend __device__ __forceinline__ Dual operator*(const Dual& a, double b) {
        Dual r;
        r.v = a.v * b;
#pragma unroll
        for (int k = 0; k < K; ++k) r.d[k] = a.d[k] * b;
        return r;
    }
    friend __device__ __forceinline__ Dual operator*(double a, const Dual& b) {
        Dual r;
        r.v = a * b.v;
#pragma unroll
        for (int k = 0; k < K; ++k) r.d[k] = a * b.d[k];
        return r;
    }
    friend __device__ __forceinline__ Dual operator/(const Dual& a, const Dual& b) {
        Dual r;
        r.v = a.v / b.v;
        const double inv = 1.0 / b.v;
#pragma unroll
        for (int k = 0; k < K; ++k) r.d[k] = (a.d[k] - r.v * b.d[k]) * inv;
        return r;
    }
    friend __device__ __forceinline__ Dual operator/(const Dual& a, double b) {
        Dual r;
        r.v = a.v / b;
#pragma unroll
        for (int k = 0; k < K; ++k) r.d[k] = a.d[k] / b;
        return r;
    }
    friend __device__ __forceinline__ Dual operator/(double a, const Dual& b) {
        Dual r;
        r.v = a / b.v;
        const double s = -r.v / b.v;
#pragma unroll
        for (int k = 0; k < K; ++k) r.d[k] = s * b.d[k];
        return r;
    }
    template <class U>
    __device__ __forceinline__ Dual& operator+=(const U& b) { return *this = *this + b; }
    template <class U>
    __device__ __forceinline__ Dual& operator-=(const U& b) { return *this = *this - b; }
    template <class U>
    __device__ __forceinline__ Dual& operator*=(const U& b) { return *this = *this * b; }
    template <class U>
    __device__ __forceinline__ Dual& operator/=(const U& b) { return *this = *this / b; }

    // --- comparisons: values only ----------------------------------------------------------------------------------------
#define FCAMD_DUAL_CMP(op)                                                                                  \
    friend __device__ __forceinline__ bool operator op(const Dual& a, const Dual& b) { return a.v op b.v; } \
    friend __device__ __forceinline__ bool operator op(const Dual& a, double b) { return a.v op b; }        \
    friend __device__ __forceinline__ bool operator op(double a, const Dual& b) { return a op b.v; }
    FCAMD_DUAL_CMP(<)
    FCAMD_DUAL_CMP(<=)
    FCAMD_DUAL_CMP(>)
    FCAMD_DUAL_CMP(>=)
    FCAMD_DUAL_CMP(==)
    FCAMD_DUAL_CMP(!=)
#undef FCAMD_DUAL_CMP
};

__device__ __forceinline__ double fcamd_value(double x) { return x; }
template <int K>
__device__ __forceinline__ double fcamd_value(const Dual<K>& x) { return x.v; }

// f(a) with value fa and derivative dfa (chain rule)
template <int K>
__device__ __forceinline__ Dual<K> dual_chain(const Dual<K>& a, double fa, double dfa) {
    Dual<K> r;
    r.v = fa;
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = dfa * a.d[k];
    return r;
}

// --- functions (found by argument-dependent lookup; the value is the global double function's) ------------------------------
template <int K>
__device__ __forceinline__ Dual<K> sqrt(const Dual<K>& a) {
    Dual<K> r;
    r.v = ::sqrt(a.v);
    const double s = 0.5 / r.v;
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = a.d[k] == 0.0 ? 0.0 : s * a.d[k];  // a zero partial stays zero (also at sqrt(0))
    return r;
}
template <int K>
__device__ __forceinline__ Dual<K> exp(const Dual<K>& a) {
    const double e = ::exp(a.v);
    return dual_chain(a, e, e);
}
template <int K>
__device__ __forceinline__ Dual<K> log(const Dual<K>& a) {
    return dual_chain(a, ::log(a.v), 1.0 / a.v);
}
// d/da a^b = b a^b / a: one pow; at a = 0 the limit (0 for b > 1 or b = 0, 1 for b = 1, inf for 0 < b < 1)
template <int K>
__device__ __forceinline__ Dual<K> pow(const Dual<K>& a, double b) {
    const double v = ::pow(a.v, b);
    const double at0 = (b > 1.0 || b == 0.0) ? 0.0 : (b == 1.0 ? 1.0 : __builtin_inf());
    return dual_chain(a, v, a.v != 0.0 ? b * (v / a.v) : at0);
}
template <int K>
__device__ __forceinline__ Dual<K> pow(const Dual<K>& a, const Dual<K>& b) {
    Dual<K> r = pow(a, b.v);
    const double lg = r.v * ::log(a.v);
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (b.d[k] != 0.0) r.d[k] = __builtin_fma(lg, b.d[k], r.d[k]);
    return r;
}
template <int K>
__device__ __forceinline__ Dual<K> pow(double a, const Dual<K>& b) {
    const double v = ::pow(a, b.v);
    return dual_chain(b, v, v * ::log(a));
}
template <int K>
__device__ __forceinline__ Dual<K> fabs(const Dual<K>& a) {
    return dual_chain(a, ::fabs(a.v), a.v < 0.0 ? -1.0 : 1.0);
}
template <int K>
__device__ __forceinline__ Dual<K> fmin(const Dual<K>& a, const Dual<K>& b) {
    Dual<K> r = (b.v < a.v || a.v != a.v) ? b : a;
    r.v = ::fmin(a.v, b.v);
    return r;
}
template <int K>
__device__ __forceinline__ Dual<K> fmax(const Dual<K>& a, const Dual<K>& b) {
    Dual<K> r = (b.v > a.v || a.v != a.v) ? b : a;
    r.v = ::fmax(a.v, b.v);
    return r;
}
template <int K>
__device__ __forceinline__ Dual<K> fmin(const Dual<K>& a, double b) { return fmin(a, Dual<K>(b)); }
template <int K>
__device__ __forceinline__ Dual<K> fmin(double a, const Dual<K>& b) { return fmin(Dual<K>(a), b); }
template <int K>
__device__ __forceinline__ Dual<K> fmax(const Dual<K>& a, double b) { return fmax(a, Dual<K>(b)); }
template <int K>
__device__ __forceinline__ Dual<K> fmax(double a, const Dual<K>& b) { return fmax(Dual<K>(a), b); }
template <int K>
__device__ __forceinline__ Dual<K> tanh(const Dual<K>& a) {
    const double th = ::tanh(a.v);
    return dual_chain(a, th, 1.0 - th * th);
}
template <int K>
__device__ __forceinline__ Dual<K> sinh(const Dual<K>& a) {
    return dual_chain(a, ::sinh(a.v), ::cosh(a.v));
}
template <int K>
__device__ __forceinline__ Dual<K> cosh(const Dual<K>& a) {
    return dual_chain(a, ::cosh(a.v), ::sinh(a.v));
}

// fma(a, b, c): the value is one rounding, as __builtin_fma of the values; every mix of Dual and double
template <int K>
__device__ __forceinline__ Dual<K> fma(const Dual<K>& a, const Dual<K>& b, const Dual<K>& c) {
    Dual<K> r;
    r.v = __builtin_fma(a.v, b.v, c.v);
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = __builtin_fma(a.d[k], b.v, __builtin_fma(a.v, b.d[k], c.d[k]));
    return r;
}
template <int K>
__device__ __forceinline__ Dual<K> fma(const Dual<K>& a, double b, const Dual<K>& c) {
    Dual<K> r;
    r.v = __builtin_fma(a.v, b, c.v);
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = __builtin_fma(a.d[k], b, c.d[k]);
    return r;
}
template <int K>
__device__ __forceinline__ Dual<K> fma(double a, const Dual<K>& b, const Dual<K>& c) { return fma(b, a, c); }
template <int K>
__device__ __forceinline__ Dual<K> fma(const Dual<K>& a, const Dual<K>& b, double c) { return fma(a, b, Dual<K>(c)); }
template <int K>
__device__ __forceinline__ Dual<K> fma(const Dual<K>& a, double b, double c) {
    Dual<K> r;
    r.v = __builtin_fma(a.v, b, c);
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = a.d[k] * b;
    return r;
}
template <int K>
__device__ __forceinline__ Dual<K> fma(double a, const Dual<K>& b, double c) { return fma(b, a, c); }
template <int K>
__device__ __forceinline__ Dual<K> fma(double a, double b, const Dual<K>& c) {
    Dual<K> r = c;
    r.v = __builtin_fma(a, b, c.v);
    return r;
}

// y_i = sum_k x_k * M[6 k + i] as the ascending-k FMA chain of row_times_matrix_fma (tile_io.h), for a Dual x and a constant M.
// With one unit seed in x_j the partial of y_i is exactly M[6 j + i].
template <int K>
__device__ __forceinline__ void row_times_matrix_fma(const Dual<K> (&x)[6], const double* M, Dual<K> (&y)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        Dual<K> acc = x[0] * M[i];
#pragma unroll
        for (int k = 1; k < 6; ++k) acc = fma(x[k], M[6 * k + i], acc);
        y[i] = acc;
    }
}

}  // namespace fcamd

using fcamd::Dual;
using fcamd::fcamd_value;
// the double row_times_matrix_fma of user_law_api.h and the Dual one above form one overload set
using fcamd::row_times_matrix_fma;
