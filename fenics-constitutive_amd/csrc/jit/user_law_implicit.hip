// Kernel template of user laws in implicit mode (userlaw.py, tangent="implicit"): the point step around the user's
// fcamd_user_start / fcamd_user_residual / fcamd_user_update (user_law_implicit.h), inside the tile code of user_law_tile.h.
// Compiled behind the generated definitions that user_law_tile.h lists, the template UserHistoryT<T> and
//   FCAMD_USER_UNKNOWNS   N, the local unknowns
//   FCAMD_USER_IM_KJ      directions per Jacobian pass: J = dr / dx from ceil(N / KJ) evaluations of residual<Dual<KJ>>
//   FCAMD_USER_IM_KT      0: the stress-only kernel; K > 0: the tangent kernel, ceil(6 / K) passes of Dual<K> over the strain columns
//   FCAMD_USER_IM_SLOT    params[SLOT] = max_iter, params[SLOT + 1] = tol (behind the law's own parameters)
//
// Per tile: start<double>; the Newton loop while a ballot of the lanes still iterating is non-zero (all of them have taken the
// same number of steps, so the step count is uniform); update<double> and the stores of stress and history.  The tangent kernel
// then, per pass: J again at the final x, R = dr / deps from residual<Dual<KT>> with eps seeded, X = -J^-1 R for the lanes that
// solved, the partials of start<Dual<KT>> for the others, and update<Dual<KT>> on (eps, x) carrying them.  One pass (K = 6)
// writes the 36 partials like the explicit template's tangent, several passes write their own columns and the pass loop is
// rolled, as in user_law_ad.hip.  A tile without a lane that solved skips J and the solve (uniform branch).
#pragma once
#include "user_law_tile.h"

namespace fcamd_user {

constexpr int kN = FCAMD_USER_UNKNOWNS;
constexpr int kKJ = FCAMD_USER_IM_KJ;
constexpr int kKT = FCAMD_USER_IM_KT;
constexpr int kJPasses = (kN + kKJ - 1) / kKJ;
static_assert(kN >= 1 && kKJ >= 1 && kKJ <= kN && kKT >= 0 && kKT <= 6, "implicit mode: unknowns or directions out of range");
static_assert(FCAMD_USER_IM_SLOT + 2 <= kMaxParams, "implicit mode: no room for max_iter and tol behind the parameters");

// the committed history as constants of type T
template <class T>
__device__ __forceinline__ void history_as(const UserHistoryT<double>& h, UserHistoryT<T>& th) {
#define FCAMD_X(k, name, dim) \
    _Pragma("unroll") for (int i = 0; i < (dim); ++i) th.name[i] = T(h.name[i]);
    FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
}

// r and J = dr / dx at x: pass c seeds the unknowns [c KJ, c KJ + KJ).  The passes are unrolled: J stays in registers.
__device__ __forceinline__ void user_jacobian(const UserParams& p, double t, double del_t, const double (&e)[6], const double (&s)[6],
                                              const UserHistoryT<double>& h, const double (&x)[kN], double (&r)[kN],
                                              double (&J)[kN * kN]) {
    using TJ = Dual<kKJ>;
    TJ de[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) de[j] = TJ(e[j]);
#pragma unroll
    for (int c = 0; c < kJPasses; ++c) {
        TJ dx[kN], dr[kN];
#pragma unroll
        for (int j = 0; j < kN; ++j) {
            dx[j] = TJ(x[j]);
#pragma unroll
            for (int k = 0; k < kKJ; ++k) dx[j].d[k] = j == c * kKJ + k ? 1.0 : 0.0;
        }
        fcamd_user_residual<TJ>(p, t, del_t, de, s, h, dx, dr);
#pragma unroll
        for (int i = 0; i < kN; ++i) {
            if (c == 0) r[i] = dr[i].v;
#pragma unroll
            for (int k = 0; k < kKJ; ++k)
                if (c * kKJ + k < kN) J[kN * i + c * kKJ + k] = dr[i].d[k];
        }
    }
}

// columns [c K, c K + K) of the tile's tangent from the partials of the lanes' stress (several passes: no 6x6 D is kept):
// through the wave's LDS region, then one 8-byte store per entry, consecutive lanes on consecutive entries of a row segment.
// The store of user_law_ad.hip, which an implicit program does not include (its include closure keys the autodiff code objects).
template <bool FULL, int K>
__device__ __forceinline__ void user_columns_out(const UserArgs& a, const Dual<K> (&ds)[6], int c, double* region, long long p0,
                                                 int npts, int lane) {
    constexpr int kW = 6 * K;  // doubles per point and pass (<= kUserWide)
    double col[kW];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int k = 0; k < K; ++k) col[i * K + k] = ds[i].d[k];
    lds_put_point<kW>(region, lane, col);
    wave_sync();
    double* dst = a.tangent + p0 * 36 + c * K;
#pragma unroll
    for (int m = 0; m < kW; ++m) {
        const int q = m * kWave + lane;  // entry q of the region: point q / kW, row (q % kW) / K, column (q % K)
        const int pt = q / kW, rem = q - pt * kW, i = rem / K, k = rem - i * K;
        if (FULL || pt < npts) dst[pt * 36 + 6 * i + k] = region[q];
    }
    wave_sync();
}

// the consistent tangent of the tile, KT strain columns per pass (the tangent kernel; the values are stored already)
template <bool FULL, bool NT, int KT>
__device__ __forceinline__ void user_tangent(const UserArgs& a, const UserParams& p, double* region, long long p0, int npts, int lane,
                                             const double (&e)[6], const double (&s)[6], const UserHistoryT<double>& h,
                                             const double (&x)[kN], bool solved) {
    using T = Dual<KT>;
    constexpr int kPasses = (6 + KT - 1) / KT;
    const bool any_solved = __builtin_amdgcn_ballot_w64(solved) != 0ull;
    double D[kPasses == 1 ? 36 : 1];
#pragma nounroll
    for (int c = 0; c < kPasses; ++c) {
        T de[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            de[j] = T(e[j]);
#pragma unroll
            for (int k = 0; k < KT; ++k) de[j].d[k] = j == c * KT + k ? 1.0 : 0.0;
        }
        double X[kN * KT];
        if (any_solved) {
            double r[kN], J[kN * kN];
            user_jacobian(p, a.t, a.del_t, e, s, h, x, r, J);
            T cx[kN], dr[kN];
#pragma unroll
            for (int i = 0; i < kN; ++i) cx[i] = T(x[i]);
            fcamd_user_residual<T>(p, a.t, a.del_t, de, s, h, cx, dr);
#pragma unroll
            for (int i = 0; i < kN; ++i)
#pragma unroll
                for (int k = 0; k < KT; ++k) X[KT * i + k] = -dr[i].d[k];
            dense_solve<kN, KT>(J, X);
        } else {
#pragma unroll
            for (int i = 0; i < kN * KT; ++i) X[i] = 0.0;
        }
        // the lanes that did not solve: x (the same bits) and its partials from start
        T dx[kN];
        fcamd_user_start<T>(p, a.t, a.del_t, de, s, h, dx);
#pragma unroll
        for (int i = 0; i < kN; ++i) {
            dx[i].v = x[i];
#pragma unroll
            for (int k = 0; k < KT; ++k) dx[i].d[k] = solved ? X[KT * i + k] : dx[i].d[k];
        }
        T ds[6];
        UserHistoryT<T> dh;
#pragma unroll
        for (int j = 0; j < 6; ++j) ds[j] = T(s[j]);
        history_as<T>(h, dh);
        fcamd_user_update<T>(p, a.t, a.del_t, de, dx, ds, dh);
        if constexpr (kPasses == 1) {
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int k = 0; k < 6; ++k) D[6 * i + k] = ds[i].d[k];
        } else {
            user_columns_out<FULL>(a, ds, c, region, p0, npts, lane);
        }
    }
    if constexpr (kPasses == 1) user_out<36, FULL, NT>(D, region, lane, a.tangent + p0 * 36, npts * 36);
}

// start<double> and the Newton loop of one tile: x on return.  `live`: the lanes whose points count (the others never iterate).
// `solved`: the lanes whose x came out of the loop; returns whether the lane's point did not converge.  Wave-collective: the loop
// runs while a ballot of the lanes still iterating is non-zero.
__device__ __forceinline__ bool user_newton(const UserParams& p, double t, double del_t, const double (&e)[6], const double (&s)[6],
                                            const UserHistoryT<double>& h, bool live, int max_iter, double tol, double (&x)[kN],
                                            bool& solved) {
    const int code = fcamd_user_start<double>(p, t, del_t, e, s, h, x);
    solved = live && code == 1;  // the lanes whose x comes out of the Newton loop
    bool failed = code != 0 && code != 1;
    bool active = solved;
    for (int it = 0; __builtin_amdgcn_ballot_w64(active) != 0ull; ++it) {
        double r[kN], J[kN * kN];
        user_jacobian(p, t, del_t, e, s, h, x, r, J);
        bool conv = true;
#pragma unroll
        for (int i = 0; i < kN; ++i) conv = conv && __builtin_fabs(r[i]) <= tol;  // false for a NaN
        bool step = active && !conv && it < max_iter;
        failed = failed || (active && !conv && !step);
        if (__builtin_amdgcn_ballot_w64(step) != 0ull) {  // uniform: the last check of a tile solves nothing
            const bool ok = dense_solve<kN, 1>(J, r);
            failed = failed || (step && !ok);
            step = step && ok;
#pragma unroll
            for (int i = 0; i < kN; ++i) x[i] = step ? x[i] - r[i] : x[i];  // a lane that has finished keeps its x
        }
        active = step;
    }
    return failed;
}

template <bool FULL, bool NT>
__device__ __forceinline__ unsigned long long user_tile(const UserArgs& a, const UserParams& p, double* region, long long p0,
                                                        int npts, int lane) {
    double g[9], s[6], e[6];
    UserHistoryT<double> h;
    user_tile_in<FULL, NT>(a, region, p0, npts, lane, g, s, e, h);
    const bool live = FULL || lane < npts;
    const int max_iter = (int)a.params[FCAMD_USER_IM_SLOT];
    const double tol = a.params[FCAMD_USER_IM_SLOT + 1];

    double x[kN];
    bool solved;
    const bool failed = user_newton(p, a.t, a.del_t, e, s, h, live, max_iter, tol, x, solved);
    const unsigned long long bad = __builtin_amdgcn_ballot_w64(live && failed);

    {
        double sv[6];
        UserHistoryT<double> hv = h;
#pragma unroll
        for (int i = 0; i < 6; ++i) sv[i] = s[i];
        fcamd_user_update<double>(p, a.t, a.del_t, e, x, sv, hv);
        transpose_out<6, FULL, NT>(sv, region, lane, a.stress_out + p0 * 6, npts * 6);
#define FCAMD_X(k, name, dim) user_out<dim, FULL, NT>(hv.name, region, lane, a.h_out[k] + p0 * (dim), npts * (dim));
        FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
    }

    if constexpr (kKT > 0) user_tangent<FULL, NT, kKT>(a, p, region, p0, npts, lane, e, s, h, x, solved);
    return (unsigned long long)__popcll(bad);
}

}  // namespace fcamd_user
