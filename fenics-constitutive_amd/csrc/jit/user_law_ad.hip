// Kernel template of user laws in autodiff mode (userlaw.py, tangent="autodiff"): the point step around the user's
// fcamd_user_stress<T> (user_law_ad.h), inside the tile code of user_law_tile.h.  Compiled behind the generated definitions that
// user_law_tile.h lists, the template UserHistoryT<T> (the committed history is read as UserHistoryT<double>) and
//   FCAMD_USER_AD_K     0: the stress-only kernel (T = double, one pass); K > 0: the tangent kernel, ceil(6 / K) passes of
//                       T = Dual<K>, pass c seeding the strain columns [c K, c K + K)
//
// The tangent kernel writes the values of its first pass out (stress, history, return code) before the later passes, so they
// are dead there; the later passes keep only the partials of sigma.  With K = 6 (one pass) the 36 partials are written like
// the explicit template's tangent.  With K < 6 the pass loop is rolled (its index uniform, so the passes do not overlap) and
// every pass writes its own 6 K columns (user_columns_out): no 6x6 D is kept in registers.  Define FCAMD_USER_AD_DEBUG to check
// that every pass computes the first pass's stress and return code; a point where they differ counts as not converged.
#pragma once
#include "user_law_tile.h"

namespace fcamd_user {

constexpr int kK = FCAMD_USER_AD_K;
constexpr int kPasses = kK > 0 ? (6 + kK - 1) / kK : 1;

// the values of a history / stress array of Duals (or doubles)
template <int NC, class T>
__device__ __forceinline__ void values_of(const T (&x)[NC], double (&v)[NC]) {
#pragma unroll
    for (int i = 0; i < NC; ++i) v[i] = fcamd_value(x[i]);
}

// stress and history of one lane -> the tile's output arrays
template <bool FULL, bool NT, class T>
__device__ __forceinline__ void user_values_out(const UserArgs& a, const T (&s)[6], const UserHistoryT<T>& h, double* region,
                                                long long p0, int npts, int lane) {
    double sv[6];
    values_of<6>(s, sv);
    transpose_out<6, FULL, NT>(sv, region, lane, a.stress_out + p0 * 6, npts * 6);
#define FCAMD_X(k, name, dim)                                                                  \
    {                                                                                          \
        double hv[dim];                                                                        \
        values_of<dim>(h.name, hv);                                                            \
        user_out<dim, FULL, NT>(hv, region, lane, a.h_out[k] + p0 * (dim), npts * (dim));      \
    }
    FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
}

// columns [c K, c K + K) of the tile's tangent, from the partials of the lanes' stress (K < 6: the tangent kernel of several
// passes, which keeps no D): through the wave's LDS region, then one 8-byte store per entry, consecutive lanes on consecutive
// entries of a point's row segment.  Plain stores: the passes of a tile fill the same cache lines one after another.
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

template <bool FULL, bool NT>
__device__ __forceinline__ unsigned long long user_tile(const UserArgs& a, const UserParams& p, double* region, long long p0,
                                                        int npts, int lane) {
    double g[9], s[6], e[6];
    UserHistoryT<double> h;
    user_tile_in<FULL, NT>(a, region, p0, npts, lane, g, s, e, h);
    const bool live = FULL || lane < npts;
    if constexpr (kK == 0) {
        const int rc = fcamd_user_stress<double>(p, a.t, a.del_t, e, s, h);
        const unsigned long long bad = __builtin_amdgcn_ballot_w64(live && rc != 0);
        user_values_out<FULL, NT>(a, s, h, region, p0, npts, lane);
        return (unsigned long long)__popcll(bad);
    } else {
        using T = Dual<kK>;
        double D[kPasses == 1 ? 36 : 1];
        int rc = 0;
#ifdef FCAMD_USER_AD_DEBUG
        double s0[6];
#endif
#pragma nounroll
        for (int c = 0; c < kPasses; ++c) {
            T de[6], ds[6];
            UserHistoryT<T> dh;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                de[j] = T(e[j]);
#pragma unroll
                for (int k = 0; k < kK; ++k) de[j].d[k] = j == c * kK + k ? 1.0 : 0.0;
                ds[j] = T(s[j]);
            }
#define FCAMD_X(k, name, dim)          \
    _Pragma("unroll") for (int i = 0; i < (dim); ++i) dh.name[i] = T(h.name[i]);
            FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
            const int r = fcamd_user_stress<T>(p, a.t, a.del_t, de, ds, dh);
            if constexpr (kPasses == 1) {
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int k = 0; k < 6; ++k) D[6 * i + k] = ds[i].d[k];
            } else {
                user_columns_out<FULL>(a, ds, c, region, p0, npts, lane);
            }
            if (c == 0) {
                rc = r;
                user_values_out<FULL, NT>(a, ds, dh, region, p0, npts, lane);
#ifdef FCAMD_USER_AD_DEBUG
                values_of<6>(ds, s0);
#endif
            }
#ifdef FCAMD_USER_AD_DEBUG
            else {
                bool same = r == rc;
#pragma unroll
                for (int i = 0; i < 6; ++i) same = same && fcamd_value(ds[i]) == s0[i];
                if (!same) rc = rc != 0 ? rc : -1;
            }
#endif
        }
        const unsigned long long bad = __builtin_amdgcn_ballot_w64(live && rc != 0);
        if constexpr (kPasses == 1) user_out<36, FULL, NT>(D, region, lane, a.tangent + p0 * 36, npts * 36);
        return (unsigned long long)__popcll(bad);
    }
}

}  // namespace fcamd_user
