// Kernel template of user laws in autodiff mode (userlaw.py, tangent="autodiff"): the memory side of user_law.hip around the
// user's fcamd_user_stress<T> (user_law_ad.h).  Read at run time and compiled with hiprtc behind the generated definitions of
// user_law.hip (FCAMD_USER_WAVES, FCAMD_USER_NHIST, FCAMD_USER_HISTORY_FIELDS, UserParams, fcamd_user_params), the template
// UserHistoryT<T> and
//   FCAMD_USER_AD_K     0: the stress-only kernel (T = double, one pass); K > 0: the tangent kernel, ceil(6 / K) passes of
//                       T = Dual<K>, pass c seeding the strain columns [c K, c K + K)
//
// The tangent kernel writes the values of its first pass out (stress, history, return code) before the later passes, so they
// are dead there; the later passes keep only the partials of sigma.  With K = 6 (one pass) the 36 partials are written like
// the explicit template's tangent.  With K < 6 the pass loop is rolled (its index uniform, so the passes do not overlap) and
// every pass writes its own 6 K columns (user_columns_out): no 6x6 D is kept in registers.  Define FCAMD_USER_AD_DEBUG to check
// that every pass computes the first pass's stress and return code; a point where they differ counts as not converged.
#pragma once

namespace fcamd_user {
using namespace fcamd;

constexpr int kMaxParams = 32;
constexpr int kNH = FCAMD_USER_NHIST > 0 ? FCAMD_USER_NHIST : 1;
constexpr int kUserWide = 18;
constexpr int kUserRegion = kWave * kUserWide;
constexpr int kUserMaxDim = 2 * kUserWide;
constexpr int kK = FCAMD_USER_AD_K;
constexpr int kPasses = kK > 0 ? (6 + kK - 1) / kK : 1;

// the only kernel parameter: the layout of user_law.hip's UserArgs (userlaw.py: _args_type)
struct UserArgs {
    const double* grad;
    const double* stress_in;
    double* stress_out;
    double* tangent;             // [36 n]; nullptr only in the stress-only kernel
    const double* h_in[kNH];
    double* h_out[kNH];
    unsigned long long* nonconv;
    long long n;
    double t, del_t;
    double factor;
    double params[kMaxParams];
};

template <int NC>
__device__ __forceinline__ void user_in(const Chunks<NC>& c, double* region, int lane, double (&x)[NC]) {
    static_assert(NC <= kUserMaxDim, "history field wider than the LDS region");
    if constexpr (NC <= kUserWide) {
        transpose_in<NC>(c, region, lane, x);
    } else {
        constexpr int kHalf = 16 * NC;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int k = 0; k < Chunks<NC>::K; ++k) {
                const int q = k * kWave + lane - h * kHalf;
                if (q >= 0 && q < kHalf && chunk_live<NC>(k, lane)) reinterpret_cast<d2*>(region)[q] = c.v[k];
            }
            wave_sync();
            if ((lane >> 5) == h) {
#pragma unroll
                for (int i = 0; i < NC; ++i) x[i] = region[(lane & 31) * NC + i];
            }
            wave_sync();
        }
    }
}

template <int NC, bool FULL, bool NT>
__device__ __forceinline__ void user_out(const double (&x)[NC], double* region, int lane, double* dst, int nelem) {
    static_assert(NC <= kUserMaxDim, "history field wider than the LDS region");
    if constexpr (NC <= kUserWide) {
        transpose_out<NC, FULL, NT>(x, region, lane, dst, nelem);
    } else {
        constexpr int kHalf = 16 * NC;
        constexpr int kPer = (kHalf + kWave - 1) / kWave;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if ((lane >> 5) == h) {
#pragma unroll
                for (int i = 0; i < NC; ++i) region[(lane & 31) * NC + i] = x[i];
            }
            wave_sync();
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const int q = k * kWave + lane;
                if (q < kHalf) {
                    const d2 v = reinterpret_cast<const d2*>(region)[q];
                    const int e = 2 * (q + h * kHalf);
                    if constexpr (FULL) {
                        store16<NT>(dst + e, v);
                    } else {
                        if (e < nelem) dst[e] = v.x;
                        if (e + 1 < nelem) dst[e + 1] = v.y;
                    }
                }
            }
            wave_sync();
        }
    }
}

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

// one 64-point tile (FULL) or the ragged last one (npts < 64); returns the tile's non-converged points (wave-uniform)
template <bool FULL, bool NT>
__device__ __forceinline__ unsigned long long user_tile(const UserArgs& a, const UserParams& p, double* region, long long p0,
                                                        int npts, int lane) {
    Chunks<9> cg;
    Chunks<6> cs;
    tile_load<9, FULL, NT>(cg, a.grad + p0 * 9, npts * 9, lane);
    tile_load<6, FULL, NT>(cs, a.stress_in + p0 * 6, npts * 6, lane);
#define FCAMD_X(k, name, dim) \
    Chunks<dim> c_##name;     \
    tile_load<dim, FULL, NT>(c_##name, a.h_in[k] + p0 * (dim), npts * (dim), lane);
    FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
    double g[9], s[6], e[6];
    UserHistoryT<double> h;
    transpose_in<9>(cg, region, lane, g);
    transpose_in<6>(cs, region, lane, s);
#define FCAMD_X(k, name, dim) user_in<dim>(c_##name, region, lane, h.name);
    FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
#ifdef FCAMD_USER_ROTATE
    fcamd_user_rotate(g, s, h);  // objective rate (rotation.h): the double committed state, before any Dual is seeded
#endif
    mandel_strain(g, a.factor, e);
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

extern "C" __global__ void __launch_bounds__(fcamd::kBlock, FCAMD_USER_WAVES) fcamd_user_law_kernel(const fcamd_user::UserArgs a) {
    using namespace fcamd_user;
    __shared__ __attribute__((aligned(16))) double scratch[kWavesPerBlock][kUserRegion];
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    double* region = scratch[wave];
    const UserParams p = fcamd_user_params(a.params);
    const long long nfull = a.n / kWave;
    const long long wstride = (long long)gridDim.x * kWavesPerBlock;
    unsigned long long bad = 0;
    long long tile = (long long)blockIdx.x * kWavesPerBlock + wave;
    for (; tile < nfull; tile += wstride) bad += user_tile<true, true>(a, p, region, tile * kWave, kWave, lane);
    if (tile == nfull && a.n > nfull * kWave) bad += user_tile<false, false>(a, p, region, tile * kWave, (int)(a.n - tile * kWave), lane);
    if (bad != 0 && lane == 0) atomicAdd(a.nonconv, bad);
}
