// Kernel template of the 1-D / 2-D wrappers around a user law (wrappers.py: UniaxialStrainFrom3D, PlaneStrainFrom3D,
// PlaneStressFrom3D, UniaxialStressFrom3D around a UserLaw with an explicit or an autodiff tangent): map, evaluate and map back
// in one launch.  Compiled behind the generated definitions that user_law_tile.h lists and
//   FCAMD_USER_WRAP          the built-in kernels' numbering (kernels/wrapped_io.h, stress_wrapped.h): 1 uniaxial strain, 2 plane
//                            strain, 3 plane stress, 4 uniaxial stress
//   FCAMD_USER_AD_K          defined (0) for an autodiff law (fcamd_user_stress<T>), undefined for an explicit one (fcamd_user_point)
//
// One point.  The mapping is wrapped_load / wrapped_store_stress of kernels/wrapped_io.h, restated on this
// template's own argument struct: the low-dimensional gradient is padded with zeros (1-D: g[0]; 2-D: (0,1,2,3) -> (0,1,3,4)), the
// committed 3-D stress row is the wrapper's cached one with the mapped Mandel components from the caller (0 or 0..3), the full
// row goes back to the cache and the mapped components to the caller (plane-stress zz as exactly 0.0).  No 3-D gradient or
// tangent array exists.
//
// Strain wrappers (1, 2): one evaluation of the law's point function on the padded point -- the bits of the evaluate kernel on
// the padded arrays.  The tangent is the block [0:4, 0:4] (entry [0][0]) of the 3-D one: the entries of the D an explicit law
// returns, or the partials of ONE fcamd_user_stress<Dual<K>> pass seeded on the mapped strain components only (K = 4 / 1),
// which is also the evaluation.
//
// Stress wrappers (3, 4): the rule of wrappers._StressFrom3D._evaluate_3d for a law without a known elastic tangent, per lane in
// registers.  The free increments (3: d_eps_zz; 4: d_eps_yy, d_eps_zz) start at 0; every evaluation starts from the committed
// stress and history, kept in registers next to the trial state; a lane is converged when sigma_b == 0 or
// |sigma_b|_inf <= 1e-12 |sigma|_2 (six Mandel components, summed in index order), otherwise d <- d - C_bb^-1 sigma_b with that
// iterate's tangent in the closed forms of stress_wrapped.h; a non-finite update or 50 evaluations without convergence fail
// the lane.  The wave evaluates until no lane updates; a lane that has finished keeps its increment, so its last evaluation
// repeats its bits and no result depends on the other points of the wave.  Outputs are those of the last evaluation; the
// tangent is the Schur complement in the expressions of wrappers._condense.  For an autodiff law C comes from one Dual<4> pass
// (plane stress) or one Dual<3> pass on components 0, 1, 2 (uniaxial stress): the Newton block and all the condensation needs.
//
// Memory: per point the low-dimensional gradient, stress and tangent, the 48-byte cache row in and out and the history in and
// out.  Full tiles move 16-byte non-temporal chunks through the wave's LDS region, the ragged last tile guarded 8-byte accesses.
#pragma once
#ifdef FCAMD_USER_FIELDS
#error "the 1-D / 2-D wrappers take no per-point parameter fields"
#endif
#ifdef FCAMD_USER_ROTATE
#error "the 1-D / 2-D wrappers take no objective rate"
#endif
#include "user_law_tile.h"

namespace fcamd_user {

constexpr int kWrap = FCAMD_USER_WRAP;
static_assert(kWrap >= 1 && kWrap <= 4, "FCAMD_USER_WRAP: 1 uniaxial strain, 2 plane strain, 3 plane stress, 4 uniaxial stress");
constexpr bool kWrap1D = kWrap == 1 || kWrap == 4;
constexpr int kLD = kWrap1D ? 1 : 4;                          // doubles per point of the low-dimensional gradient and stress
constexpr int kCols = kWrap == 1 ? 1 : kWrap == 4 ? 3 : 4;    // strain components 0 .. kCols - 1 whose tangent columns are formed
constexpr int kWrapMaxIter = 50;                              // wrappers.STRESS_WRAP_MAX_ITER
constexpr double kWrapRtol = 1e-12;                           // wrappers.STRESS_WRAP_RTOL

#ifdef FCAMD_USER_AD_K
using WrappedHistory = UserHistoryT<double>;
#else
using WrappedHistory = UserHistory;
#endif

// the only kernel parameter; userlaw.py mirrors the layout (_wrapped_args_type).  In place, as the wrappers are.
struct WrappedArgs {
    const double* grad;          // [n] or [4 n]: the low-dimensional gradient
    double* stress;              // [n] or [4 n]: the mapped committed stress in, the mapped stress out
    double* tangent;             // [n] or [16 n]: the low-dimensional (condensed) tangent
    double* cache3d;             // [6 n]: the wrapper's cached 3-D stress rows, in and out
    double* h[kNH];              // history fields, in and out
    unsigned long long* nonconv; // one word: points whose last evaluation returned non-zero or whose local iteration failed
    long long n;                 // points
    double t, del_t;
    double factor;               // Mandel factor of the off-diagonal strains (the Python laws')
    double params[kMaxParams];   // UserParams, in order
};

// one evaluation of the lane's point from the committed state (s, h) on the gradient g: trial state (st, ht), the return code
// and the tangent columns J[kCols i + j] = d sigma_i / d eps_j, j < kCols
__device__ __forceinline__ int wrapped_point(const WrappedArgs& a, const UserParams& p, const double (&g)[9], const double (&s)[6],
                                             const WrappedHistory& h, double (&st)[6], WrappedHistory& ht, double (&J)[6 * kCols]) {
    double e[6];
    mandel_strain(g, a.factor, e);
#ifndef FCAMD_USER_AD_K
#pragma unroll
    for (int i = 0; i < 6; ++i) st[i] = s[i];
    ht = h;
    double D[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) D[i] = 0.0;
    const int rc = fcamd_user_point(p, a.t, a.del_t, g, e, st, D, ht);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < kCols; ++j) J[kCols * i + j] = D[6 * i + j];
    return rc;
#else
    // the seeds sit on the Mandel strain, as in the tangent kernel (user_law_ad.hip): direction k is component k
    using T = Dual<kCols>;
    T te[6], ts[6];
    UserHistoryT<T> th;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        te[j] = T(e[j]);
#pragma unroll
        for (int k = 0; k < kCols; ++k) te[j].d[k] = j == k ? 1.0 : 0.0;
        ts[j] = T(s[j]);
    }
#define FCAMD_X(k, name, dim) \
    _Pragma("unroll") for (int i = 0; i < (dim); ++i) th.name[i] = T(h.name[i]);
    FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
    const int rc = fcamd_user_stress<T>(p, a.t, a.del_t, te, ts, th);
#pragma unroll
    for (int i = 0; i < 6; ++i) st[i] = ts[i].v;
#define FCAMD_X(k, name, dim) \
    _Pragma("unroll") for (int i = 0; i < (dim); ++i) ht.name[i] = th.name[i].v;
    FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < kCols; ++j) J[kCols * i + j] = ts[i].d[j];
    return rc;
#endif
}

// one 64-point tile (FULL) or the ragged last one (npts < 64); returns the tile's failed points (wave-uniform)
template <bool FULL, bool NT>
__device__ __forceinline__ unsigned long long wrapped_tile(const WrappedArgs& a, const UserParams& p, double* region, long long p0,
                                                           int npts, int lane) {
    const bool live = FULL || lane < npts;
    double g[9], s[6];
    WrappedHistory h;
    {
        // every load of the tile is issued before the first transposition
        Chunks<6> cc;
        Chunks<kLD> cg, cs;
        tile_load<6, FULL, NT>(cc, a.cache3d + p0 * 6, npts * 6, lane);
        tile_load<kLD, FULL, NT>(cg, a.grad + p0 * kLD, npts * kLD, lane);
        tile_load<kLD, FULL, NT>(cs, a.stress + p0 * kLD, npts * kLD, lane);
#define FCAMD_X(k, name, dim) \
    Chunks<dim> c_##name;     \
    tile_load<dim, FULL, NT>(c_##name, a.h[k] + p0 * (dim), npts * (dim), lane);
        FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
        double g_lo[kLD], s_lo[kLD];
        transpose_in<kLD>(cg, region, lane, g_lo);
        transpose_in<kLD>(cs, region, lane, s_lo);
        transpose_in<6>(cc, region, lane, s);
#define FCAMD_X(k, name, dim) user_in<dim>(c_##name, region, lane, h.name);
        FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
#pragma unroll
        for (int i = 0; i < 9; ++i) g[i] = 0.0;
        if constexpr (kWrap1D) {
            g[0] = g_lo[0];
        } else {
            g[0] = g_lo[0], g[1] = g_lo[1], g[3] = g_lo[2], g[4] = g_lo[3];
        }
#pragma unroll
        for (int i = 0; i < kLD; ++i) s[i] = s_lo[i];  // mapped components come from the caller, the others persist
    }

    double st[6], J[6 * kCols];
    WrappedHistory ht;
    int rc = wrapped_point(a, p, g, s, h, st, ht, J);
    bool failed = false;
    if constexpr (kWrap >= 3) {
        double d0 = 0.0, d1 = 0.0;  // 3: d_eps_zz; 4: d_eps_yy, d_eps_zz
        bool done = false;
        for (int evals = 1;; ++evals) {
            double nn = st[0] * st[0];
#pragma unroll
            for (int i = 1; i < 6; ++i) nn = nn + st[i] * st[i];
            const double tol = kWrapRtol * sqrt(nn);
            bool conv;
            double n0, n1 = 0.0;
            if constexpr (kWrap == 3) {
                const double r = st[2];
                conv = r == 0.0 || __builtin_fabs(r) <= tol;
                n0 = d0 - r / J[kCols * 2 + 2];
            } else {
                const double r1 = st[1], r2 = st[2];
                conv = (r1 == 0.0 && r2 == 0.0) || __builtin_fmax(__builtin_fabs(r1), __builtin_fabs(r2)) <= tol;
                const double c11 = J[kCols * 1 + 1], c12 = J[kCols * 1 + 2], c21 = J[kCols * 2 + 1], c22 = J[kCols * 2 + 2];
                const double det = c11 * c22 - c12 * c21;
                n0 = d0 - (c22 * r1 - c12 * r2) / det;
                n1 = d1 - (c11 * r2 - c21 * r1) / det;
            }
            done = done || conv || !live;
            const bool finite = __builtin_isfinite(n0) && __builtin_isfinite(n1);
            const bool step = !done && evals < kWrapMaxIter && finite;
            failed = failed || (!done && !step);  // out of evaluations, or a singular C_bb / a non-finite update
            done = done || failed;
            if (__builtin_amdgcn_ballot_w64(step) == 0ull) break;  // nobody moved: the last evaluation stands
            d0 = step ? n0 : d0;  // a finished lane keeps its increment
            d1 = step ? n1 : d1;
            if constexpr (kWrap == 3) {
                g[8] = d0;
            } else {
                g[4] = d0;
                g[8] = d1;
            }
            rc = wrapped_point(a, p, g, s, h, st, ht, J);
        }
    }
    const unsigned long long bad = __builtin_amdgcn_ballot_w64(live && (rc != 0 || failed));

    // the full row to the cache, the mapped components to the caller
    transpose_out<6, FULL, NT>(st, region, lane, a.cache3d + p0 * 6, npts * 6);
    {
        double s_lo[kLD];
#pragma unroll
        for (int i = 0; i < kLD; ++i) s_lo[i] = (kWrap == 3 && i == 2) ? 0.0 : st[i];  // plane stress: the constrained zz is exactly 0
        transpose_out<kLD, FULL, NT>(s_lo, region, lane, a.stress + p0 * kLD, npts * kLD);
    }
#define FCAMD_X(k, name, dim) user_out<dim, FULL, NT>(ht.name, region, lane, a.h[k] + p0 * (dim), npts * (dim));
    FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X

    if constexpr (kWrap == 1) {
        double ct[1] = {J[0]};
        transpose_out<1, FULL, NT>(ct, region, lane, a.tangent + p0, npts);
    } else if constexpr (kWrap == 2) {
        double ct[16];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) ct[4 * i + j] = J[kCols * i + j];
        transpose_out<16, FULL, NT>(ct, region, lane, a.tangent + p0 * 16, npts * 16);
    } else if constexpr (kWrap == 3) {
        // C_ij - (C_i2 / C_22) C_2j, row and column 2 exactly zero
        const double c22 = J[kCols * 2 + 2];
        double ct[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double u = i == 2 ? 0.0 : J[kCols * i + 2] / c22;
#pragma unroll
            for (int j = 0; j < 4; ++j) ct[4 * i + j] = (i == 2 || j == 2) ? 0.0 : J[kCols * i + j] - u * J[kCols * 2 + j];
        }
        transpose_out<16, FULL, NT>(ct, region, lane, a.tangent + p0 * 16, npts * 16);
    } else {
        // C00 - [C01 C02] C_bb^-1 [C10 C20]^T
        const double c11 = J[kCols * 1 + 1], c12 = J[kCols * 1 + 2], c21 = J[kCols * 2 + 1], c22 = J[kCols * 2 + 2];
        const double c10 = J[kCols * 1 + 0], c20 = J[kCols * 2 + 0];
        const double det = c11 * c22 - c12 * c21;
        const double y1 = (c22 * c10 - c12 * c20) / det, y2 = (c11 * c20 - c21 * c10) / det;
        double ct[1] = {J[0] - (J[1] * y1 + J[2] * y2)};
        transpose_out<1, FULL, NT>(ct, region, lane, a.tangent + p0, npts);
    }
    return (unsigned long long)__popcll(bad);
}

}  // namespace fcamd_user

extern "C" __global__ void __launch_bounds__(fcamd::kBlock, FCAMD_USER_WAVES) fcamd_user_law_wrapped_kernel(const fcamd_user::WrappedArgs a) {
    using namespace fcamd_user;
    __shared__ __attribute__((aligned(16))) double scratch[kWavesPerBlock][kUserRegion];
    const int lane = (int)threadIdx.x & (kWave - 1);
    // wave index as a scalar: tile index and the tile base pointers live in SGPRs
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    double* region = scratch[wave];
    const UserParams p = fcamd_user_params(a.params);
    const long long nfull = a.n / kWave;
    const long long wstride = (long long)gridDim.x * kWavesPerBlock;
    unsigned long long bad = 0;
    long long tile = (long long)blockIdx.x * kWavesPerBlock + wave;
    for (; tile < nfull; tile += wstride) bad += wrapped_tile<true, true>(a, p, region, tile * kWave, kWave, lane);
    if (tile == nfull && a.n > nfull * kWave) bad += wrapped_tile<false, false>(a, p, region, tile * kWave, (int)(a.n - tile * kWave), lane);
    if (bad != 0 && lane == 0) atomicAdd(a.nonconv, bad);
}
