// Fused 3D -> plane-stress / uniaxial-stress wrapper tiles (PlaneStressFrom3D / UniaxialStressFrom3D): a per-point local
// Newton iteration on the out-of-plane strain increments around the 3-D laws' own point functions.
// Part of the device code of libfcamd (translation unit: ../fcamd_kernels.hip, which holds the kernels and launchers).
#pragma once
#include "tile_io.h"
#include "wrapped_io.h"
#include "history_rows.h"
#include "law_von_mises.h"
#include "law_comfe_mises.h"
#include "law_drucker_prager.h"

namespace fcamd {

// WRAP = 3 (plane stress): the 2-D gradient maps to 3-D as under plane strain, the unknown is d_eps_zz (Mandel component 2).
// WRAP = 4 (uniaxial stress): component 11 of gradient and stress, the unknowns are d_eps_yy and d_eps_zz (components 1, 2).
// The committed 3-D stress row is the cached one with the mapped components from the caller (Mandel 0..3 / 0), the history
// is the 3-D law's.  Per point:
//   start      C^e_bb d = -(sigma0_b + C^e_ba d_eps_a) with the law's elastic tangent (an elastic point is done after one evaluation)
//   iterate    evaluate the 3-D point update from the committed stress and history; r = sigma_b;
//              converged if |r|_inf <= 1e-12 |sigma|_2 (Mandel) or r == 0, else d <- d - C_bb^-1 r with that iterate's tangent
//   give up    after kStressWrapMaxIter evaluations, or when C_bb is singular / the step is not finite: counted non-converged
//   outputs    those of the last evaluated iterate: history, the full 3-D stress row to the cache, the mapped components to the
//              caller (plane-stress zz written as 0.0), the Schur complement C_aa - C_ab C_bb^-1 C_ba in the low-dimensional layout
// The committed stress and the committed [alpha, plastic strain] rows are parked in the wave's LDS region (structure of arrays,
// conflict-free) during the loop; the loop ends when the ballot of the unconverged lanes is empty.  Tangent entries are formed
// per lane from the law's compact coefficients (never a 6x6 matrix); only entries (i, j) with i, j < 4 exist here.
constexpr int kStressWrapMaxIter = 50;
constexpr double kStressWrapRtol = 1e-12;
// LDS region of a stress-wrapper wave: the 4x4 condensed tangent of 64 points leaves through it (16 doubles per point)
constexpr int kStressWrapRegion = 64 * 16;

template <int LAW>
struct SWPoint;

// LinearElasticityModel: sigma = sigma0 + d_eps @ D, tangent D (table c)
template <>
struct SWPoint<LAW_LE> {
    static constexpr int kHist = 0;
    double s[6];
    bool plastic = false;
    __device__ __forceinline__ static double elastic(ScalarsRef, const Tables* T, int i, int j) { return T->c[6 * i + j]; }
    __device__ __forceinline__ double at(ScalarsRef sc, const Tables* T, int i, int j) const { return elastic(sc, T, i, j); }
    __device__ __forceinline__ void eval(ScalarsRef, const Tables* T, bool, const double (&e)[6], const double (&s0)[6],
                                         const double*, int, double, WaveStats&) {
        double ds[6];
        row_times_matrix_fma(e, T->a, ds);
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i] = s0[i] + ds[i];
    }
};

// VonMises3D: the eps_n rows only accumulate (eps_n += gamma N), so only alpha enters the loop
template <>
struct SWPoint<LAW_VM3D> {
    static constexpr int kHist = 0;
    double s[6], B, C;
    VMReturn rm;
    bool plastic = false;
    __device__ __forceinline__ static double elastic(ScalarsRef sc, const Tables* T, int i, int j) {
        return T->a[6 * i + j] + sc.s[2] * T->b[6 * i + j];
    }
    __device__ __forceinline__ double at(ScalarsRef, const Tables* T, int i, int j) const {
        return (T->a[6 * i + j] + B * T->b[6 * i + j]) + C * (rm.N[i] * rm.N[j]);  // as tangent_mises forms it
    }
    __device__ __forceinline__ void eval(ScalarsRef sc, const Tables*, bool live, const double (&e)[6], const double (&s0)[6],
                                         const double*, int, double alpha_n, WaveStats& st) {
        VMTrial tr;
        vm_trial(sc, e, s0, alpha_n, tr);
        plastic = live && (tr.phitr > 0.0);
        rm = VMReturn();
        if (plastic) vm_return(sc, tr, alpha_n, rm, st);
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i] = s0[i];
        vm_stress(sc, tr, rm, s);
        vm_tangent_coefficients(sc, rm, B, C);
    }
};

// comfe-rs MisesPlasticity3D: history [alpha, eps_p(6)] parked with the stress
template <>
struct SWPoint<LAW_COMFE_MISES> {
    static constexpr int kHist = 7;
    double s[6], h[7], B, sc2, nv[6];
    bool plastic = false;
    __device__ __forceinline__ static double elastic(ScalarsRef sc, const Tables* T, int i, int j) {
        return T->a[6 * i + j] + sc.s[5] * T->b[6 * i + j];
    }
    __device__ __forceinline__ double at(ScalarsRef, const Tables* T, int i, int j) const {
        return (T->a[6 * i + j] + B * T->b[6 * i + j]) + (sc2 * nv[j]) * nv[i];
    }
    __device__ __forceinline__ void eval(ScalarsRef sc, const Tables*, bool live, const double (&e)[6], const double (&s0)[6],
                                         const double* park, int lane, double, WaveStats&) {
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i] = s0[i];
#pragma unroll
        for (int i = 0; i < 7; ++i) h[i] = park[(6 + i) * kWave + lane];
        plastic = cm_point(sc, live, e, s, h, B, sc2, nv);
    }
};

// the Drucker-Prager laws: history [alpha, plastic strain(6)] parked with the stress
template <bool HYPER>
struct SWPointDP {
    static constexpr int kHist = 7;
    double s[6], h[7], sd[4];  // sd: rho s_tr, components 0..3
    DPTangent tg;
    bool plastic = false, tip = false;
    __device__ __forceinline__ static double elastic(ScalarsRef, const Tables* T, int i, int j) { return T->c[6 * i + j]; }
    __device__ __forceinline__ double at(ScalarsRef, const Tables* T, int i, int j) const {
        // as tangent_dp_chunk forms it; elastic points carry E itself
        if (!plastic) return T->c[6 * i + j];
        const double oi = i < 3 ? 1.0 : 0.0, oj = j < 3 ? 1.0 : 0.0;
        return (tg.t11 * T->a[6 * i + j] + tg.tP * T->b[6 * i + j]) + ((tg.tss * sd[i]) * sd[j] + (tg.t1s * oi) * sd[j] + (tg.ts1 * sd[i]) * oj);
    }
    __device__ __forceinline__ void eval(ScalarsRef sc, const Tables*, bool live, const double (&e)[6], const double (&s0)[6],
                                         const double* park, int lane, double, WaveStats& st) {
#pragma unroll
        for (int i = 0; i < 7; ++i) h[i] = park[(6 + i) * kWave + lane];
        DPTrial t;
        dp_trial<HYPER>(sc, e, s0, t);
        plastic = live && (t.m.f > 0.0);
        tg = DPTangent();
        tg.t11 = sc.s[2], tg.tP = sc.s[7];
        if (plastic) dp_return<HYPER>(sc, e, s0, t, h, tg, st);
        tip = t.tip;
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i] = t.sig1[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) sd[i] = tg.rho * t.s_tr[i];
    }
};
template <>
struct SWPoint<LAW_COMFE_DP> : SWPointDP<false> {};
template <>
struct SWPoint<LAW_COMFE_DP_HYPER> : SWPointDP<true> {};

// one point's local iteration; `park` holds the committed stress (rows 0..5) and history (rows 6..12) of the wave's points
template <int LAW, int WRAP>
__device__ __forceinline__ void stress_wrap_iterate(ScalarsRef sc, const Tables* T_in, bool live, const double (&e_in)[6],
                                                    const double* park, int lane, double alpha_n, SWPoint<LAW>& pt,
                                                    WaveStats& st) {
    using P = SWPoint<LAW>;
    // elastic start
    double d0, d1 = 0.0;
    {
        const Tables* T = T_in;
        double s0[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) s0[i] = park[i * kWave + lane];
        if constexpr (WRAP == 3) {
            const double rhs = s0[2] + ((P::elastic(sc, T, 2, 0) * e_in[0] + P::elastic(sc, T, 2, 1) * e_in[1]) + P::elastic(sc, T, 2, 3) * e_in[3]);
            d0 = -rhs / P::elastic(sc, T, 2, 2);
        } else {
            const double r1 = s0[1] + P::elastic(sc, T, 1, 0) * e_in[0], r2 = s0[2] + P::elastic(sc, T, 2, 0) * e_in[0];
            const double c11 = P::elastic(sc, T, 1, 1), c12 = P::elastic(sc, T, 1, 2), c21 = P::elastic(sc, T, 2, 1), c22 = P::elastic(sc, T, 2, 2);
            const double det = c11 * c22 - c12 * c21;
            d0 = -((c22 * r1 - c12 * r2) / det);
            d1 = -((c11 * r2 - c21 * r1) / det);
        }
    }
    bool active = true, failed = false;
    int evals = 0;
    for (;;) {
        if (active) {
            // the LDS tables are loop-invariant: left alone, the compiler hoists their entries out of the loop into registers
            const Tables* T = T_in;
            asm volatile("" : "+s"(T));
            double e[6], s0[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) e[i] = e_in[i], s0[i] = park[i * kWave + lane];
            if constexpr (WRAP == 3) {
                e[2] = d0;
            } else {
                e[1] = d0;
                e[2] = d1;
            }
            pt.eval(sc, T, live, e, s0, park, lane, alpha_n, st);
            ++evals;
            double nn = pt.s[0] * pt.s[0];
#pragma unroll
            for (int i = 1; i < 6; ++i) nn = nn + pt.s[i] * pt.s[i];
            const double tol = kStressWrapRtol * sqrt(nn);
            bool conv;
            if constexpr (WRAP == 3) {
                const double r = pt.s[2];
                conv = r == 0.0 || __builtin_fabs(r) <= tol;
                if (!conv) {
                    const double c = pt.at(sc, T, 2, 2);
                    const double nd = d0 - r / c;
                    if (!__builtin_isfinite(nd)) failed = true;
                    d0 = nd;
                }
            } else {
                const double r1 = pt.s[1], r2 = pt.s[2];
                conv = (r1 == 0.0 && r2 == 0.0) || fmax(__builtin_fabs(r1), __builtin_fabs(r2)) <= tol;
                if (!conv) {
                    const double c11 = pt.at(sc, T, 1, 1), c12 = pt.at(sc, T, 1, 2), c21 = pt.at(sc, T, 2, 1), c22 = pt.at(sc, T, 2, 2);
                    const double det = c11 * c22 - c12 * c21;
                    const double n0 = d0 - (c22 * r1 - c12 * r2) / det, n1 = d1 - (c11 * r2 - c21 * r1) / det;
                    if (!__builtin_isfinite(n0) || !__builtin_isfinite(n1)) failed = true;
                    d0 = n0, d1 = n1;
                }
            }
            if (!conv && evals >= kStressWrapMaxIter) failed = true;
            active = !conv && !failed;
        }
        if (__ballot(active) == 0ull) break;
    }
    st.nonconv += (live && failed) ? 1ull : 0ull;
}

template <int LAW, int WRAP, bool FULL, bool NT>
__device__ __forceinline__ void tile_stress_wrapped(ArgsRef a, const Tables* T, double* region, long long p0, int npts, int lane,
                                                    WaveStats& st) {
    using P = SWPoint<LAW>;
    const bool live = FULL || lane < npts;
    Chunks<7> ch;
    if constexpr (P::kHist == 7) tile_load<7, FULL, NT>(ch, a.h0_in + p0 * 7, npts * 7, lane);
    const double alpha_n = (LAW == LAW_VM3D && live) ? a.h1_in[p0 + lane] : 0.0;
    double g[9], s0[6], e[6];
    wrapped_load<WRAP, FULL, NT>(a, region, p0, npts, lane, g, s0);
    mandel_strain(g, a.sc.s[0], e);
    if constexpr (P::kHist == 7) {
        double h[7];
        transpose_in<7>(ch, region, lane, h);
#pragma unroll
        for (int i = 0; i < 7; ++i) region[(6 + i) * kWave + lane] = h[i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) region[i * kWave + lane] = s0[i];

    P pt;
    stress_wrap_iterate<LAW, WRAP>(a.sc, T, live, e, region, lane, alpha_n, pt, st);
    wave_sync();  // the parked rows are dead: the region serves the transpositions below

    const unsigned long long mask = __ballot(live && pt.plastic);
    st.plastic += (lane == 0) ? (unsigned long long)__popcll(mask) : 0ull;
    if constexpr (LAW == LAW_COMFE_DP || LAW == LAW_COMFE_DP_HYPER) st.domain += (live && pt.tip) ? 1ull : 0ull;

    if constexpr (LAW == LAW_VM3D) {
        MaskedRows<FULL, NT> er;
        if (mask != 0ull) er.request(a.h0_in, p0, npts, lane, mask, a.masked_max);
        double ep[6];
        if (mask != 0ull) er.gather(region, lane, ep);
        wrapped_store_stress<WRAP, FULL, NT>(a, region, p0, npts, lane, pt.s);
        if (mask != 0ull) {
#pragma unroll
            for (int i = 0; i < 6; ++i) ep[i] = pt.plastic ? ep[i] + pt.rm.gamma * pt.rm.N[i] : ep[i];
            er.store(a.h0_out, p0, npts, lane, region, ep);
            if (live && ((mask >> (lane & ~3)) & 0xFull) != 0ull) a.h1_out[p0 + lane] = alpha_n + a.sc.s[3] * pt.rm.gamma;
        }
    } else {
        wrapped_store_stress<WRAP, FULL, NT>(a, region, p0, npts, lane, pt.s);
        if constexpr (P::kHist == 7) {
            if (mask != 0ull) transpose_out<7, FULL, NT>(pt.h, region, lane, a.h0_out + p0 * 7, npts * 7);
        }
    }

    if (a.tangent) {
        const ScalarsRef sc = a.sc;
        if constexpr (WRAP == 4) {
            // C00 - [C01 C02] C_bb^-1 [C10 C20]^T
            const double c11 = pt.at(sc, T, 1, 1), c12 = pt.at(sc, T, 1, 2), c21 = pt.at(sc, T, 2, 1), c22 = pt.at(sc, T, 2, 2);
            const double c10 = pt.at(sc, T, 1, 0), c20 = pt.at(sc, T, 2, 0);
            const double det = c11 * c22 - c12 * c21;
            const double y1 = (c22 * c10 - c12 * c20) / det, y2 = (c11 * c20 - c21 * c10) / det;
            const double v = pt.at(sc, T, 0, 0) - (pt.at(sc, T, 0, 1) * y1 + pt.at(sc, T, 0, 2) * y2);
            if (live) a.tangent[p0 + lane] = v;
        } else {
            // C_ij - (C_i2 / C_22) C_2j, row and column 2 exactly zero; 16 doubles per point through the region
            const double c22 = pt.at(sc, T, 2, 2);
            double ct[16];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double u = i == 2 ? 0.0 : pt.at(sc, T, i, 2) / c22;
#pragma unroll
                for (int j = 0; j < 4; ++j) ct[4 * i + j] = (i == 2 || j == 2) ? 0.0 : pt.at(sc, T, i, j) - u * pt.at(sc, T, 2, j);
            }
            transpose_out<16, FULL, NT>(ct, region, lane, a.tangent + p0 * 16, npts * 16);
        }
    }
}

}  // namespace fcamd
