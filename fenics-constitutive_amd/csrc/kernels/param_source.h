// Where a law's constants come from: the launch's uniform Scalars (fill_constants in fcamd_capi.cpp), or -- the field kernels,
// evaluate_fields_kernel -- the raw parameters of each lane's own point, from which the constants are derived in registers.
// Part of the device code of libfcamd (translation unit: ../fcamd_kernels.hip, which holds the kernels and launchers).
//
// Parity rule: a lane source derives every constant with the very expression and operation order of fill_constants / lame /
// elastic_tangent_full, without FP contraction, so a field whose values all equal v gives the bits of the scalar law with v.
// Only the raw values stay live (5 doubles for VonMises3D); a derived constant is computed where it is used.
#pragma once
#include "tile_io.h"

namespace fcamd {

// (the library is built with -ffp-contract=off; the derivations below must stay uncontracted whatever the build flags say)
#pragma clang fp contract(off)

// raw parameter k of the point p0 + lane: its field value, or the model's scalar (also for the idle lanes of a ragged tile)
__device__ __forceinline__ double field_value(int k, long long p0, int lane, bool live) {
    FieldsRef fa = field_args();
    const double* f = fa.f[k];
    return (f != nullptr && live) ? f[p0 + lane] : fa.v[k];
}

// --- VonMises3D: s[1]=ka, s[2]=2*mu, s[3]=sqrt(2/3), s[4]=y0, s[5]=y00-y0, s[6]=-w, s[7]=(-2)*mu, s[8]=((2/3)*(y00-y0))*w,
//     s[9]=(4*mu)*mu; table a = ka*xioi
struct VMUniform {
    ScalarsRef sc;
    __device__ __forceinline__ double ka() const { return sc.s[1]; }
    __device__ __forceinline__ double two_mu() const { return sc.s[2]; }
    __device__ __forceinline__ double s23() const { return sc.s[3]; }
    __device__ __forceinline__ double y0() const { return sc.s[4]; }
    __device__ __forceinline__ double dy() const { return sc.s[5]; }
    __device__ __forceinline__ double mw() const { return sc.s[6]; }
    __device__ __forceinline__ double m2mu() const { return sc.s[7]; }
    __device__ __forceinline__ double c23dyw() const { return sc.s[8]; }
    __device__ __forceinline__ double four_mu2() const { return sc.s[9]; }
};
struct VMLane {
    ScalarsRef sc;  // the parameter-free constant sqrt(2/3)
    double ka_, mu, y0_, y00, w;
    __device__ __forceinline__ double ka() const { return ka_; }
    __device__ __forceinline__ double two_mu() const { return 2 * mu; }
    __device__ __forceinline__ double s23() const { return sc.s[3]; }
    __device__ __forceinline__ double y0() const { return y0_; }
    __device__ __forceinline__ double dy() const { return y00 - y0_; }
    __device__ __forceinline__ double mw() const { return -w; }
    __device__ __forceinline__ double m2mu() const { return -2 * mu; }
    __device__ __forceinline__ double c23dyw() const { return (2.0 / 3.0) * (y00 - y0_) * w; }
    __device__ __forceinline__ double four_mu2() const { return 4 * mu * mu; }
};
template <bool FIELDS>
__device__ __forceinline__ auto vm_params(ArgsRef a, long long p0, int lane, bool live) {
    if constexpr (FIELDS)  // params: p_ka, p_mu, p_y0, p_y00, p_w
        return VMLane{a.sc, field_value(0, p0, lane, live), field_value(1, p0, lane, live), field_value(2, p0, lane, live),
                      field_value(3, p0, lane, live), field_value(4, p0, lane, live)};
    else
        return VMUniform{a.sc};
}

// --- comfe-rs MisesPlasticity3D: s[2]=kappa, s[3]=y_0, s[4]=h, s[5]=2*mu, s[6]=3*mu+h, s[7]=sqrt(3/2), s[8]=3*mu,
//     s[9]=1/(1+h/(3 mu)); table a = kappa*soo
struct CMUniform {
    ScalarsRef sc;
    __device__ __forceinline__ double kappa() const { return sc.s[2]; }
    __device__ __forceinline__ double y_0() const { return sc.s[3]; }
    __device__ __forceinline__ double h() const { return sc.s[4]; }
    __device__ __forceinline__ double two_mu() const { return sc.s[5]; }
    __device__ __forceinline__ double den() const { return sc.s[6]; }
    __device__ __forceinline__ double s32() const { return sc.s[7]; }
    __device__ __forceinline__ double three_mu() const { return sc.s[8]; }
    __device__ __forceinline__ double hfac() const { return sc.s[9]; }
};
struct CMLane {
    ScalarsRef sc;  // the parameter-free constant sqrt(3/2)
    double mu, kappa_, y_0_, h_;
    __device__ __forceinline__ double kappa() const { return kappa_; }
    __device__ __forceinline__ double y_0() const { return y_0_; }
    __device__ __forceinline__ double h() const { return h_; }
    __device__ __forceinline__ double two_mu() const { return 2. * mu; }
    __device__ __forceinline__ double den() const { return 3. * mu + h_; }
    __device__ __forceinline__ double s32() const { return sc.s[7]; }
    __device__ __forceinline__ double three_mu() const { return 3. * mu; }
    __device__ __forceinline__ double hfac() const { return 1.0 / (1.0 + (h_ / (3.0 * mu))); }
};
template <bool FIELDS>
__device__ __forceinline__ auto cm_params(ArgsRef a, long long p0, int lane, bool live) {
    if constexpr (FIELDS)  // params: mu, kappa, y_0, h
        return CMLane{a.sc, field_value(0, p0, lane, live), field_value(1, p0, lane, live), field_value(2, p0, lane, live),
                      field_value(3, p0, lane, live)};
    else
        return CMUniform{a.sc};
}

// --- the two linear-elastic laws: the four distinct entries of the point's 6x6 matrix, {[i][i] (i < 3), [i][j] (i != j < 3),
//     [i][i] (i >= 3), the rest}.  LinearElasticityModel: elastic_tangent_full (fcamd_capi.cpp) from E, nu; comfe-rs
//     LinearElasticity3D: (2 mu) P_dev + (3 kappa) P_vol (comfe_projections) from mu, kappa.
struct ElasticEntries {
    double d[4];
};
__device__ __forceinline__ ElasticEntries le_entries(double E, double nu) {
    const double mu = E / (2.0 * (1.0 + nu));                  // lame()
    const double lam = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu));
    return ElasticEntries{{2.0 * mu + lam, lam, 2.0 * mu, 0.0}};
}
__device__ __forceinline__ ElasticEntries comfe_le_entries(double mu, double kappa) {
    // comfe_projections: pvol = s * (1/3), pdev = delta + pvol * -1.0 (s = 1 inside the 3x3 block, else 0)
    const double pv1 = 1.0 * (1.0 / 3.0), pv0 = 0.0 * (1.0 / 3.0);
    const double pd_dd = 1.0 + pv1 * -1.0, pd_od = 0.0 + pv1 * -1.0, pd_sh = 1.0 + pv0 * -1.0, pd_z = 0.0 + pv0 * -1.0;
    const double a = 2.0 * mu, b = 3.0 * kappa;
    return ElasticEntries{{a * pd_dd + b * pv1, a * pd_od + b * pv1, a * pd_sh + b * pv0, a * pd_z + b * pv0}};
}
// entry [i][j] of the point's matrix
__device__ __forceinline__ double elastic_entry(const double* d, int i, int j) {
    return (i < 3 && j < 3) ? (i == j ? d[0] : d[1]) : (i == j ? d[2] : d[3]);
}

}  // namespace fcamd
