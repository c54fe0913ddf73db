// LinearElasticityModel (models/linear_elasticity_model.py:26-45) and comfe-rs LinearElasticity3D (linear_elasticity.rs:42-75).
// Part of the device code of libfcamd (translation unit: ../fcamd_kernels.hip, which holds the kernels and launchers).
#pragma once
#include "tile_io.h"
#include "tangent_writers.h"
#include "wrapped_io.h"
#include "param_source.h"

namespace fcamd {

// ---------------------------------------------------------------------------------------
// tile bodies, one per law.  `region` is the wave's LDS scratch, `T` the staged tables.
// ---------------------------------------------------------------------------------------

// the point's own 6x6 matrix from its four distinct entries (param_source.h), in registers
__device__ __forceinline__ void elastic_matrix(const ElasticEntries& d, double (&M)[36]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) M[6 * i + j] = elastic_entry(d.d, i, j);
}

// per-point parameters (FIELDS): the four entries are published for the tangent writer once the tile's stress is stored
template <bool FULL, bool NT>
__device__ __forceinline__ void tangent_elastic_fields(const StressBases& sb, const ElasticEntries& d, double* region, long long p0,
                                                       int npts, int lane) {
    if (!sb.tan) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) region[10 * lane + k] = d.d[k];
    wave_sync();
    tangent_elastic_points<FULL, NT>(region, sb.tan, p0, npts, lane);
    wave_sync();
}

// --- LinearElasticityModel: sigma += d_eps @ D ; tangent = tile(D) ----------------------
// FIELDS: E and / or nu per point (evaluate_fields_kernel: field_args()), D built per lane as elastic_tangent_full builds it
template <bool IDX, bool FULL, bool NT, bool FIELDS = false>
__device__ __forceinline__ void tile_linear_elasticity(ArgsRef a, const StressBases& sb, const Tables* T,
                                                       double* region, int* rows_lds, long long p0,
                                                       int npts, int lane, int r0) {
    Chunks<9> cg;
    StressRows<IDX, FULL, NT> sr;
    tile_load<9, FULL, NT>(cg, a.grad + p0 * 9, npts * 9, lane);
    sr.load(a, sb, p0, npts, lane, rows_lds);
    if constexpr (FIELDS) {
        const bool live = FULL || lane < npts;
        const ElasticEntries d = le_entries(field_value(0, p0, lane, live), field_value(1, p0, lane, live));
        double g[9], s[6], e[6], ds[6], D[36];
        transpose_in<9>(cg, region, lane, g);
        sr.get(region, lane, s);
        mandel_strain(g, a.sc.s[0], e);
        elastic_matrix(d, D);
        row_times_matrix_fma(e, D, ds);
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i] = s[i] + ds[i];
        sr.put(sb, region, lane, s, p0, npts, rows_lds);
        tangent_elastic_fields<FULL, NT>(sb, d, region, p0, npts, lane);
        return;
    }
    // the constant tangent does not depend on the loads: stream it while they are in flight
    if (sb.tan) {
        if constexpr (IDX) wave_sync();  // rows_lds visible to all lanes
        tangent_const<IDX, FULL, NT>(T->c, sb.tan, p0, rows_lds, npts, lane, r0);
    }
    double g[9], s[6], e[6], ds[6];
    transpose_in<9>(cg, region, lane, g);
    sr.get(region, lane, s);
    mandel_strain(g, a.sc.s[0], e);
    row_times_matrix_fma(e, T->a, ds);
#pragma unroll
    for (int i = 0; i < 6; ++i) s[i] = s[i] + ds[i];
    sr.put(sb, region, lane, s, p0, npts, rows_lds);
}

// --- comfe-rs LinearElasticity3D: sigma += C . d_eps (column axpy, no FMA) ---------------
// FIELDS: mu and / or kappa per point, C built per lane as fill_constants builds it
template <bool IDX, bool FULL, bool NT, bool FIELDS = false>
__device__ __forceinline__ void tile_comfe_le(ArgsRef a, const StressBases& sb, const Tables* T, double* region,
                                              int* rows_lds, long long p0, int npts, int lane, int r0) {
    Chunks<9> cg;
    StressRows<IDX, FULL, NT> sr;
    tile_load<9, FULL, NT>(cg, a.grad + p0 * 9, npts * 9, lane);
    sr.load(a, sb, p0, npts, lane, rows_lds);
    if constexpr (FIELDS) {
        const bool live = FULL || lane < npts;
        const ElasticEntries d = comfe_le_entries(field_value(0, p0, lane, live), field_value(1, p0, lane, live));
        double g[9], s[6], e[6], C[36];
        transpose_in<9>(cg, region, lane, g);
        sr.get(region, lane, s);
        mandel_strain(g, a.sc.s[0], e);
        elastic_matrix(d, C);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double acc = C[6 * i] * e[0];
#pragma unroll
            for (int j = 1; j < 6; ++j) acc = C[6 * i + j] * e[j] + acc;
            s[i] = s[i] + acc;
        }
        sr.put(sb, region, lane, s, p0, npts, rows_lds);
        tangent_elastic_fields<FULL, NT>(sb, d, region, p0, npts, lane);
        return;
    }
    if (sb.tan) {
        if constexpr (IDX) wave_sync();  // rows_lds visible to all lanes
        tangent_const<IDX, FULL, NT>(T->c, sb.tan, p0, rows_lds, npts, lane, r0);
    }
    double g[9], s[6], e[6];
    transpose_in<9>(cg, region, lane, g);
    sr.get(region, lane, s);
    mandel_strain(g, a.sc.s[0], e);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double acc = T->a[6 * i] * e[0];
#pragma unroll
        for (int j = 1; j < 6; ++j) acc = T->a[6 * i + j] * e[j] + acc;
        s[i] = s[i] + acc;
    }
    sr.put(sb, region, lane, s, p0, npts, rows_lds);
}

// LinearElasticityModel behind the wrappers (what the reference's own tests wrap, test_elasticity.py:206,278)
template <int WRAP, bool FULL, bool NT>
__device__ __forceinline__ void tile_linear_elasticity_wrapped(ArgsRef a, const Tables* T, double* region,
                                                               long long p0, int npts, int lane) {
    if (a.tangent) wrapped_tangent_const<WRAP, FULL, NT>(a, T->c, p0, npts, lane);
    double g[9], s[6], e[6], ds[6];
    wrapped_load<WRAP, FULL, NT>(a, region, p0, npts, lane, g, s);
    mandel_strain(g, a.sc.s[0], e);
    row_times_matrix_fma(e, T->a, ds);
#pragma unroll
    for (int i = 0; i < 6; ++i) s[i] = s[i] + ds[i];
    wrapped_store_stress<WRAP, FULL, NT>(a, region, p0, npts, lane, s);
}

}  // namespace fcamd
