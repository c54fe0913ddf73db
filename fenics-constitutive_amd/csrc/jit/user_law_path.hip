// Kernel template of UserLaw.evaluate_path (userlaw.py): material points driven through a whole load path of S steps in one
// launch, the state of a tile's 64 points in registers across the steps.  Compiled behind the generated definitions that
// user_law_tile.h lists and
//   FCAMD_USER_PATH          1: explicit law (fcamd_user_point), 2: autodiff (fcamd_user_stress<T>), 3: implicit (start / residual /
//                            update; FCAMD_USER_UNKNOWNS, FCAMD_USER_IM_KJ, FCAMD_USER_IM_KT = 0 and FCAMD_USER_IM_SLOT as for
//                            user_law_implicit.hip, whose Newton loop is the point step)
//   FCAMD_PATH_NCTRL         F, the number of stress-controlled Mandel components (0: pure strain control)
//   FCAMD_PATH_CTRL          their indices, comma separated (only with F > 0)
//
// One step of one lane.  The row of the load path gives the Mandel strain increment de of the strain-controlled
// components and the total stress the controlled ones must reach; those start at de = 0.  Every evaluation builds the symmetric
// gradient g from de (diagonals copied, off-diagonal pairs de[c] / 2**0.5), eps = mandel_strain(g, factor) and runs the law's
// point step from the step's committed state, kept in registers next to the trial state: a strain-controlled step computes the
// bits of the evaluate kernel on that gradient.  A lane is converged when max_c |sigma_c - target_c| <= tol; otherwise, while
// fewer than max_iter updates have been made, de_free -= J^-1 r with J = d sigma_free / d eps_free (explicit laws: the entries of
// the D the point function returns; autodiff laws: the partials of one fcamd_user_stress<Dual<F>> pass seeded on the controlled
// components, which is also the evaluation) and the pivoted in-register LU of the implicit laws.  The wave evaluates until no
// lane updates; a lane that has finished keeps its de, so its last evaluation repeats its bits and no result depends on the
// other points of the wave.  The last evaluation is recorded and committed.  A lane whose point function returns non-zero there,
// or whose control loop does not converge, has failed: it keeps its committed state, its records are NaN from that step on and
// it takes no further part.
//
// Memory: the committed stress and history are read once per tile and written once; per step the kernel reads the load row
// (shared path: six wave-uniform doubles; per-point path: the step's contiguous 3 KiB run, requested one step ahead) and writes
// the records (48 B per point each; runs of 48 B per point stay 16-byte aligned).  Full tiles move 16-byte non-temporal chunks
// through the wave's LDS region, the ragged last tile guarded 8-byte accesses.
#pragma once
#if FCAMD_USER_PATH == 3
#include "user_law_implicit.hip"
#else
#include "user_law_implicit.h"  // dense_solve, Dual
#include "user_law_tile.h"
#endif

namespace fcamd_user {

constexpr int kF = FCAMD_PATH_NCTRL;
constexpr int kFs = kF > 0 ? kF : 1;  // array extents
static_assert(kF >= 0 && kF <= 6, "evaluate_path: 0 to 6 stress-controlled components");
static_assert(FCAMD_USER_PATH != 3 || kF == 0, "evaluate_path: implicit laws are strain-controlled");
#if FCAMD_PATH_NCTRL > 0
__device__ constexpr int kCtrl[kF] = {FCAMD_PATH_CTRL};
#else
__device__ constexpr int kCtrl[1] = {0};
#endif

#if FCAMD_USER_PATH == 1
using PathHistory = UserHistory;
#else
using PathHistory = UserHistoryT<double>;
#endif

// the only kernel parameter; userlaw.py mirrors the layout (_path_args_type)
struct PathArgs {
    const double* load;      // [S, 6] (one path for all points) or [S, n, 6]
    const double* del_t;     // [S]; step k runs at t_k = t0 + del_t[0] + ... + del_t[k - 1], summed in this order
    double* stress;          // [6 n] committed stress: in before the path, out after the last step a point completed
    double* h[kNH];          // history fields, likewise
    double* stress_path;     // [S, n, 6] or nullptr
    double* strain_path;     // [S, n, 6] or nullptr
    int* failed;             // [n]: the first step the point failed, or -1
    long long n;             // points
    long long steps;         // S
    long long per_point;     // load has a row per point and step
    long long max_iter;      // of the control loop
    double t0;               // the time before the first step
    double tol;              // of the control loop
    double factor;           // Mandel factor of the off-diagonal strains (the Python laws')
    double sq2;              // 2**0.5: the off-diagonal gradient entries are de[c] / sq2
    double params[kMaxParams];
#ifdef FCAMD_USER_FIELDS
    const double* fields[kNF];
#endif
};

// the symmetric gradient whose Mandel strain increment is de (tests/material_point.py: grad_from_mandel_strain)
__device__ __forceinline__ void path_gradient(const double (&de)[6], double sq2, double (&g)[9]) {
    g[0] = de[0];
    g[4] = de[1];
    g[8] = de[2];
    g[1] = g[3] = de[3] / sq2;
    g[2] = g[6] = de[4] / sq2;
    g[5] = g[7] = de[5] / sq2;
}

// one evaluation of the lane's point from the committed state (s, h) at the increment de: trial state (st, ht), the return code,
// and J = d sigma_ctrl / d eps_ctrl (F x F, row-major; F > 0 only)
__device__ __forceinline__ int path_point(const PathArgs& a, const UserParams& p, double t, double del_t, const double (&de)[6],
                                          const double (&s)[6], const PathHistory& h, bool active, double (&st)[6], PathHistory& ht,
                                          double (&J)[kFs * kFs]) {
    double g[9], e[6];
    path_gradient(de, a.sq2, g);
    mandel_strain(g, a.factor, e);
#if FCAMD_USER_PATH == 1
#pragma unroll
    for (int i = 0; i < 6; ++i) st[i] = s[i];
    ht = h;
    double D[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) D[i] = 0.0;
    const int rc = fcamd_user_point(p, t, del_t, g, e, st, D, ht);
    if constexpr (kF > 0) {
#pragma unroll
        for (int i = 0; i < kF; ++i)
#pragma unroll
            for (int j = 0; j < kF; ++j) J[kF * i + j] = D[6 * kCtrl[i] + kCtrl[j]];
    }
    return rc;
#elif FCAMD_USER_PATH == 2
    if constexpr (kF == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) st[i] = s[i];
        ht = h;
        return fcamd_user_stress<double>(p, t, del_t, e, st, ht);
    } else {
        // the Mandel strain of component c depends on de[c] alone and with slope one (diagonals: copied; off-diagonals:
        // factor * (x / sq2 + x / sq2), the law's own strain measure): the seeds sit on eps
        using T = Dual<kFs>;
        T te[6], ts[6];
        UserHistoryT<T> th;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            te[j] = T(e[j]);
            ts[j] = T(s[j]);
        }
#pragma unroll
        for (int k = 0; k < kF; ++k) te[kCtrl[k]].d[k] = 1.0;
#define FCAMD_X(k, name, dim) \
    _Pragma("unroll") for (int i = 0; i < (dim); ++i) th.name[i] = T(h.name[i]);
        FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
        const int rc = fcamd_user_stress<T>(p, t, del_t, te, ts, th);
#pragma unroll
        for (int i = 0; i < 6; ++i) st[i] = ts[i].v;
#define FCAMD_X(k, name, dim) \
    _Pragma("unroll") for (int i = 0; i < (dim); ++i) ht.name[i] = th.name[i].v;
        FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
#pragma unroll
        for (int i = 0; i < kF; ++i)
#pragma unroll
            for (int j = 0; j < kF; ++j) J[kF * i + j] = ts[kCtrl[i]].d[j];
        return rc;
    }
#else
    // the stress-only point step of user_law_implicit.hip; a lane that has failed does not hold the wave's Newton loop
    double x[kN];
    bool solved;
    const bool failed = user_newton(p, t, del_t, e, s, h, active, (int)a.params[FCAMD_USER_IM_SLOT], a.params[FCAMD_USER_IM_SLOT + 1],
                                    x, solved);
#pragma unroll
    for (int i = 0; i < 6; ++i) st[i] = s[i];
    ht = h;
    fcamd_user_update<double>(p, t, del_t, e, x, st, ht);
    return failed ? 1 : 0;
#endif
}

// one 64-point tile (FULL) or the ragged last one (npts < 64) through all steps
template <bool FULL, bool NT>
__device__ __forceinline__ void path_tile(const PathArgs& a, const UserParams& p, double* region, long long p0, int npts, int lane) {
    const bool live = FULL || lane < npts;
    double s[6];
    PathHistory h;
    {
        // every load of the tile is issued before the first transposition
        Chunks<6> cs;
        tile_load<6, FULL, NT>(cs, a.stress + p0 * 6, npts * 6, lane);
#define FCAMD_X(k, name, dim) \
    Chunks<dim> c_##name;     \
    tile_load<dim, FULL, NT>(c_##name, a.h[k] + p0 * (dim), npts * (dim), lane);
        FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
        transpose_in<6>(cs, region, lane, s);
#define FCAMD_X(k, name, dim) user_in<dim>(c_##name, region, lane, h.name);
        FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
    }
    const bool per_point = a.per_point != 0;  // uniform
    const int max_iter = (int)a.max_iter;
    const double nan = __builtin_nan("");
    int failed_at = -1;
    double t = a.t0;  // t_k: the sequential double sum a loop of evaluate calls accumulates on the host
    Chunks<6> next;  // per-point path: the load row of the coming step
    if (per_point) tile_load<6, FULL, NT>(next, a.load + p0 * 6, npts * 6, lane);
#pragma nounroll
    for (long long k = 0; k < a.steps; ++k) {
        const double del_t = a.del_t[k];
        double de[6];
        if (per_point) {
            transpose_in<6>(next, region, lane, de);
            if (k + 1 < a.steps) tile_load<6, FULL, NT>(next, a.load + ((k + 1) * a.n + p0) * 6, npts * 6, lane);
        } else {
#pragma unroll
            for (int c = 0; c < 6; ++c) de[c] = a.load[k * 6 + c];
        }
        double target[kFs];
        if constexpr (kF > 0) {
#pragma unroll
            for (int i = 0; i < kF; ++i) {
                target[i] = de[kCtrl[i]];
                de[kCtrl[i]] = 0.0;
            }
        }
        const bool active = live && failed_at < 0;
        double st[6];
        PathHistory ht;
        double J[kFs * kFs];
        int rc = path_point(a, p, t, del_t, de, s, h, active, st, ht, J);
        bool control_failed = false;
        if constexpr (kF > 0) {
            for (int it = 0;; ++it) {
                double r[kFs];
                bool conv = true;
#pragma unroll
                for (int i = 0; i < kF; ++i) {
                    r[i] = st[kCtrl[i]] - target[i];
                    conv = conv && __builtin_fabs(r[i]) <= a.tol;  // false for a NaN
                }
                bool step = active && !control_failed && !conv && it < max_iter;  // a singular J has ended the lane's loop
                control_failed = control_failed || (active && !conv && !step);
                if (__builtin_amdgcn_ballot_w64(step) == 0ull) break;  // uniform
                const bool ok = dense_solve<kFs, 1>(J, r);
                control_failed = control_failed || (step && !ok);
                step = step && ok;
#pragma unroll
                for (int i = 0; i < kF; ++i) de[kCtrl[i]] = step ? de[kCtrl[i]] - r[i] : de[kCtrl[i]];  // a finished lane keeps its de
                if (__builtin_amdgcn_ballot_w64(step) == 0ull) break;  // nobody moved: the last evaluation stands
                rc = path_point(a, p, t, del_t, de, s, h, active, st, ht, J);
            }
        }
        const bool step_failed = active && (rc != 0 || control_failed);
        const bool commit = active && !step_failed;
        failed_at = step_failed ? (int)k : failed_at;
        if (commit) {
#pragma unroll
            for (int i = 0; i < 6; ++i) s[i] = st[i];
            h = ht;
        }
        if (a.stress_path != nullptr) {
            double rec[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) rec[i] = commit ? st[i] : nan;
            transpose_out<6, FULL, NT>(rec, region, lane, a.stress_path + (k * a.n + p0) * 6, npts * 6);
        }
        if (a.strain_path != nullptr) {
            double rec[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) rec[i] = commit ? de[i] : nan;
            transpose_out<6, FULL, NT>(rec, region, lane, a.strain_path + (k * a.n + p0) * 6, npts * 6);
        }
        t = t + del_t;
    }
    transpose_out<6, FULL, NT>(s, region, lane, a.stress + p0 * 6, npts * 6);
#define FCAMD_X(k, name, dim) user_out<dim, FULL, NT>(h.name, region, lane, a.h[k] + p0 * (dim), npts * (dim));
    FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
    if (live) a.failed[p0 + lane] = failed_at;
}

#ifdef FCAMD_USER_FIELDS
template <bool FULL, bool NT>
__device__ __forceinline__ UserParams path_lane_params(const PathArgs& a, long long p0, int npts, int lane) {
    UserFieldValues f;
    user_fields_load<FULL, NT>(a.fields, p0, npts, lane, f);
    return fcamd_user_params(a.params, f);
}
#endif

}  // namespace fcamd_user

extern "C" __global__ void __launch_bounds__(fcamd::kBlock, FCAMD_USER_WAVES) fcamd_user_law_path_kernel(const fcamd_user::PathArgs a) {
    using namespace fcamd_user;
    __shared__ __attribute__((aligned(16))) double scratch[kWavesPerBlock][kUserRegion];
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    double* region = scratch[wave];
#ifndef FCAMD_USER_FIELDS
    const UserParams p = fcamd_user_params(a.params);
#endif
    const long long nfull = a.n / kWave;
    const long long wstride = (long long)gridDim.x * kWavesPerBlock;
    long long tile = (long long)blockIdx.x * kWavesPerBlock + wave;
#ifdef FCAMD_USER_FIELDS  // UserParams per lane and tile
    for (; tile < nfull; tile += wstride) path_tile<true, true>(a, path_lane_params<true, true>(a, tile * kWave, kWave, lane), region, tile * kWave, kWave, lane);
    if (tile == nfull && a.n > nfull * kWave) {
        const int npts = (int)(a.n - tile * kWave);
        path_tile<false, false>(a, path_lane_params<false, false>(a, tile * kWave, npts, lane), region, tile * kWave, npts, lane);
    }
#else
    for (; tile < nfull; tile += wstride) path_tile<true, true>(a, p, region, tile * kWave, kWave, lane);
    if (tile == nfull && a.n > nfull * kWave) path_tile<false, false>(a, p, region, tile * kWave, (int)(a.n - tile * kWave), lane);
#endif
}
