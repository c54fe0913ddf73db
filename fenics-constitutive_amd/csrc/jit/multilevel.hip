// The aggregation multilevel preconditioner of the device solver (multilevel.py: MultilevelPreconditioner): z = M^-1 r over a
// hierarchy of aggregates with Galerkin coarse matrices, applied inside the conjugate gradients of conjugate_gradient.hip.  Read at
// run time and compiled with hiprtc behind the generated definitions FCAMD_CG_D (dofs per node), FCAMD_CG_PRECOND = 2 (the update
// kernel forms neither z nor rz) and FCAMD_CG_SLAB; the program holds the solver's five kernels and the five below.
//
// Every level is a block CSR matrix of D x D blocks (level 0: the values of the TangentMatrix in either format), so the products
// of every level are fcamd_cg_matvec_kernel (mode kQuiet) and the inverses of the nodes' own blocks fcamd_cg_inverse_kernel, with
// per-level arguments.  The kernels here, 256-thread blocks, grid-stride, a lane per scalar entry, all on one stream; every one
// returns at once when the status of the control block is not "running":
//
// Galerkin kernel: the values of level l + 1 from those of level l.  Coarse block K, entry (r, s):
//   f = 0.0;  f = f + value_l(k, r, s)  over the fine blocks k = fold[fold_ptr[K] .. fold_ptr[K + 1]), ascending
// with value_l(k, r, s) at dest_base[k] + r * dest_stride[k] + s on level 0 (the tables of the TangentMatrix: both formats give
// the same bits) and at D*D*k + D*r + s on the coarse levels.
// Restriction kernel: rc[D I + c] = 0.0;  rc = rc + d[D i + c]  over the members i of aggregate I, ascending; d = b or b - q.
// Prolongation kernel: x[D i + c] = x[D i + c] + xc[D agg[i] + c], skipped where the mask (level 0: the constrained dofs) is set.
// Smoothing kernel: t = 0.0;  t = t + inv[v][c][s] * d[D v + s], s ascending, d = b or b - q (every lane forms the D entries of its
// node in registers); x = t (plain), x = omega * t (first) or x = x + omega * t.
// Closing kernel: r . z by the ordered dot of conjugate_gradient.hip (same segments, tree and last-block reduction); in the start
// p = z, else rz_old = rz; rz = r . z; not rz > 0: status indefinite.
// No floating-point atomics, no MFMA; every product is rounded before its sum (-ffp-contract=off).
#pragma once
#include "conjugate_gradient.hip"

namespace fcamd_ml {
using namespace fcamd_cg;

// the only parameter of every kernel here; multilevel.py mirrors the layout
struct Args {
    const double* fine_values;    // Galerkin: the values of level l
    double* coarse_values;        // Galerkin: [n_coarse] the values of level l + 1, block CSR
    const int* fold_ptr;          // [coarse blocks + 1]
    const int* fold;              // [fine blocks] the fine blocks of every coarse block, ascending
    const long long* dest_base;   // level 0: [fine blocks]; null on the coarse levels
    const int* dest_stride;       // level 0: [fine blocks]
    const int* mem_ptr;           // [aggregates + 1]
    const int* members;           // [fine nodes] the members of every aggregate, ascending
    const int* agg;               // [fine nodes]
    const unsigned char* mask;    // prolongation: [n] or null
    const double* b;              // smoothing, restriction: the level's right-hand side
    const double* q;              // smoothing, restriction: K x (use_q)
    double* x;                    // smoothing, prolongation: the level's solution
    const double* xc;             // prolongation: the coarse solution
    double* rc;                   // restriction: the coarse right-hand side
    const double* inv;            // smoothing: [nodes][D][D]
    const double* r;              // closing
    const double* z;              // closing
    double* p;                    // closing (start)
    double* partials;             // closing: [nseg]
    Control* sc;
    double omega;
    long long n;                  // scalar entries of the level (D * nodes)
    long long n_coarse;           // Galerkin: scalar values of the coarse level; restriction: its scalar entries
    long long nseg;               // closing
    int first;                    // smoothing: x = omega * t
    int plain;                    // smoothing: x = t
    int use_q;                    // smoothing, restriction: d = b - q
    int start;                    // closing: p = z, rz_old stays
};

}  // namespace fcamd_ml

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_ml_galerkin_kernel(const fcamd_ml::Args a) {
    using namespace fcamd_ml;
    if (a.sc->status != kRunning) return;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < a.n_coarse; e += stride) {
        const long long kc = e / DD;
        const int rs = (int)(e - kc * DD);
        const int r = rs / D, s = rs - r * D;
        const int j1 = a.fold_ptr[kc + 1];
        double f = 0.0;
        for (int j = a.fold_ptr[kc]; j < j1; ++j) {
            const int k = a.fold[j];
            const long long at = a.dest_base ? a.dest_base[k] + (long long)r * a.dest_stride[k] + s : (long long)DD * k + D * r + s;
            f = f + a.fine_values[at];
        }
        a.coarse_values[e] = f;
    }
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_ml_restrict_kernel(const fcamd_ml::Args a) {
    using namespace fcamd_ml;
    if (a.sc->status != kRunning) return;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < a.n_coarse; e += stride) {
        const long long I = e / D;
        const int c = (int)(e - I * D);
        const int m1 = a.mem_ptr[I + 1];
        double rc = 0.0;
        for (int m = a.mem_ptr[I]; m < m1; ++m) {
            const long long g = (long long)D * a.members[m] + c;
            double d = a.b[g];
            if (a.use_q) d = d - a.q[g];
            rc = rc + d;
        }
        a.rc[e] = rc;
    }
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_ml_prolong_kernel(const fcamd_ml::Args a) {
    using namespace fcamd_ml;
    if (a.sc->status != kRunning) return;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < a.n; e += stride) {
        if (a.mask && a.mask[e]) continue;
        const long long i = e / D;
        const int c = (int)(e - i * D);
        a.x[e] = a.x[e] + a.xc[(long long)D * a.agg[i] + c];
    }
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_ml_smooth_kernel(const fcamd_ml::Args a) {
    using namespace fcamd_ml;
    if (a.sc->status != kRunning) return;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < a.n; e += stride) {
        const long long v = e / D;
        const double* m = a.inv + (long long)D * e;  // inv[v][c][.]
        double t = 0.0;
#pragma unroll
        for (int s = 0; s < D; ++s) {
            const long long g = v * D + s;
            double d = a.b[g];
            if (a.use_q) d = d - a.q[g];
            t = t + m[s] * d;
        }
        if (a.plain)
            a.x[e] = t;
        else if (a.first)
            a.x[e] = a.omega * t;
        else
            a.x[e] = a.x[e] + a.omega * t;
    }
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_ml_close_kernel(const fcamd_ml::Args a) {
    using namespace fcamd_ml;
    __shared__ double red[kBlock + 2];
    Control* sc = a.sc;
    if (sc->status != kRunning) return;
    const int t = (int)threadIdx.x;
    for (long long seg = blockIdx.x; seg < a.nseg; seg += gridDim.x) {
        double acc = 0.0;
#pragma unroll 1
        for (int i = 0; i < kPerLane; ++i) {
            const long long e = seg * kSeg + t + (long long)kBlock * i;
            if (e < a.n) {
                const double z = a.z[e];
                acc = acc + a.r[e] * z;
                if (a.start) a.p[e] = z;
            }
        }
        const double total = block_tree(acc, red, t);
        if (t == 0) a.partials[seg] = total;
    }
    if (last_block(sc, red, t)) {
        const double rz = final_sum(a.partials, a.nseg, red, t);
        if (t == 0) {
            if (!a.start) sc->rz_old = sc->rz;
            sc->rz = rz;
            if (!(rz > 0.0)) sc->status = kIndefinite;
        }
    }
}
