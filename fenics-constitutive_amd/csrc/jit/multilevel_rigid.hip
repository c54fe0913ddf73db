// The rigid-body coarse space of the multilevel preconditioner (multilevel.py: MultilevelPreconditioner(coarse_space="rigid_body")):
// a coarse node carries Dc = G + R dofs, G translations and R rotations (G the space dimension: R = 3 in 3-D, 1 in 2-D).  Read at
// run time and compiled with hiprtc behind the definitions of multilevel.hip and FCAMD_ML_GDIM = G.  Two programs per object:
//   the fine program    FCAMD_CG_D = G:   level 0; the transfer kernels below are those of the pair (G, Dc)
//   the coarse program  FCAMD_CG_D = Dc:  every level l >= 1 (products, inverses, smoothing on Dc x Dc blocks); the pair (Dc, Dc)
// In both, Df = FCAMD_CG_D is the dofs per node of the FINE level of a transfer.
//
// Every node i of a level has the offset o_i = x_i - x_agg(i) from its aggregate's position (multilevel.py forms both on the host).
// B(o) is the G x R matrix of theta -> theta x o:  3-D  [[0, oz, -oy], [-oz, 0, ox], [oy, -ox, 0]],  2-D  [-oy, ox]^T  (a minus is a
// negation of the offset's entry, the zeros are +0.0).  The prolongation block of node i is
//   P_i = [I_G  B(o_i)]  (G x Dc, from level 0)      P_i = [[I_G, B(o_i)], [0, I_R]]  (Dc x Dc, from a level l >= 1)
// formed in registers, entry by entry, from the G doubles of o_i; nothing of P is stored.  All of P's entries take part in the
// sums below, its zeros and ones too (a product with 0.0 or 1.0 is a product).
//
// Three kernels, 256-thread blocks, grid-stride, a lane per scalar entry of the destination; every one returns at once when the
// status of the control block is not "running":
//
// Galerkin kernel: coarse block K = (I, J), entry (r, s), 0 <= r, s < Dc:
//   f = 0.0;  over the fine blocks k = fold[fold_ptr[K] .. fold_ptr[K + 1]), ascending, k = (i, j) = (block_row[k], indices[k]):
//     t = 0.0;  for a = 0 .. Df - 1 ascending:
//       u = 0.0;  u = u + value(k, a, b) * P_j[b][s],  b = 0 .. Df - 1 ascending
//       t = t + P_i[a][r] * u
//     f = f + t
//   value(k, a, b) at dest_base[k] + a * dest_stride[k] + b on level 0 (both formats: the same bits), at Df*Df*k + Df*a + b else.
// Restriction kernel: aggregate I, entry c, 0 <= c < Dc:
//   rc = 0.0;  over the members i of I, ascending:  t = 0.0;  t = t + P_i[a][c] * d[Df i + a],  a ascending;  rc = rc + t
//   d = b or b - q (formed here).
// Prolongation kernel: node i, entry r, 0 <= r < Df, skipped where the mask (level 0: the constrained dofs) is set:
//   t = 0.0;  t = t + P_i[r][c] * xc[Dc agg[i] + c],  c = 0 .. Dc - 1 ascending;  x[Df i + r] = x[Df i + r] + t
// No floating-point atomics, no MFMA; every product is rounded before its sum (-ffp-contract=off).
#pragma once
#include "multilevel.hip"

namespace fcamd_mr {
using namespace fcamd_cg;

constexpr int G = FCAMD_ML_GDIM;       // the space dimension
constexpr int R = G == 3 ? 3 : 1;      // rotations
constexpr int Dc = G + R;              // dofs of a coarse node
constexpr int Df = D;                  // dofs of a node of the fine level of the pair
static_assert(G == 2 || G == 3, "the rigid-body coarse space is for 2 and 3 dimensions");
static_assert(Df == G || Df == Dc, "the program's block size is the fine or the coarse one");

// the only parameter of the three kernels; multilevel.py mirrors the layout
struct Args {
    const double* fine_values;    // Galerkin: the values of level l
    double* coarse_values;        // Galerkin: [n_coarse] the values of level l + 1, block CSR of Dc x Dc blocks
    const int* fold_ptr;          // [coarse blocks + 1]
    const int* fold;              // [fine blocks] the fine blocks of every coarse block, ascending
    const long long* dest_base;   // level 0: [fine blocks]; null on the coarse levels
    const int* dest_stride;       // level 0: [fine blocks]
    const int* block_row;         // Galerkin: [fine blocks] the row node of every fine block
    const int* indices;           // Galerkin: [fine blocks] its column node
    const double* offsets;        // [fine nodes][G]
    const int* mem_ptr;           // [aggregates + 1]
    const int* members;           // [fine nodes] the members of every aggregate, ascending
    const int* agg;               // [fine nodes]
    const unsigned char* mask;    // prolongation: [n] or null
    const double* b;              // restriction: the fine level's right-hand side
    const double* q;              // restriction: K x (use_q)
    double* x;                    // prolongation: the fine level's solution
    const double* xc;             // prolongation: the coarse solution
    double* rc;                   // restriction: the coarse right-hand side
    Control* sc;
    long long n;                  // prolongation: scalar entries of the fine level (Df * nodes)
    long long n_coarse;           // Galerkin: scalar values of the coarse level; restriction: its scalar entries
    int use_q;                    // restriction: d = b - q
    int pad;
};

struct Offset {
    double x, y, z;
};

__device__ __forceinline__ Offset offset_of(const double* offsets, long long node) {
    const double* o = offsets + (long long)G * node;
    Offset v;
    v.x = o[0];
    v.y = o[1];
    v.z = G == 3 ? o[G - 1] : 0.0;
    return v;
}

// P[a][c], 0 <= a < Df, 0 <= c < Dc (selects on values: no array, so a run-time a or c costs no scratch)
__device__ __forceinline__ double p_entry(const Offset& o, int a, int c) {
    if (a >= G || c < G) return a == c ? 1.0 : 0.0;
    const int t = c - G;
    if constexpr (G == 2) {
        return a == 0 ? -o.y : o.x;
    } else {
        if (a == 0) return t == 0 ? 0.0 : (t == 1 ? o.z : -o.y);
        if (a == 1) return t == 0 ? -o.z : (t == 1 ? 0.0 : o.x);
        return t == 0 ? o.y : (t == 1 ? -o.x : 0.0);
    }
}

}  // namespace fcamd_mr

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_mr_galerkin_kernel(const fcamd_mr::Args a) {
    using namespace fcamd_mr;
    if (a.sc->status != kRunning) return;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < a.n_coarse; e += stride) {
        const long long kc = e / (Dc * Dc);
        const int rs = (int)(e - kc * (Dc * Dc));
        const int r = rs / Dc, s = rs - r * Dc;
        const int j1 = a.fold_ptr[kc + 1];
        double f = 0.0;
        for (int j = a.fold_ptr[kc]; j < j1; ++j) {
            const int k = a.fold[j];
            const Offset oi = offset_of(a.offsets, a.block_row[k]), oj = offset_of(a.offsets, a.indices[k]);
            const long long at = a.dest_base ? a.dest_base[k] : (long long)DD * k;
            const long long rstride = a.dest_base ? a.dest_stride[k] : Df;
            double t = 0.0;
#pragma unroll
            for (int ar = 0; ar < Df; ++ar) {
                double u = 0.0;
#pragma unroll
                for (int bc = 0; bc < Df; ++bc) u = u + a.fine_values[at + ar * rstride + bc] * p_entry(oj, bc, s);
                t = t + p_entry(oi, ar, r) * u;
            }
            f = f + t;
        }
        a.coarse_values[e] = f;
    }
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_mr_restrict_kernel(const fcamd_mr::Args a) {
    using namespace fcamd_mr;
    if (a.sc->status != kRunning) return;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < a.n_coarse; e += stride) {
        const long long I = e / Dc;
        const int c = (int)(e - I * Dc);
        const int m1 = a.mem_ptr[I + 1];
        double rc = 0.0;
        for (int m = a.mem_ptr[I]; m < m1; ++m) {
            const long long i = a.members[m];
            const Offset o = offset_of(a.offsets, i);
            double t = 0.0;
#pragma unroll
            for (int ar = 0; ar < Df; ++ar) {
                const long long g = (long long)Df * i + ar;
                double d = a.b[g];
                if (a.use_q) d = d - a.q[g];
                t = t + p_entry(o, ar, c) * d;
            }
            rc = rc + t;
        }
        a.rc[e] = rc;
    }
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_mr_prolong_kernel(const fcamd_mr::Args a) {
    using namespace fcamd_mr;
    if (a.sc->status != kRunning) return;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < a.n; e += stride) {
        if (a.mask && a.mask[e]) continue;
        const long long i = e / Df;
        const int r = (int)(e - i * Df);
        const Offset o = offset_of(a.offsets, i);
        const double* xc = a.xc + (long long)Dc * a.agg[i];
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < Dc; ++c) t = t + p_entry(o, r, c) * xc[c];
        a.x[e] = a.x[e] + t;
    }
}
