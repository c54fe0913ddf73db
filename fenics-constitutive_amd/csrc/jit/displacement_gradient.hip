// The gradient producer (gradient.py: DisplacementGradient): the displacement-gradient increment of every quadrature point from a
// nodal displacement increment, written as the very array the law kernels read.  Read at run time and compiled with hiprtc
// behind the generated definitions:
//   FCAMD_DG_D        geometric dimension: 1, 2 or 3
//   FCAMD_DG_A        nodes per cell
//   FCAMD_DG_Q        quadrature points per cell
//   FCAMD_DG_AFFINE   1: jinv[C][D][D], one inverse Jacobian per cell; 0: jinv[C][Q][D][D], one per point
//   FCAMD_DG_NABLA    1: out[D*D*p + D*r + x] = d u_x / d x_r (nabla_grad, the layout of include/fcamd.h); 0: d u_r / d x_x
//   FCAMD_DG_WAVES    waves per SIMD the register budget is cut for
//
// Shape of the law kernels (user_law_tile.h): 256-thread blocks, one wave per 64-point tile, one lane per point, a grid-stride
// loop over the tiles, the ragged last tile separate.  Point p = Q*c + q is point q of cell c.  With -ffp-contract=off the
// arithmetic of a point is exactly, in this order,
//   R[r][k] = 0.0;  for a = 0..A-1:  R[r][k] = R[r][k] + du[D*dofmap[c][a] + r] * ref[q][a][k]
//   G[r][x] = 0.0;  for k = 0..D-1:  G[r][x] = G[r][x] + R[r][k] * jinv[c(,q)][k][x]
//
// Memory: ref (Q*A*D doubles, one table for the mesh) is staged once per block into LDS; per-point jinv rows arrive as the
// coalesced 16-byte chunks of tile_load / transpose_in, per-cell ones are gathered (the Q lanes of a cell ask for one address);
// du and dofmap are gathered per lane (the nodal vector is small and stays in the L2 / Infinity Cache); the gradient leaves through
// transpose_out as the 16-byte non-temporal stream the law kernels then read.  Dead lanes of the ragged tile form no cell index
// and load nothing.  Index arithmetic is 64-bit.
#pragma once
#include "tile_io.h"

namespace fcamd_dg {
using namespace fcamd;

constexpr int D = FCAMD_DG_D, A = FCAMD_DG_A, Q = FCAMD_DG_Q, DD = D * D;
constexpr bool kAffine = FCAMD_DG_AFFINE != 0, kNabla = FCAMD_DG_NABLA != 0;
constexpr int kTable = Q * A * D;
constexpr int kTablePad = (kTable + 1) & ~1;  // the regions behind the table stay on the 16-byte grid
constexpr int kRegion = kWave * DD;           // the wave's transposition region: 64 points x D*D doubles
constexpr int kUnrollA = 2;  // more keeps more gathered values in flight than 64 VGPRs hold (D = 3)
// gradient.py (lds_bytes, LDS_CAP) refuses such a shape before it gets here
static_assert((kTablePad + kWavesPerBlock * kRegion) * 8 <= 64 * 1024, "reference table too large for the LDS of a block");
static_assert(D >= 1 && D <= 3 && A >= 1 && Q >= 1, "shape");

// the only kernel parameter; gradient.py mirrors the layout (GradArgs)
struct GradArgs {
    const double* du;    // [D n_nodes], component r of node v at D*v + r
    const int* dofmap;   // [C][A] node numbers
    const double* ref;   // [Q][A][D] reference-element basis gradients at the quadrature points
    const double* jinv;  // [C][D][D] or [C][Q][D][D]: jinv[..][k][x] = d xi_k / d x_x
    double* out;         // [D*D n]
    long long n;         // points = Q * cells
};

// one 64-point tile (FULL) or the ragged last one (npts < 64) starting at point p0
template <bool FULL, bool NT>
__device__ __forceinline__ void grad_tile(const GradArgs& a, const double* table, double* region, long long p0, int npts, int lane) {
    const bool live = FULL || lane < npts;
    long long c = 0;
    int q = 0;
    if (live) {
        const long long p = p0 + lane;
        c = p / Q;
        q = (int)(p - c * Q);
    }
    double g[DD];
#pragma unroll
    for (int i = 0; i < DD; ++i) g[i] = 0.0;
    double R[D][D];
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
        for (int k = 0; k < D; ++k) R[r][k] = 0.0;
    if (live) {
        const int* row = a.dofmap + c * A;
        const double* t = table + q * (A * D);
#pragma unroll(kUnrollA)
        for (int b = 0; b < A; ++b) {
            const long long v = (long long)row[b] * D;
#pragma unroll
            for (int r = 0; r < D; ++r) {
                const double u = a.du[v + r];
#pragma unroll
                for (int k = 0; k < D; ++k) R[r][k] = R[r][k] + u * t[b * D + k];
            }
        }
    }
    double J[DD];
    if constexpr (kAffine) {
#pragma unroll
        for (int i = 0; i < DD; ++i) J[i] = live ? a.jinv[c * DD + i] : 0.0;
    } else {  // issued behind the gather: the chunks held across it would not fit the budget of 8 waves per SIMD
        Chunks<DD> cj;
        tile_load<DD, FULL, NT>(cj, a.jinv + p0 * DD, npts * DD, lane);
        transpose_in<DD>(cj, region, lane, J);
    }
    if (live) {
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int x = 0; x < D; ++x) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) s = s + R[r][k] * J[D * k + x];
                g[kNabla ? D * x + r : D * r + x] = s;
            }
    }
    transpose_out<DD, FULL, NT>(g, region, lane, a.out + p0 * DD, npts * DD);
}

}  // namespace fcamd_dg

extern "C" __global__ void __launch_bounds__(fcamd::kBlock, FCAMD_DG_WAVES) fcamd_displacement_gradient_kernel(const fcamd_dg::GradArgs a) {
    using namespace fcamd_dg;
    __shared__ __attribute__((aligned(16))) double table[kTablePad];
    __shared__ __attribute__((aligned(16))) double scratch[kWavesPerBlock][kRegion];
    for (int i = (int)threadIdx.x; i < kTable; i += kBlock) table[i] = a.ref[i];
    __syncthreads();
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    double* region = scratch[wave];
    const long long nfull = a.n / kWave;
    const long long wstride = (long long)gridDim.x * kWavesPerBlock;
    long long tile = (long long)blockIdx.x * kWavesPerBlock + wave;
    for (; tile < nfull; tile += wstride) grad_tile<true, true>(a, table, region, tile * kWave, kWave, lane);
    if (tile == nfull && a.n > nfull * kWave) grad_tile<false, false>(a, table, region, tile * kWave, (int)(a.n - tile * kWave), lane);
}
