// The transpose of the gradient producer (force.py: InternalForce): nodal internal forces f = sum_p B_p^T sigma_p w_p from the
// stress of every quadrature point, and the tangent action y = sum_p B_p^T C_p B_p v w_p from the tangent and the gradient of v.
// Read at run time and compiled with hiprtc behind the generated definitions:
//   FCAMD_IF_D           geometric dimension: 1, 2 or 3 (the stress has S = 1, 4 or 6 Mandel components)
//   FCAMD_IF_A           nodes per cell
//   FCAMD_IF_Q           quadrature points per cell (at most 64)
//   FCAMD_IF_AFFINE      1: jinv[C][D][D], one inverse Jacobian per cell; 0: jinv[C][Q][D][D], one per point
//   FCAMD_IF_NABLA       layout of the gradient the tangent action reads: 1: grad[D*D*p + D*r + x] = d v_x / d x_r; 0: d v_r / d x_x
//   FCAMD_IF_SOURCE      0: src is the stress [S n]; 1: src is the tangent [S*S n], s = C e formed in registers
//   FCAMD_IF_ACCUMULATE  1: the node sum starts from out's value; 0: from 0.0
//   FCAMD_IF_WAVES       waves per SIMD the register budget of the element kernel is cut for
//
// Two kernels, launched one behind the other on one stream.
//
// Element kernel: 256-thread blocks, one wave per tile, a grid-stride loop over the tiles, the short last tile separate
// (user_law_tile.h).  A tile is W = 64/Q whole cells (one less where W*Q*D*D would be odd: every tile base of stress, jinv and
// gradient then stays on the 16-byte grid), one lane per point, so no cell straddles a wave.  With -ffp-contract=off the arithmetic
// is exactly, in this order (H the double of sqrt(0.5)),
//   T[i][i] = s[i];  T[i][j] = T[j][i] = s[3 + m] * H   for the m-th pair of (0,1), (0,2), (1,2)
//   tangent action:  e = (G00, G11, G22, H*(G01+G10), H*(G02+G20), H*(G12+G21));  s[i] = 0.0;  s[i] = s[i] + C[i][j] * e[j], j ascending
//   fe[c][a][r] = 0.0;  for q = 0..Q-1:
//     g[x] = 0.0;  g[x] = g[x] + ref[q][a][k] * jinv[c(,q)][k][x], k ascending
//     t    = 0.0;  t    = t + T[r][x] * g[x], x ascending
//     fe[c][a][r] = fe[c][a][r] + t * weights[c][q]
// Every lane forms t * w of its point for D nodes at a time and puts them into the wave's LDS region (64 x D*D doubles, the
// producer's); the lanes are then re-dealt over (cell, node, r) and add the Q values in ascending q.
//
// Node kernel: one lane per nodal dof, a grid-stride loop;  f = 0.0 (or out's value);  f = f + fe[c][a][r] over the node's CSR
// entries c*A + a in ascending order.  No floating-point atomics anywhere: the order of every sum is fixed.
//
// Memory: ref is staged once per block into LDS; stress, per-point jinv and the gradient arrive as coalesced 16-byte non-temporal
// chunks and are transposed through the region; the tangent arrives the same way in slabs of 8 (D = 3), 16 (D = 2) or 64 points
// whose lanes then read their rows; per-cell jinv and the weights are read per lane.  fe leaves as plain stores (the node kernel
// reads it at once).  Dead lanes load nothing.  Index arithmetic is 64-bit.
#pragma once
#include "tile_io.h"

namespace fcamd_if {
using namespace fcamd;

constexpr int D = FCAMD_IF_D, A = FCAMD_IF_A, Q = FCAMD_IF_Q, DD = D * D;
constexpr int S = D == 3 ? 6 : (D == 2 ? 4 : 1), SS = S * S;
constexpr bool kAffine = FCAMD_IF_AFFINE != 0, kNabla = FCAMD_IF_NABLA != 0, kTangent = FCAMD_IF_SOURCE != 0;
constexpr bool kAccumulate = FCAMD_IF_ACCUMULATE != 0;
static_assert(D >= 1 && D <= 3 && A >= 1 && Q >= 1 && Q <= kWave, "shape");
constexpr int kW0 = kWave / Q;
constexpr int W = (kW0 > 1 && (kW0 * Q * DD) % 2 != 0) ? kW0 - 1 : kW0;  // cells per tile
constexpr int kPts = W * Q;                                             // points of a whole tile
constexpr bool kEven = (kPts * DD) % 2 == 0;  // whole tiles start on the 16-byte grid (not so only for W = 1 with Q and D odd)
constexpr int kTable = Q * A * D;
constexpr int kTablePad = (kTable + 1) & ~1;
constexpr int kRegion = kWave * DD;  // the wave's region: 64 points x D*D doubles
constexpr int NG = D;                // nodes per group: 64 lanes x NG*D doubles fill the region
// points whose tangent rows pass through the region at a time: D = 3 half of what fits (8 points: 20 registers of chunks in flight
// next to e and s do not fit 64 VGPRs), else what fits (16 and 64)
constexpr int kSlab = D == 3 ? kRegion / SS / 2 : kRegion / SS;
constexpr int kSlabNC = (kSlab * SS + kWave - 1) / kWave;  // the slab's image: doubles per lane
constexpr double H = 0x1.6a09e667f3bcdp-1;  // 0x3FE6A09E667F3BCD, sqrt(0.5) rounded; 1/sqrt(2.0) is one ulp below
// force.py (lds_bytes, LDS_CAP) refuses such a shape before it gets here
static_assert((kTablePad + kWavesPerBlock * kRegion) * 8 <= 64 * 1024, "reference table too large for the LDS of a block");
// the m-th shear component of the Mandel vector is the pair (0,1), (0,2), (1,2)
constexpr int kPairs = D == 3 ? 3 : (D == 2 ? 1 : 0);
__device__ constexpr int pair_i(int m) { return m == 2 ? 1 : 0; }
__device__ constexpr int pair_j(int m) { return m == 0 ? 1 : 2; }
static_assert(S <= DD && kSlabNC <= DD && NG * D == DD, "region");

// the element kernel's only parameter; force.py mirrors the layout (ElementArgs)
struct ElementArgs {
    const double* src;      // [S n] stress or [S*S n] tangent
    const double* grad;     // [D*D n] gradient of v in the producer's layout (tangent action only)
    const double* ref;      // [Q][A][D]
    const double* jinv;     // [C][D][D] or [C][Q][D][D]
    const double* weights;  // [C][Q]
    double* fe;             // [C][A][D]
    long long n_cells;
};
// the node kernel's
struct NodeArgs {
    const double* fe;     // [C][A][D]
    const int* node_ptr;  // [n_nodes + 1]
    const int* adj;       // entries c*A + a, ascending within a node
    double* out;          // [D n_nodes]
    long long n_dofs;
};

// the first `nelem` doubles at src dealt over the lanes in the image of tile_load.  ALIGNED (src on the 16-byte grid): 16-byte
// non-temporal chunks and, where nelem is odd, one 8-byte load for the last double; else guarded 8-byte loads
template <int NC, bool ALIGNED>
__device__ __forceinline__ void load_image(Chunks<NC>& c, const double* src, int nelem, int lane) {
    if constexpr (ALIGNED) {
        const int whole = nelem >> 1;  // chunk k*64 + lane is whole below this index (the lane compared with a scalar: no register per k)
        const double* mine = src + 2 * lane;
#pragma unroll
        for (int k = 0; k < Chunks<NC>::K; ++k) {
            d2 v;
            v.x = 0.0;
            v.y = 0.0;
            if (lane < whole - k * kWave)
                v = load16<true>(mine + 2 * k * kWave);
            else if ((nelem & 1) && lane == whole - k * kWave)
                v.x = mine[2 * k * kWave];
            c.v[k] = v;
        }
    } else {
        tile_load<NC, false, false>(c, src, nelem, lane);
    }
}

// the NC doubles of this lane's point out of an AoS tile of npts points
template <int NC, bool ALIGNED>
__device__ __forceinline__ void load_points(const double* src, int npts, double* region, int lane, double (&x)[NC]) {
    Chunks<NC> c;
    load_image<NC, ALIGNED>(c, src, npts * NC, lane);
    transpose_in<NC>(c, region, lane, x);
}

// s = C e of this lane's point; the tile's tangent rows pass through the region slab by slab
__device__ __forceinline__ void tangent_times_strain(const double* tan, int npts, double* region, int lane, const double (&e)[S], double (&s)[S]) {
#pragma unroll
    for (int i = 0; i < S; ++i) s[i] = 0.0;
#pragma unroll 1
    for (int first = 0; first < npts; first += kSlab) {
        const int pts = npts - first < kSlab ? npts - first : kSlab;
        Chunks<kSlabNC> c;
        load_image<kSlabNC, kEven>(c, tan + (long long)first * SS, pts * SS, lane);
        tile_to_lds<kSlabNC>(c, region, lane);
        wave_sync();
        if (lane >= first && lane < first + pts) {
            const double* row = region + (lane - first) * SS;
#pragma unroll
            for (int i = 0; i < S; ++i) {
#pragma unroll
                for (int j = 0; j < S; ++j) s[i] = s[i] + row[S * i + j] * e[j];
                __builtin_amdgcn_sched_barrier(0);  // a row's reads at a time: all S*S in flight do not fit 64 VGPRs
            }
        }
        wave_sync();
    }
}

// the tile of `ncells` cells starting at cell c0 (FULL: W cells)
template <bool FULL>
__device__ __forceinline__ void force_tile(const ElementArgs& a, const double* table, double* region, long long c0, int ncells, int lane) {
    const int npts = FULL ? kPts : ncells * Q;
    const bool live = lane < npts;
    const long long p0 = c0 * Q;
    const int cl = live ? lane / Q : 0;
    const int q = live ? lane - cl * Q : 0;
    double s[S];
    if constexpr (kTangent) {
        double gv[DD];
        load_points<DD, kEven>(a.grad + p0 * DD, npts, region, lane, gv);
        double G[D][D];  // G[r][x] = d v_r / d x_x
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int x = 0; x < D; ++x) G[r][x] = gv[kNabla ? D * x + r : D * r + x];
        double e[S];
#pragma unroll
        for (int i = 0; i < D; ++i) e[i] = G[i][i];
        if constexpr (D == 2) e[S / 2] = 0.0;  // zz: no strain in the plane
#pragma unroll
        for (int m = 0; m < kPairs; ++m) e[3 + m] = H * (G[pair_i(m)][pair_j(m)] + G[pair_j(m)][pair_i(m)]);
        tangent_times_strain(a.src + p0 * SS, npts, region, lane, e, s);
    } else {
        load_points<S, kEven>(a.src + p0 * S, npts, region, lane, s);
    }
    double T[D][D];
#pragma unroll
    for (int i = 0; i < D; ++i) T[i][i] = s[i];
#pragma unroll
    for (int m = 0; m < kPairs; ++m) T[pair_i(m)][pair_j(m)] = T[pair_j(m)][pair_i(m)] = s[3 + m] * H;
    double J[DD];
    if constexpr (kAffine) {
#pragma unroll
        for (int i = 0; i < DD; ++i) J[i] = live ? a.jinv[(c0 + cl) * DD + i] : 0.0;
    } else {
        load_points<DD, kEven>(a.jinv + p0 * DD, npts, region, lane, J);
    }
    int wl = lane;
    asm volatile("" : "+v"(wl));  // the address is formed here, not kept as a per-lane pointer across the tile loop: registers
    const double w = live ? __builtin_nontemporal_load(a.weights + p0 + wl) : 0.0;
    const double* t = table + q * (A * D);
#pragma unroll 1
    for (int a0 = 0; a0 < A; a0 += NG) {
        if (live) {
#pragma unroll
            for (int b = 0; b < NG; ++b) {
                if (a0 + b < A) {
                    double g[D];
#pragma unroll
                    for (int x = 0; x < D; ++x) {
                        g[x] = 0.0;
#pragma unroll
                        for (int k = 0; k < D; ++k) g[x] = g[x] + t[(a0 + b) * D + k] * J[D * k + x];
                    }
#pragma unroll
                    for (int r = 0; r < D; ++r) {
                        double tr = 0.0;
#pragma unroll
                        for (int x = 0; x < D; ++x) tr = tr + T[r][x] * g[x];
                        region[lane * DD + b * D + r] = tr * w;
                    }
                }
            }
        }
        wave_sync();
        // lanes re-dealt over (cell, node of the group, r): the Q values of a cell's point in ascending q
        for (int o = lane; o < ncells * DD; o += kWave) {
            const int ce = o / DD;
            const int j = o - ce * DD;  // D * (node of the group) + r
            if (a0 + j / D < A) {
                const double* v = region + ce * (Q * DD) + j;
                double acc = 0.0;
                for (int k = 0; k < Q; ++k) acc = acc + v[k * DD];
                a.fe[((c0 + ce) * A + a0) * D + j] = acc;
            }
        }
        wave_sync();
    }
}

}  // namespace fcamd_if

extern "C" __global__ void __launch_bounds__(fcamd::kBlock, FCAMD_IF_WAVES) fcamd_internal_force_element_kernel(const fcamd_if::ElementArgs a) {
    using namespace fcamd_if;
    __shared__ __attribute__((aligned(16))) double table[kTablePad];
    __shared__ __attribute__((aligned(16))) double scratch[kWavesPerBlock][kRegion];
    for (int i = (int)threadIdx.x; i < kTable; i += kBlock) table[i] = a.ref[i];
    __syncthreads();
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    double* region = scratch[wave];
    const long long nfull = a.n_cells / W;
    const long long wstride = (long long)gridDim.x * kWavesPerBlock;
    long long tile = (long long)blockIdx.x * kWavesPerBlock + wave;
    for (; tile < nfull; tile += wstride) force_tile<true>(a, table, region, tile * W, W, lane);
    if (tile == nfull && a.n_cells > nfull * W) force_tile<false>(a, table, region, tile * W, (int)(a.n_cells - nfull * W), lane);
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_internal_force_node_kernel(const fcamd_if::NodeArgs a) {
    using namespace fcamd_if;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n_dofs; i += stride) {
        const long long v = i / D;
        const int r = (int)(i - v * D);
        double f = kAccumulate ? a.out[i] : 0.0;
        const int last = a.node_ptr[v + 1];
        for (int k = a.node_ptr[v]; k < last; ++k) f = f + a.fe[(long long)a.adj[k] * D + r];
        a.out[i] = f;
    }
}
