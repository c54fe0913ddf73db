// The assembled tangent stiffness (matrix.py: TangentMatrix): K = sum_p B_p^T C_p B_p w_p as the values of a sparse matrix whose
// pattern the host built once.  Read at run time and compiled with hiprtc behind the generated definitions:
//   FCAMD_TM_D       geometric dimension: 1, 2 or 3 (the tangent has S x S entries per point, S = 1, 4 or 6)
//   FCAMD_TM_A       nodes per cell
//   FCAMD_TM_Q       quadrature points per cell
//   FCAMD_TM_AFFINE  1: jinv[C][D][D], one inverse Jacobian per cell; 0: jinv[C][Q][D][D], one per point
//   FCAMD_TM_SLAB    points whose tangent, jinv, weights and basis gradients sit in a wave's LDS region at a time
//   FCAMD_TM_WAVES   waves per SIMD the register budget of the element kernel is cut for
//
// Two kernels, launched one behind the other on one stream, once per chunk of cells (the scratch between them is bounded).
//
// Element kernel: 256-thread blocks, one wave per tile, a grid-stride loop over the tiles.  With M = A*D columns a tile is
// CW = max(1, 64 / M) whole cells; a lane owns ONE column (b, s) of one cell's element matrix and keeps the M entries of that
// column in registers across the points of the cell, so the sum over q runs in ascending q inside one lane (where M > 64 the
// columns are taken in passes of 64).  With -ffp-contract=off the arithmetic of a column is exactly, in this order (H the double
// of sqrt(0.5)), the tangent action of internal_force.hip on the unit displacement of local node b in direction s:
//   g[a][x] = 0.0;  g[a][x] = g[a][x] + ref[q][a][k] * jinv[c(,q)][k][x], k ascending
//   G[r][x] = r == s ? g[b][x] : 0.0
//   e = (G00, G11, G22, H*(G01+G10), H*(G02+G20), H*(G12+G21));  sv[i] = 0.0;  sv[i] = sv[i] + C[i][j] * e[j], j ascending
//   T[i][i] = sv[i];  T[i][j] = T[j][i] = sv[3 + m] * H
//   t = 0.0;  t = t + T[r][x] * g[a][x], x ascending;   ke[a][r][b][s] = ke[a][r][b][s] + t * w[c][q], q ascending from 0.0
// Nothing is dropped: the zero entries of G take part as +0.0.  The points of a tile pass through the wave's LDS region in slabs:
// the tangent rows, the per-point jinv and the weights arrive as coalesced 16-byte non-temporal chunks (8-byte loads where the
// slab does not start on the 16-byte grid), the wave forms g[point][a][x] of the slab together, and every lane then reads C, g
// and w of its cell's points from the region (lanes of one cell read the same address: a broadcast).  The element matrix leaves
// row-major, ke[c][a][r][b][s]: a wave's store of one row is one contiguous run per cell.
//
// Gather kernel: one lane per scalar entry (block k, r, s) of the pattern, a grid-stride loop (the first chunk's over all entries, a
// later chunk's over the range of blocks its cells touch, which the host knows).  The block's contributions
// (c, a, b) with dofmap[c][a] == v and dofmap[c][b] == u are listed ascending in c*A*A + a*A + b; the lane starts from 0.0 (or
// values' own content), adds ke[c][a][r][b][s] over the contributions of THIS chunk's cells in list order and writes
// values[base[k] + r * stride[k] + s] -- base and stride come from the host, which is all the kernel knows of BSR or CSR.  The
// D*D lanes of a block read D runs of D neighbouring doubles of one (c, a, ., b, .) block.  An entry whose row or column dof is
// constrained is written as the constant 1.0 (diagonal) or 0.0 and never read or added to.  No floating-point atomics anywhere.
#pragma once
#include "tile_io.h"

namespace fcamd_tm {
using namespace fcamd;

constexpr int D = FCAMD_TM_D, A = FCAMD_TM_A, Q = FCAMD_TM_Q, DD = D * D;
constexpr int S = D == 3 ? 6 : (D == 2 ? 4 : 1), SS = S * S;
constexpr bool kAffine = FCAMD_TM_AFFINE != 0;
constexpr int M = A * D;                          // columns (and rows) of an element matrix
constexpr int MM = M * M;
constexpr int CW = M >= kWave ? 1 : kWave / M;    // cells per tile
constexpr int kPasses = (M + kWave - 1) / kWave;  // passes over the columns (1 unless M > 64)
constexpr int kSlab = FCAMD_TM_SLAB;
constexpr int kPts = CW * Q;  // points of a whole tile
static_assert(D >= 1 && D <= 3 && A >= 1 && Q >= 1 && kSlab >= 1, "shape");
constexpr int even(int n) { return (n + 1) & ~1; }
// the wave's region: tangent rows, per-point jinv, basis gradients, weights of a slab (every part on the 16-byte grid)
constexpr int kOffC = 0;
constexpr int kOffJ = kOffC + even(kSlab * SS);
constexpr int kOffG = kOffJ + (kAffine ? 0 : even(kSlab * DD));
constexpr int kOffW = kOffG + even(kSlab * M);
constexpr int kRegion = kOffW + even(kSlab);
constexpr int kTable = Q * A * D;
constexpr int kTablePad = even(kTable);
constexpr double H = 0x1.6a09e667f3bcdp-1;  // 0x3FE6A09E667F3BCD, sqrt(0.5) rounded; 1/sqrt(2.0) is one ulp below
// matrix.py (lds_bytes, LDS_CAP) refuses such a shape before it gets here
static_assert((kTablePad + kWavesPerBlock * kRegion) * 8 <= 64 * 1024, "tables too large for the LDS of a block");
constexpr int kPairs = D == 3 ? 3 : (D == 2 ? 1 : 0);
__device__ constexpr int pair_i(int m) { return m == 2 ? 1 : 0; }
__device__ constexpr int pair_j(int m) { return m == 0 ? 1 : 2; }

// the element kernel's only parameter (the arrays start at the chunk's first cell); matrix.py mirrors the layout
struct ElementArgs {
    const double* tangent;  // [C][Q][S][S]
    const double* ref;      // [Q][A][D]
    const double* jinv;     // [C][D][D] or [C][Q][D][D]
    const double* weights;  // [C][Q]
    double* ke;             // [C][A][D][A][D]
    long long n_cells;      // of the chunk
};
// the gather kernel's
struct GatherArgs {
    const double* ke;             // the chunk's element matrices
    const int* blk_ptr;           // [nnzb + 1] into contrib
    const int* contrib;           // c*A*A + a*A + b, ascending within a block
    const long long* dest_base;   // [nnzb] position of entry (0, 0) of the block in values
    const int* dest_stride;       // [nnzb] distance of the block's rows in values
    const int* block_row;         // [nnzb] node v of the block (read with a mask only)
    const int* block_col;         // [nnzb] node u
    const unsigned char* mask;    // [D n_nodes] 1: constrained dof; or null
    double* values;
    long long entry0;     // the entries this launch covers: entry0 <= D*D*k + D*r + s < n_entries (a later chunk: its own blocks' range)
    long long n_entries;
    long long key_lo;     // the chunk's contributions: key_lo <= c*A*A + a*A + b < key_hi
    long long key_hi;
    long long cell0;      // the chunk's first cell
    int first;            // 1: the first chunk of a call (it starts the entries); 0: a later one (it goes on from values)
    int accumulate;       // 1: the first chunk starts from values' content; 0: from 0.0
};

// `n` doubles from src into the region at dst, dealt over the lanes: 16-byte non-temporal chunks where src is on the 16-byte grid
// (the same for the whole wave), 8-byte loads else and for an odd last double
__device__ __forceinline__ void stage(double* dst, const double* src, int n, int lane) {
    if ((reinterpret_cast<unsigned long long>(src) & 15ull) == 0ull) {
        const int whole = n >> 1;
        for (int i = lane; i < whole; i += kWave) reinterpret_cast<d2*>(dst)[i] = load16<true>(src + 2 * i);
        if ((n & 1) && lane == 0) dst[n - 1] = __builtin_nontemporal_load(src + n - 1);
    } else {
        for (int i = lane; i < n; i += kWave) dst[i] = __builtin_nontemporal_load(src + i);
    }
}

// the tile of `ncells` cells starting at cell c0 of the chunk
__device__ __forceinline__ void matrix_tile(const ElementArgs& a, const double* table, double* region, long long c0, int ncells, int lane) {
    const int npts = ncells * Q;
    const long long p0 = c0 * Q;
    double* Cs = region + kOffC;
    double* Js = region + kOffJ;
    double* gs = region + kOffG;
    double* ws = region + kOffW;
#pragma unroll 1
    for (int pass = 0; pass < kPasses; ++pass) {
        const int item = pass * kWave + lane;  // (cell of the tile, column)
        const int cl = item / M;
        const int col = item - cl * M;
        const bool live = cl < ncells;
        const int b = col / D;
        const int s = col - b * D;
        double acc[M];
#pragma unroll
        for (int i = 0; i < M; ++i) acc[i] = 0.0;
#pragma unroll 1
        for (int first = 0; first < npts; first += kSlab) {
            const int pts = npts - first < kSlab ? npts - first : kSlab;
            stage(Cs, a.tangent + (p0 + first) * SS, pts * SS, lane);
            if constexpr (!kAffine) stage(Js, a.jinv + (p0 + first) * DD, pts * DD, lane);
            stage(ws, a.weights + p0 + first, pts, lane);
            wave_sync();
            // g[point][a][x] of the slab, the wave together
            for (int o = lane; o < pts * M; o += kWave) {
                const int pt = o / M;
                const int ax = o - pt * M;
                const int an = ax / D;
                const int x = ax - an * D;
                const int tp = first + pt;  // point of the tile
                const int ce = tp / Q;
                const int q = tp - ce * Q;
                const double* t = table + (q * A + an) * D;
                double g = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double j = kAffine ? a.jinv[(c0 + ce) * DD + D * k + x] : Js[pt * DD + D * k + x];
                    g = g + t[k] * j;
                }
                gs[o] = g;
            }
            wave_sync();
            if (live) {
                // this cell's points of the slab, ascending q
                int lo = cl * Q - first, hi = lo + Q;
                lo = lo < 0 ? 0 : lo;
                hi = hi > pts ? pts : hi;
#pragma unroll 1
                for (int pt = lo; pt < hi; ++pt) {
                    const double* Cp = Cs + pt * SS;
                    const double* gp = gs + pt * M;
                    double G[D][D];
#pragma unroll
                    for (int r = 0; r < D; ++r)
#pragma unroll
                        for (int x = 0; x < D; ++x) G[r][x] = r == s ? gp[b * D + x] : 0.0;
                    double e[S];
#pragma unroll
                    for (int i = 0; i < D; ++i) e[i] = G[i][i];
                    if constexpr (D == 2) e[S / 2] = 0.0;  // zz: no strain in the plane
#pragma unroll
                    for (int m = 0; m < kPairs; ++m) e[3 + m] = H * (G[pair_i(m)][pair_j(m)] + G[pair_j(m)][pair_i(m)]);
                    double sv[S];
#pragma unroll
                    for (int i = 0; i < S; ++i) {
                        sv[i] = 0.0;
#pragma unroll
                        for (int j = 0; j < S; ++j) sv[i] = sv[i] + Cp[S * i + j] * e[j];
                    }
                    double T[D][D];
#pragma unroll
                    for (int i = 0; i < D; ++i) T[i][i] = sv[i];
#pragma unroll
                    for (int m = 0; m < kPairs; ++m) T[pair_i(m)][pair_j(m)] = T[pair_j(m)][pair_i(m)] = sv[3 + m] * H;
                    const double w = ws[pt];
#pragma unroll
                    for (int an = 0; an < A; ++an) {
#pragma unroll
                        for (int r = 0; r < D; ++r) {
                            double t = 0.0;
#pragma unroll
                            for (int x = 0; x < D; ++x) t = t + T[r][x] * gp[an * D + x];
                            acc[an * D + r] = acc[an * D + r] + t * w;
                        }
                    }
                }
            }
            wave_sync();
        }
        if (live && col < M) {
            double* dst = a.ke + (c0 + cl) * MM + col;
#pragma unroll
            for (int i = 0; i < M; ++i) dst[(long long)i * M] = acc[i];
        }
    }
}

}  // namespace fcamd_tm

extern "C" __global__ void __launch_bounds__(fcamd::kBlock, FCAMD_TM_WAVES) fcamd_tangent_matrix_element_kernel(const fcamd_tm::ElementArgs a) {
    using namespace fcamd_tm;
    __shared__ __attribute__((aligned(16))) double table[kTablePad];
    __shared__ __attribute__((aligned(16))) double scratch[kWavesPerBlock][kRegion];
    for (int i = (int)threadIdx.x; i < kTable; i += kBlock) table[i] = a.ref[i];
    __syncthreads();
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    double* region = scratch[wave];
    const long long ntiles = (a.n_cells + CW - 1) / CW;
    const long long wstride = (long long)gridDim.x * kWavesPerBlock;
    for (long long tile = (long long)blockIdx.x * kWavesPerBlock + wave; tile < ntiles; tile += wstride) {
        const long long c0 = tile * CW;
        const long long left = a.n_cells - c0;
        matrix_tile(a, table, region, c0, left < CW ? (int)left : CW, lane);
    }
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_tangent_matrix_gather_kernel(const fcamd_tm::GatherArgs a) {
    using namespace fcamd_tm;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = a.entry0 + (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n_entries; i += stride) {
        const long long k = i / DD;
        const int rs = (int)(i - k * DD);
        const int r = rs / D;
        const int s = rs - r * D;
        double* dst = a.values + a.dest_base[k] + (long long)r * a.dest_stride[k] + s;
        if (a.mask != nullptr) {
            const long long row = (long long)a.block_row[k] * D + r, colm = (long long)a.block_col[k] * D + s;
            if (a.mask[row] || a.mask[colm]) {
                if (a.first) *dst = row == colm ? 1.0 : 0.0;
                continue;
            }
        }
        const int end = a.blk_ptr[k + 1];
        int j = a.blk_ptr[k];
        if (!a.first) {  // the first contribution of this chunk: the list is ascending
            int hi = end;
            while (j < hi) {
                const int mid = j + (hi - j) / 2;
                if (a.contrib[mid] < a.key_lo)
                    j = mid + 1;
                else
                    hi = mid;
            }
        }
        int key = j < end ? a.contrib[j] : 0;
        const bool any = j < end && key < a.key_hi;
        if (!any && !a.first) continue;  // nothing of this chunk: the entry stays as it is
        double f = (a.first && !a.accumulate) ? 0.0 : *dst;
        while (j < end && key < a.key_hi) {
            const int c = key / (A * A);
            const int ab = key - c * (A * A);
            const int an = ab / A;
            const int bn = ab - an * A;
            f = f + a.ke[(c - a.cell0) * MM + (long long)(an * D + r) * M + bn * D + s];
            ++j;
            key = j < end ? a.contrib[j] : 0;
        }
        *dst = f;
    }
}
