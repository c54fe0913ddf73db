// The first Galerkin step of the multilevel preconditioner of a TangentOperator with the rigid-body coarse space (multilevel.py:
// MultilevelPreconditioner(A, coarse_space="rigid_body")): the Dc x Dc blocks of level 1 straight from the element matrices,
// K1 = P^T (M K M + I - M) P with P_i = [I_D  B(o_i)], with no fine matrix in between.  Read at run time and compiled with hiprtc
// behind the generated definitions:
//   FCAMD_MF_D   dofs per node = the space dimension: 2 or 3 (Dc = 3 or 6)
//   FCAMD_MF_A   nodes per cell
//
// The element matrices ke[c][a][a'][b][b'] of a chunk of cells come from fcamd_tangent_matrix_element_kernel (tangent_matrix.hip)
// in a bounded scratch; the kernel here follows it on the same stream, once per chunk.  The contribution lists (c*A*A + a*A + b of
// every coarse block, ascending) are those of multilevel_free.hip.  B(o) and P's entries are the ones of multilevel_rigid.hip.
//
// The rule, for coarse block K = (I, J) and entry (r, s), 0 <= r, s < Dc:
//   first chunk:  f = 0.0;  with a mask and I == J, over the members i of I, ascending:
//                   t = 0.0;  for a = 0 .. D-1 ascending, where dof D*i + a is constrained:  t = t + P_i[a][r] * P_i[a][s];   f = f + t
//   later chunk:  f = the value that is there
//   over the contributions (c, a, b) of THIS chunk's cells in list order, i = dofmap[c][a], j = dofmap[c][b]:
//     t = 0.0;  for a' = 0 .. D-1 ascending, skipped where dof D*i + a' is constrained:
//       u = 0.0;  for b' = 0 .. D-1 ascending, skipped where dof D*j + b' is constrained:  u = u + ke[c][a][a'][b][b'] * P_j[b'][s]
//       t = t + P_i[a'][r] * u
//     f = f + t
// and values1[Dc*Dc*K + Dc*r + s] = f (block CSR).
//
// The lanes of one coarse block work together: a GROUP of GL lanes (3-D: a whole wave, 36 of its 64 lanes own an entry; 2-D: 16
// lanes, 9 own an entry, four groups per wave) takes one coarse block, 256 / GL groups per 256-thread block, grid-stride over the
// coarse blocks of the launch.  Lane 0 of a group finds the block's contributions of this chunk (a later chunk: one bisection per
// coarse block) and the group hears of it through LDS.  The group then stages batches through LDS: NB = GL / (D*D) contributions at
// a time -- every lane loads one double of a D x D sub-block of ke; the first NB*2*D lanes load one coordinate of the two nodes'
// offsets and the constrained byte of the same dof -- and, in the start, NM = GL / D members at a time (one coordinate and one
// byte per lane).  Behind a barrier every entry's lane runs its chain over the staged batch in list order, reading LDS at
// group-uniform addresses (broadcasts).  So each ke sub-block, offset and mask byte is fetched from memory once per coarse block
// and chunk, and the order of an entry's sum is the rule's whatever the batch, the block size, the grid or the scratch.  The trips of
// the batch loops are made uniform over the block (the largest count of its groups, by LDS) so that the barriers are
// __syncthreads().  No floating-point atomics, no MFMA; every product is rounded before its sum (-ffp-contract=off).
#pragma once
#include "tile_io.h"

namespace fcamd_mfr {
using namespace fcamd;

constexpr int D = FCAMD_MF_D, A = FCAMD_MF_A, DD = D * D;
constexpr int R = D == 3 ? 3 : 1;  // rotations
constexpr int Dc = D + R;          // dofs of a coarse node
constexpr int EE = Dc * Dc;        // entries of a coarse block
constexpr int M = A * D;           // columns (and rows) of an element matrix
constexpr long long MM = (long long)M * M;
constexpr int GL = D == 3 ? 64 : 16;  // lanes of a group
constexpr int GROUPS = kBlock / GL;   // coarse blocks a thread block has in hand
constexpr int NB = GL / DD;           // contributions of a batch: 7 or 4
constexpr int NM = GL / D;            // members of a batch of the start: 21 or 8
static_assert(D == 2 || D == 3, "the rigid-body coarse space is for 2 and 3 dimensions");
static_assert(A >= 1 && kBlock % GL == 0 && EE <= GL && NB >= 1 && NB * 2 * D <= GL && NM * D <= GL, "shape");

// the kernel's only parameter; multilevel.py mirrors the layout
struct Args {
    const double* ke;            // the chunk's element matrices [cells of the chunk][A][D][A][D]
    const int* blk_ptr;          // [coarse blocks + 1] into contrib
    const int* contrib;          // c*A*A + a*A + b, ascending within a coarse block
    const int* dofmap;           // [C][A]
    const unsigned char* mask;   // [D n_nodes] 1: constrained dof; or null
    const int* block_row;        // [coarse blocks] aggregate I of the block
    const int* block_col;        // [coarse blocks] aggregate J
    const int* mem_ptr;          // [aggregates + 1] (read with a mask only)
    const int* members;          // [fine nodes] the members of every aggregate, ascending
    const double* offsets;       // [fine nodes][D] the offsets of level 0
    double* values;              // [Dc*Dc coarse blocks] the values of level 1, block CSR
    long long block0;    // the coarse blocks this launch covers: block0 <= K < block1 (a later chunk: the range its cells touch)
    long long block1;
    long long key_lo;    // the chunk's contributions: key_lo <= c*A*A + a*A + b < key_hi
    long long key_hi;
    long long cell0;     // the chunk's first cell
    int first;           // 1: the first chunk of a call (it starts the entries); 0: a later one (it goes on from values)
    int pad;
};

// P[a][c] of the offset o, 0 <= a < D, 0 <= c < Dc: multilevel_rigid.hip's p_entry for a fine node of D dofs
__device__ __forceinline__ double p_entry(const double* o, int a, int c) {
    if (c < D) return a == c ? 1.0 : 0.0;
    const int t = c - D;
    if constexpr (D == 2) {
        return a == 0 ? -o[1] : o[0];
    } else {
        if (a == 0) return t == 0 ? 0.0 : (t == 1 ? o[2] : -o[1]);
        if (a == 1) return t == 0 ? -o[2] : (t == 1 ? 0.0 : o[0]);
        return t == 0 ? o[1] : (t == 1 ? -o[0] : 0.0);
    }
}

}  // namespace fcamd_mfr

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_mfr_galerkin_kernel(const fcamd_mfr::Args a) {
    using namespace fcamd_mfr;
    __shared__ double s_ke[GROUPS][GL];   // [q][a'][b'] of the batch
    __shared__ double s_off[GROUPS][GL];  // contributions: [q][side][D]; members: [m][D]
    __shared__ int s_held[GROUPS][GL];    // the constrained bytes, laid out as s_off
    __shared__ int s_range[GROUPS][4];    // j0, j1 of the group's block in this chunk; the members' m0, m1
    const int g = threadIdx.x / GL, lane = threadIdx.x - g * GL;
    const int r = lane / Dc, s = lane - r * Dc;  // (an entry's lane: lane < EE)
    double* const ke = s_ke[g];
    double* const off = s_off[g];
    int* const held = s_held[g];
    const bool masked = a.mask != nullptr;
    const long long stride = (long long)gridDim.x * GROUPS;
    for (long long base = a.block0 + (long long)blockIdx.x * GROUPS; base < a.block1; base += stride) {  // (uniform over the block)
        const long long k = base + g;
        const bool live = k < a.block1;
        if (lane == 0) {
            int j0 = 0, j1 = 0, m0 = 0, m1 = 0;
            if (live) {
                j0 = a.blk_ptr[k];
                j1 = a.blk_ptr[k + 1];
                // this chunk's contributions: the list is ascending (the first chunk's begin the list)
                int lo = j0, hi = j1;
                if (!a.first) {
                    while (lo < hi) {
                        const int mid = lo + (hi - lo) / 2;
                        if (a.contrib[mid] < a.key_lo)
                            lo = mid + 1;
                        else
                            hi = mid;
                    }
                    j0 = lo;
                    hi = j1;
                }
                if (j0 < j1 && a.contrib[j1 - 1] >= a.key_hi) {  // (the last chunk's, and the only chunk's, end the list)
                    while (lo < hi) {
                        const int mid = lo + (hi - lo) / 2;
                        if (a.contrib[mid] < a.key_hi)
                            lo = mid + 1;
                        else
                            hi = mid;
                    }
                    j1 = lo;
                }
                if (a.first && masked) {
                    const int agg = a.block_row[k];
                    if (agg == a.block_col[k]) {
                        m0 = a.mem_ptr[agg];
                        m1 = a.mem_ptr[agg + 1];
                    }
                }
            }
            s_range[g][0] = j0;
            s_range[g][1] = j1;
            s_range[g][2] = m0;
            s_range[g][3] = m1;
        }
        __syncthreads();
        const int j0 = s_range[g][0], j1 = s_range[g][1], m0 = s_range[g][2], m1 = s_range[g][3];
        int batches = 0, starts = 0;  // the block's longest
#pragma unroll
        for (int h = 0; h < GROUPS; ++h) {
            const int nb = (s_range[h][1] - s_range[h][0] + NB - 1) / NB, nm = (s_range[h][3] - s_range[h][2] + NM - 1) / NM;
            batches = nb > batches ? nb : batches;
            starts = nm > starts ? nm : starts;
        }
        __syncthreads();  // (the ranges have been read: the next trip may write them)
        // (a later chunk with nothing of this block: the entry stays as it is)
        const bool mine = live && lane < EE && (a.first || j0 < j1);
        const long long e = (long long)EE * k + lane;
        double f = 0.0;
        if (mine && !a.first) f = a.values[e];
        // the start: P^T (I - M) P over the members of a diagonal block
        for (int trip = 0; trip < starts; ++trip) {
            const int at = m0 + trip * NM;
            const int count = at < m1 ? (m1 - at < NM ? m1 - at : NM) : 0;
            if (lane < count * D) {
                const int m = lane / D;
                const long long dof = (long long)a.members[at + m] * D + (lane - m * D);
                off[lane] = a.offsets[dof];
                held[lane] = a.mask[dof] ? 1 : 0;
            }
            __syncthreads();
            if (mine) {
                for (int m = 0; m < count; ++m) {
                    const double* o = off + m * D;
                    double t = 0.0;
#pragma unroll
                    for (int ar = 0; ar < D; ++ar)
                        if (held[m * D + ar]) t = t + p_entry(o, ar, r) * p_entry(o, ar, s);
                    f = f + t;
                }
            }
            __syncthreads();
        }
        // the contributions
        for (int trip = 0; trip < batches; ++trip) {
            const int at = j0 + trip * NB;
            const int count = at < j1 ? (j1 - at < NB ? j1 - at : NB) : 0;
            if (lane < count * DD) {
                const int q = lane / DD, ab = lane - q * DD;
                const int key = a.contrib[at + q];
                const int c = key / (A * A), nodes = key - c * (A * A);
                const int an = nodes / A, bn = nodes - an * A;
                const int ar = ab / D, bc = ab - ar * D;
                ke[lane] = a.ke[(c - a.cell0) * MM + (long long)(an * D + ar) * M + bn * D + bc];
            }
            if (lane < count * 2 * D) {
                const int q = lane / (2 * D), rest = lane - q * 2 * D;
                const int side = rest / D, comp = rest - side * D;
                const int key = a.contrib[at + q];
                const int c = key / (A * A), nodes = key - c * (A * A);
                const int an = nodes / A, bn = nodes - an * A;
                const long long dof = (long long)a.dofmap[(long long)c * A + (side ? bn : an)] * D + comp;
                off[lane] = a.offsets[dof];
                held[lane] = masked ? (a.mask[dof] ? 1 : 0) : 0;
            }
            __syncthreads();
            if (mine) {
                for (int q = 0; q < count; ++q) {
                    const double* oi = off + q * 2 * D;
                    const double* oj = oi + D;
                    const int* hi = held + q * 2 * D;
                    const int* hj = hi + D;
                    const double* kq = ke + q * DD;
                    double t = 0.0;
#pragma unroll
                    for (int ar = 0; ar < D; ++ar) {
                        if (hi[ar]) continue;
                        double u = 0.0;
#pragma unroll
                        for (int bc = 0; bc < D; ++bc)
                            if (!hj[bc]) u = u + kq[ar * D + bc] * p_entry(oj, bc, s);
                        t = t + p_entry(oi, ar, r) * u;
                    }
                    f = f + t;
                }
            }
            __syncthreads();
        }
        if (mine) a.values[e] = f;
    }
}
