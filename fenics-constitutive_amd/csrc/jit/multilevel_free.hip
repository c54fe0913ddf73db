// The first Galerkin step of the multilevel preconditioner of a TangentOperator (multilevel.py: MultilevelPreconditioner on an
// operator): the values of level 1 straight from the element matrices, K1 = P^T (M K M + I - M) P, with no fine matrix in between.
// Read at run time and compiled with hiprtc behind the generated definitions:
//   FCAMD_MF_D   dofs per node: 1, 2 or 3
//   FCAMD_MF_A   nodes per cell
//
// The element matrices ke[c][a][r][b][s] of a chunk of cells come from fcamd_tangent_matrix_element_kernel (tangent_matrix.hip) in
// a bounded scratch; the kernel here follows it on the same stream, once per chunk.  With piecewise-constant translation
// aggregates P^T K P is a sum over the element matrices: ke[c][a][.][b][.] lands in the coarse block (agg[dofmap[c][a]],
// agg[dofmap[c][b]]).  The host lists the contributions c*A*A + a*A + b of every coarse block, ascending (matrix.contribution_lists
// on the dofmap of aggregates: key-based, so a cell whose nodes share an aggregate is listed like any other).
//
// One lane per scalar entry (coarse block K = (I, J), r, s), 256-thread blocks, a grid-stride loop -- the first chunk's over all
// entries, a later chunk's over the range of coarse blocks its cells touch, which the host knows:
//   f = the number of constrained dofs D*i + r among the members i of I, as a double, if I == J and r == s (the identity rows of
//       M K M + I - M: 1.0 per constrained member), else 0.0;  a later chunk goes on from the value that is there
//   over the contributions (c, a, b) of THIS chunk's cells in list order: nothing where dof D*dofmap[c][a] + r or dof
//       D*dofmap[c][b] + s is constrained, else  f = f + ke[c][a][r][b][s]
// and writes values1[D*D*K + D*r + s] (block CSR).  The sum of an entry runs in one lane in ascending c*A*A + a*A + b whatever the
// chunk size: the same bits for every scratch.  No floating-point atomics; -ffp-contract=off changes nothing here (sums only).
#pragma once
#include "tile_io.h"

namespace fcamd_mf {
using namespace fcamd;

constexpr int D = FCAMD_MF_D, A = FCAMD_MF_A, DD = D * D;
constexpr int M = A * D;  // columns (and rows) of an element matrix
constexpr int MM = M * M;
static_assert(D >= 1 && D <= 3 && A >= 1, "shape");

// the kernel's only parameter; multilevel.py mirrors the layout
struct Args {
    const double* ke;            // the chunk's element matrices [cells of the chunk][A][D][A][D]
    const int* blk_ptr;          // [coarse blocks + 1] into contrib
    const int* contrib;          // c*A*A + a*A + b, ascending within a coarse block
    const int* dofmap;           // [C][A] (all cells; read with a mask only)
    const unsigned char* mask;   // [D n_nodes] 1: constrained dof; or null
    const int* block_row;        // [coarse blocks] aggregate I of the block
    const int* block_col;        // [coarse blocks] aggregate J
    const int* mem_ptr;          // [aggregates + 1] (read with a mask only)
    const int* members;          // [fine nodes] the members of every aggregate, ascending
    double* values;              // [D*D coarse blocks] the values of level 1, block CSR
    long long entry0;    // the entries this launch covers: entry0 <= D*D*K + D*r + s < n_entries (a later chunk: its own blocks' range)
    long long n_entries;
    long long key_lo;    // the chunk's contributions: key_lo <= c*A*A + a*A + b < key_hi
    long long key_hi;
    long long cell0;     // the chunk's first cell
    int first;           // 1: the first chunk of a call (it starts the entries); 0: a later one (it goes on from values)
    int pad;
};

}  // namespace fcamd_mf

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_mf_galerkin_kernel(const fcamd_mf::Args a) {
    using namespace fcamd_mf;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = a.entry0 + (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n_entries; i += stride) {
        const long long k = i / DD;
        const int rs = (int)(i - k * DD);
        const int r = rs / D;
        const int s = rs - r * D;
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
        if (!a.first && !(j < end && key < a.key_hi)) continue;  // nothing of this chunk: the entry stays as it is
        double f;
        if (a.first) {
            int held = 0;
            if (a.mask != nullptr && r == s) {
                const int agg = a.block_row[k];
                if (agg == a.block_col[k]) {
                    const int m1 = a.mem_ptr[agg + 1];
                    for (int m = a.mem_ptr[agg]; m < m1; ++m) held += a.mask[(long long)a.members[m] * D + r] ? 1 : 0;
                }
            }
            f = (double)held;
        } else {
            f = a.values[i];
        }
        while (j < end && key < a.key_hi) {
            const int c = key / (A * A);
            const int ab = key - c * (A * A);
            const int an = ab / A;
            const int bn = ab - an * A;
            bool skip = false;
            if (a.mask != nullptr) {
                const long long row = (long long)a.dofmap[(long long)c * A + an] * D + r, colm = (long long)a.dofmap[(long long)c * A + bn] * D + s;
                skip = a.mask[row] || a.mask[colm];
            }
            if (!skip) f = f + a.ke[(c - a.cell0) * MM + (long long)(an * D + r) * M + bn * D + s];
            ++j;
            key = j < end ? a.contrib[j] : 0;
        }
        a.values[i] = f;
    }
}
