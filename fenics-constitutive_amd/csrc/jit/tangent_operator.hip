// The matrix-free tangent operator (tangent_operator.py: TangentOperator): y = M K M v + (I - M) v with K = sum_p B_p^T C_p B_p w_p
// applied from the tangent of the quadrature points, M the 0/1 diagonal of the free dofs, and the nodes' own D x D blocks of
// the same K for block-Jacobi -- what the conjugate gradients of solver.py need of a matrix, without one.  Read at run time and
// compiled with hiprtc behind the generated definitions:
//   FCAMD_TO_D       geometric dimension: 1, 2 or 3 (the tangent has S x S entries per point, S = 1, 4 or 6)
//   FCAMD_TO_A       nodes per cell
//   FCAMD_TO_Q       quadrature points per cell (at most 64)
//   FCAMD_TO_AFFINE  1: jinv[C][D][D], one inverse Jacobian per cell; 0: jinv[C][Q][D][D], one per point
//   FCAMD_TO_SLAB    points whose tangent, jinv, weights and basis gradients sit in a wave's region at a time (diagonal blocks)
//   FCAMD_TO_WAVES   waves per SIMD the register budget of the element kernels is cut for
// The control block, the modes and the pieces of the ordered dot (block_tree, last_block, final_sum) are those of
// conjugate_gradient.hip, used as they stand there.
//
// THE PRODUCT: two kernels, one behind the other on one stream.
//
// Element kernel: the tiling of internal_force.hip -- 256-thread blocks, one wave per tile of W = 64/Q whole cells (one less where
// W*Q*D*D would be odd), a lane per point, a grid-stride loop over the tiles, the short last tile separate.  With
// -ffp-contract=off the arithmetic of point p = Q*c + q is exactly, in this order (H the double of sqrt(0.5)), the producer's
// (displacement_gradient.hip) followed by the tangent form of internal_force.hip:
//   u[a][r] = +0.0 where dof D*dofmap[c][a] + r is constrained, else v[D*dofmap[c][a] + r]
//   R[r][k] = 0.0;  R[r][k] = R[r][k] + u[a][r] * ref[q][a][k], a ascending
//   G[r][x] = 0.0;  G[r][x] = G[r][x] + R[r][k] * jinv[c(,q)][k][x], k ascending
//   e = (G00, G11, G22, H*(G01+G10), H*(G02+G20), H*(G12+G21));  s[i] = 0.0;  s[i] = s[i] + C[i][j] * e[j], j ascending
//   T[i][i] = s[i];  T[i][j] = T[j][i] = s[3 + m] * H   for the m-th pair of (0,1), (0,2), (1,2)
//   fe[c][a][r] = 0.0;  for q ascending:  g[x] = 0.0;  g[x] = g[x] + ref[q][a][k] * jinv[c(,q)][k][x];  t = 0.0;  t = t + T[r][x] * g[x];
//                       fe[c][a][r] = fe[c][a][r] + t * weights[c][q]
// G never leaves the registers: no gradient array, no gradient layout.  The nodal values reach the lanes through the wave's LDS
// region, D nodes of every cell of the tile at a time: the wave gathers them once per cell (dofmap, mask and v are small and
// stay in the caches), and the Q lanes of a cell read the same address (a broadcast).  The tangent arrives as in
// internal_force.hip: coalesced 16-byte non-temporal chunks, slab by slab through the region.
//
// Node kernel: a lane per nodal dof, in the order of the solver's dot -- the block of a segment of 3072 dofs, thread t the dofs
// e = seg * 3072 + t + 256 i.  A constrained dof: y[e] = v[e]; else y[e] = 0.0; y[e] = y[e] + fe[c][a][r] over the node's CSR entries
// c*A + a ascending.  v[e] * y[e] is added as the rows complete; the tree, the partials, the last block and the final sum are the
// solver's.  Mode kIterate: both kernels return at once when the status is not "running", and the dot goes to pq (not pq > 0: the
// status becomes indefinite); kPlain: the dot goes to `dot`; kQuiet: no dot, the control block is not touched (and may be null).
//
// THE DIAGONAL BLOCKS: two kernels, once per chunk of cells (the scratch between them is bounded).
//
// Element kernel: a wave per tile of max(1, 64 / A) whole cells, a lane per (cell, local node a); the lane keeps the D x D block
// ke[c][a][.][a][.] in registers across the points of the cell.  The arithmetic of column s is that of tangent_matrix.hip:
//   g[a][x] = 0.0;  g[a][x] = g[a][x] + ref[q][a][k] * jinv[c(,q)][k][x], k ascending
//   G[r][x] = r == s ? g[a][x] : 0.0
//   e, sv[i] = 0.0;  sv[i] = sv[i] + C[i][j] * e[j] (the zero entries of G take part as +0.0),  T as above
//   t = 0.0;  t = t + T[r][x] * g[a][x], x ascending;   de[c][a][r][s] = de[c][a][r][s] + t * w[c][q], q ascending from 0.0
// The points pass through the wave's region in slabs, as in tangent_matrix.hip.
// Node kernel: a lane per entry (v, r, s); the first chunk starts from 0.0, a later one from what is there; + de[c][a][r][s] over the
// node's CSR entries c*A + a of THIS chunk's cells, ascending.  An entry whose row or column dof is constrained is written by the
// first chunk as the constant 1.0 (r == s) or 0.0 and never added to.
//
// No floating-point atomics, no MFMA; dead lanes load nothing; index arithmetic is 64-bit.
#pragma once
#define FCAMD_CG_D FCAMD_TO_D
#define FCAMD_CG_PRECOND 0
#define FCAMD_CG_SLAB 1024
#include "conjugate_gradient.hip"

namespace fcamd_to {
using namespace fcamd;

constexpr int D = FCAMD_TO_D, A = FCAMD_TO_A, Q = FCAMD_TO_Q, DD = D * D;
constexpr int S = D == 3 ? 6 : (D == 2 ? 4 : 1), SS = S * S;
constexpr bool kAffine = FCAMD_TO_AFFINE != 0;
static_assert(D >= 1 && D <= 3 && A >= 1 && Q >= 1 && Q <= kWave, "shape");
constexpr int kW0 = kWave / Q;
constexpr int W = (kW0 > 1 && (kW0 * Q * DD) % 2 != 0) ? kW0 - 1 : kW0;  // cells per tile of the product
constexpr int kPts = W * Q;                                             // points of a whole tile
constexpr bool kEven = (kPts * DD) % 2 == 0;  // whole tiles start on the 16-byte grid (not so only for W = 1 with Q and D odd)
constexpr int kTable = Q * A * D;
constexpr int kTablePad = (kTable + 1) & ~1;
constexpr int kRegion = kWave * DD;  // the wave's region: 64 points x D*D doubles
constexpr int NG = D;                // nodes per group: 64 lanes x NG*D doubles fill the region
constexpr int kSlab = D == 3 ? kRegion / SS / 2 : kRegion / SS;  // points whose tangent rows pass through the region at a time
constexpr int kSlabNC = (kSlab * SS + kWave - 1) / kWave;
constexpr double H = 0x1.6a09e667f3bcdp-1;  // 0x3FE6A09E667F3BCD, sqrt(0.5) rounded; 1/sqrt(2.0) is one ulp below
// tangent_operator.py (lds_bytes, LDS_CAP) refuses such a shape before it gets here
static_assert((kTablePad + kWavesPerBlock * kRegion) * 8 <= 64 * 1024, "reference table too large for the LDS of a block");
constexpr int kPairs = D == 3 ? 3 : (D == 2 ? 1 : 0);
__device__ constexpr int pair_i(int m) { return m == 2 ? 1 : 0; }
__device__ constexpr int pair_j(int m) { return m == 0 ? 1 : 2; }
static_assert(S <= DD && kSlabNC <= DD && NG * D == DD, "region");
constexpr int kSeg = fcamd_cg::kSeg, kPerLane = fcamd_cg::kPerLane;

// the diagonal blocks: M = A*D doubles of basis gradients per point; a tile is CW cells, a lane per (cell, node)
constexpr int M = A * D;
constexpr int CW = A >= kWave ? 1 : kWave / A;
constexpr int kPasses = (A + kWave - 1) / kWave;  // passes over the nodes (1 unless A > 64)
constexpr int kDSlab = FCAMD_TO_SLAB;
constexpr int even(int n) { return (n + 1) & ~1; }
// the parts of the region: tangent rows, per-point jinv, basis gradients, weights of a slab (every part on the 16-byte grid)
constexpr int kOffC = 0;
constexpr int kOffJ = kOffC + even(kDSlab * SS);
constexpr int kOffG = kOffJ + (kAffine ? 0 : even(kDSlab * DD));
constexpr int kOffW = kOffG + even(kDSlab * M);
static_assert(kDSlab >= 1 && kOffW + even(kDSlab) <= kRegion, "the slab of the diagonal blocks does not fit the wave's region");

// the product's element kernel's only parameter; tangent_operator.py mirrors the layout (ElementArgs)
struct ElementArgs {
    const double* tangent;      // [S*S n]
    const double* v;            // [D n_nodes]
    const int* dofmap;          // [C][A]
    const unsigned char* mask;  // [D n_nodes] 1: constrained dof; or null
    const double* ref;          // [Q][A][D]
    const double* jinv;         // [C][D][D] or [C][Q][D][D]
    const double* weights;      // [C][Q]
    double* fe;                 // [C][A][D]
    const fcamd_cg::Control* sc;  // read in mode kIterate only
    long long n_cells;
    int mode;
    int pad;
};
// the product's node kernel's
struct NodeArgs {
    const double* fe;           // [C][A][D]
    const int* node_ptr;        // [n_nodes + 1]
    const int* adj;             // entries c*A + a, ascending within a node
    const double* v;            // [D n_nodes]
    const unsigned char* mask;  // or null
    double* out;                // [D n_nodes]
    double* partials;           // [nseg]
    fcamd_cg::Control* sc;      // null in mode kQuiet
    long long n_dofs;
    long long nseg;
    int mode;
    int pad;
};
// the diagonal blocks' element kernel's (the arrays start at the chunk's first cell)
struct DiagElementArgs {
    const double* tangent;  // [C][Q][S][S]
    const double* ref;      // [Q][A][D]
    const double* jinv;     // [C][D][D] or [C][Q][D][D]
    const double* weights;  // [C][Q]
    double* de;             // [C][A][D][D]
    long long n_cells;      // of the chunk
};
// the diagonal blocks' node kernel's
struct DiagNodeArgs {
    const double* de;           // the chunk's blocks
    const int* node_ptr;        // [n_nodes + 1]
    const int* adj;             // entries c*A + a, ascending within a node
    const unsigned char* mask;  // or null
    double* out;                // [n_nodes][D][D]
    long long n_entries;        // D*D * n_nodes
    long long key_lo;           // the chunk's entries: key_lo <= c*A + a < key_hi
    long long key_hi;
    int first;                  // 1: the first chunk of a call (it starts the entries); 0: a later one (it goes on from out)
    int pad;
};

// the first `nelem` doubles at src dealt over the lanes in the image of tile_load.  ALIGNED (src on the 16-byte grid): 16-byte
// non-temporal chunks and, where nelem is odd, one 8-byte load for the last double; else guarded 8-byte loads
template <int NC, bool ALIGNED>
__device__ __forceinline__ void load_image(Chunks<NC>& c, const double* src, int nelem, int lane) {
    if constexpr (ALIGNED) {
        const int whole = nelem >> 1;
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
                __builtin_amdgcn_sched_barrier(0);  // a row's reads at a time
            }
        }
        wave_sync();
    }
}

// the tile of `ncells` cells starting at cell c0 (FULL: W cells)
template <bool FULL>
__device__ __forceinline__ void product_tile(const ElementArgs& a, const double* table, double* region, long long c0, int ncells, int lane) {
    const int npts = FULL ? kPts : ncells * Q;
    const bool live = lane < npts;
    const long long p0 = c0 * Q;
    const int cl = live ? lane / Q : 0;
    const int q = live ? lane - cl * Q : 0;
    const double* t = table + q * (A * D);
    // R of the producer: the nodal values of D nodes of every cell at a time through the region, [cell][node of the group][r]
    double R[D][D];
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
        for (int k = 0; k < D; ++k) R[r][k] = 0.0;
#pragma unroll 1
    for (int a0 = 0; a0 < A; a0 += NG) {
        for (int o = lane; o < ncells * DD; o += kWave) {
            const int ce = o / DD;
            const int j = o - ce * DD;
            const int b = j / D;
            double u = 0.0;
            if (a0 + b < A) {
                const long long dof = (long long)a.dofmap[(c0 + ce) * A + a0 + b] * D + (j - b * D);
                if (a.mask == nullptr || !a.mask[dof]) u = a.v[dof];
            }
            region[o] = u;
        }
        wave_sync();
        if (live) {
            const double* u = region + cl * DD;
#pragma unroll
            for (int b = 0; b < NG; ++b) {
                if (a0 + b < A) {
#pragma unroll
                    for (int r = 0; r < D; ++r) {
                        const double ur = u[b * D + r];
#pragma unroll
                        for (int k = 0; k < D; ++k) R[r][k] = R[r][k] + ur * t[(a0 + b) * D + k];
                    }
                }
            }
        }
        wave_sync();
    }
    double J[DD];
    if constexpr (kAffine) {
#pragma unroll
        for (int i = 0; i < DD; ++i) J[i] = live ? a.jinv[(c0 + cl) * DD + i] : 0.0;
    } else {
        load_points<DD, kEven>(a.jinv + p0 * DD, npts, region, lane, J);
    }
    double s[S];
    {
        double G[D][D];  // G[r][x] = d v_r / d x_x
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int x = 0; x < D; ++x) {
                double g = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) g = g + R[r][k] * J[D * k + x];
                G[r][x] = g;
            }
        double e[S];
#pragma unroll
        for (int i = 0; i < D; ++i) e[i] = G[i][i];
        if constexpr (D == 2) e[S / 2] = 0.0;  // zz: no strain in the plane
#pragma unroll
        for (int m = 0; m < kPairs; ++m) e[3 + m] = H * (G[pair_i(m)][pair_j(m)] + G[pair_j(m)][pair_i(m)]);
        tangent_times_strain(a.tangent + p0 * SS, npts, region, lane, e, s);
    }
    double T[D][D];
#pragma unroll
    for (int i = 0; i < D; ++i) T[i][i] = s[i];
#pragma unroll
    for (int m = 0; m < kPairs; ++m) T[pair_i(m)][pair_j(m)] = T[pair_j(m)][pair_i(m)] = s[3 + m] * H;
    int wl = lane;
    asm volatile("" : "+v"(wl));  // the address is formed here, not kept as a per-lane pointer across the tile loop: registers
    const double w = live ? __builtin_nontemporal_load(a.weights + p0 + wl) : 0.0;
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

// the diagonal blocks of the tile of `ncells` cells starting at cell c0 of the chunk
__device__ __forceinline__ void diagonal_tile(const DiagElementArgs& a, const double* table, double* region, long long c0, int ncells, int lane) {
    const int npts = ncells * Q;
    const long long p0 = c0 * Q;
    double* Cs = region + kOffC;
    double* Js = region + kOffJ;
    double* gs = region + kOffG;
    double* ws = region + kOffW;
#pragma unroll 1
    for (int pass = 0; pass < kPasses; ++pass) {
        const int item = pass * kWave + lane;  // (cell of the tile, local node)
        const int cl = item / A;
        const int b = item - cl * A;
        const bool live = cl < ncells;
        double acc[D][D];  // [r][s]
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int s = 0; s < D; ++s) acc[r][s] = 0.0;
#pragma unroll 1
        for (int first = 0; first < npts; first += kDSlab) {
            const int pts = npts - first < kDSlab ? npts - first : kDSlab;
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
                    const double* gp = gs + pt * M + b * D;
                    const double w = ws[pt];
                    double e[D][S];  // the strain of every column s
#pragma unroll
                    for (int s = 0; s < D; ++s) {
                        double G[D][D];
#pragma unroll
                        for (int r = 0; r < D; ++r)
#pragma unroll
                            for (int x = 0; x < D; ++x) G[r][x] = r == s ? gp[x] : 0.0;
#pragma unroll
                        for (int i = 0; i < D; ++i) e[s][i] = G[i][i];
                        if constexpr (D == 2) e[s][S / 2] = 0.0;  // zz: no strain in the plane
#pragma unroll
                        for (int m = 0; m < kPairs; ++m) e[s][3 + m] = H * (G[pair_i(m)][pair_j(m)] + G[pair_j(m)][pair_i(m)]);
                    }
                    double svs[D][S];
#pragma unroll
                    for (int i = 0; i < S; ++i) {
#pragma unroll
                        for (int s = 0; s < D; ++s) {
                            svs[s][i] = 0.0;
#pragma unroll
                            for (int j = 0; j < S; ++j) svs[s][i] = svs[s][i] + Cp[S * i + j] * e[s][j];
                        }
                        __builtin_amdgcn_sched_barrier(0);  // a row of C at a time, shared by the D columns: registers
                    }
#pragma unroll
                    for (int s = 0; s < D; ++s) {
                        const double(&sv)[S] = svs[s];
                        double T[D][D];
#pragma unroll
                        for (int i = 0; i < D; ++i) T[i][i] = sv[i];
#pragma unroll
                        for (int m = 0; m < kPairs; ++m) T[pair_i(m)][pair_j(m)] = T[pair_j(m)][pair_i(m)] = sv[3 + m] * H;
#pragma unroll
                        for (int r = 0; r < D; ++r) {
                            double t = 0.0;
#pragma unroll
                            for (int x = 0; x < D; ++x) t = t + T[r][x] * gp[x];
                            acc[r][s] = acc[r][s] + t * w;
                        }
                    }
                }
            }
            wave_sync();
        }
        if (live && b < A) {
            double* dst = a.de + ((c0 + cl) * A + b) * DD;
#pragma unroll
            for (int r = 0; r < D; ++r)
#pragma unroll
                for (int s = 0; s < D; ++s) dst[D * r + s] = acc[r][s];
        }
    }
}

}  // namespace fcamd_to

extern "C" __global__ void __launch_bounds__(fcamd::kBlock, FCAMD_TO_WAVES) fcamd_tangent_operator_element_kernel(const fcamd_to::ElementArgs a) {
    using namespace fcamd_to;
    __shared__ __attribute__((aligned(16))) double table[kTablePad];
    __shared__ __attribute__((aligned(16))) double scratch[kWavesPerBlock][kRegion];
    if (a.mode == fcamd_cg::kIterate && a.sc->status != fcamd_cg::kRunning) return;
    for (int i = (int)threadIdx.x; i < kTable; i += kBlock) table[i] = a.ref[i];
    __syncthreads();
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    double* region = scratch[wave];
    const long long nfull = a.n_cells / W;
    const long long wstride = (long long)gridDim.x * kWavesPerBlock;
    long long tile = (long long)blockIdx.x * kWavesPerBlock + wave;
    for (; tile < nfull; tile += wstride) product_tile<true>(a, table, region, tile * W, W, lane);
    if (tile == nfull && a.n_cells > nfull * W) product_tile<false>(a, table, region, tile * W, (int)(a.n_cells - nfull * W), lane);
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_tangent_operator_node_kernel(const fcamd_to::NodeArgs a) {
    using namespace fcamd_to;
    __shared__ double red[kBlock + 2];
    fcamd_cg::Control* sc = a.sc;
    if (a.mode == fcamd_cg::kIterate && sc->status != fcamd_cg::kRunning) return;
    const int t = (int)threadIdx.x;
    for (long long seg = blockIdx.x; seg < a.nseg; seg += gridDim.x) {
        double acc = 0.0;
#pragma unroll 1
        for (int i = 0; i < kPerLane; ++i) {
            const long long e = seg * kSeg + t + (long long)kBlock * i;
            if (e < a.n_dofs) {
                const double ve = a.v[e];
                double y = ve;
                if (a.mask == nullptr || !a.mask[e]) {
                    const long long node = e / D;
                    const int r = (int)(e - node * D);
                    y = 0.0;
                    const int last = a.node_ptr[node + 1];
                    for (int k = a.node_ptr[node]; k < last; ++k) y = y + a.fe[(long long)a.adj[k] * D + r];
                }
                a.out[e] = y;
                acc = acc + ve * y;
            }
        }
        if (a.mode == fcamd_cg::kQuiet) continue;  // (the same for the whole grid: no tree, no partial)
        const double total = fcamd_cg::block_tree(acc, red, t);
        if (t == 0) a.partials[seg] = total;
    }
    if (a.mode == fcamd_cg::kQuiet) return;
    if (fcamd_cg::last_block(sc, red, t)) {
        const double pq = fcamd_cg::final_sum(a.partials, a.nseg, red, t);
        if (t == 0) {
            if (a.mode == fcamd_cg::kIterate) {
                sc->pq = pq;
                if (!(pq > 0.0)) sc->status = fcamd_cg::kIndefinite;
            } else {
                sc->dot = pq;
            }
        }
    }
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock, FCAMD_TO_WAVES) fcamd_tangent_operator_diagonal_element_kernel(const fcamd_to::DiagElementArgs a) {
    using namespace fcamd_to;
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
        diagonal_tile(a, table, region, c0, left < CW ? (int)left : CW, lane);
    }
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_tangent_operator_diagonal_node_kernel(const fcamd_to::DiagNodeArgs a) {
    using namespace fcamd_to;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n_entries; i += stride) {
        const long long v = i / DD;
        const int rs = (int)(i - v * DD);
        const int r = rs / D;
        const int s = rs - r * D;
        if (a.mask != nullptr && (a.mask[v * D + r] || a.mask[v * D + s])) {
            if (a.first) a.out[i] = r == s ? 1.0 : 0.0;
            continue;
        }
        const int last = a.node_ptr[v + 1];
        int k = a.node_ptr[v];
        while (k < last && a.adj[k] < a.key_lo) ++k;  // the first entry of this chunk: the list is ascending
        if (!a.first && !(k < last && a.adj[k] < a.key_hi)) continue;  // nothing of this chunk: the entry stays as it is
        double f = a.first ? 0.0 : a.out[i];
        for (; k < last; ++k) {
            const long long key = a.adj[k];
            if (key >= a.key_hi) break;
            f = f + a.de[(key - a.key_lo) * DD + rs];
        }
        a.out[i] = f;
    }
}
