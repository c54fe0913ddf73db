// Preconditioned conjugate gradients on the assembled tangent stiffness (solver.py: ConjugateGradient): K x = b solved on the
// device, K the values a TangentMatrix wrote (block CSR or scalar CSR over the same pattern).  Read at run time and compiled with
// hiprtc behind the generated definitions:
//   FCAMD_CG_D        dofs per node: 1, 2 or 3 (the blocks are D x D); 6 for the rigid-body coarse levels of multilevel_rigid.hip
//   FCAMD_CG_PRECOND  1: z = M^-1 r with the inverses of the nodes' own blocks (block-Jacobi); 0: z is r and rz is rr; 2: z and rz
//                     come from outside (multilevel.hip: the cycle's kernels and its closing kernel run between the update and
//                     the direction kernel); the update kernel forms neither
//   FCAMD_CG_SLAB     doubles of values a wave holds in its LDS region at a time (a multiple of 128)
//
// Five kernels, 256-thread blocks, all on one stream; every one reads what it needs from the Control block in device memory and
// returns at once when the status there is not "running", so launches enqueued behind the end of a solve do nothing.
//
// The ordered dot (every dot of the solver, fused or not).  The vector is cut into segments of kSeg = 3072 consecutive entries
// (divisible by 1, 2 and 3: a segment holds whole nodes).  A block takes a segment at a time (grid-stride loop); thread t forms
//   acc = 0.0;  acc = acc + a[e] * b[e]  over  e = seg * kSeg + t + 256 i,  i = 0 .. 11 ascending  (entries past the end: skipped)
// the 256 values are added by the tree  red[t] = red[t] + red[t + h],  h = 128, 64, .., 1,  and red[0] goes to partials[seg].
// A block that has written its partials passes a __threadfence() and adds one to an integer counter; the block that finds the
// counter at gridDim.x - 1 is the last: it resets the counter, forms  acc = 0.0;  acc = acc + partials[t + 256 i], i ascending
// over all segments, and the same tree, once.  The result depends on the vector alone, not on the grid, the CU count or the run.
//
// Matrix-vector kernel: q = K p and the segment partials of p.q.  Scalar row e = D v + r is
//   q[e] = 0.0;  q[e] = q[e] + value(k, r, s) * p[D * indices[k] + s]   over k = indptr[v] .. indptr[v + 1] ascending, s ascending
// with value(k, r, s) at D*D*k + D*r + s (block CSR) or D*D*indptr[v] + r*D*nb + D*(k - indptr[v]) + s (scalar CSR, nb the blocks
// of the row): the dest_base / dest_stride pair of matrix.py, recomputed from indptr so that only the values and the column
// indices stream.  Thread t of the block of a segment owns the rows e = seg * kSeg + t + 256 i -- the lane order of the dot, so
// p[e] * q[e] is added as the rows complete.  For one i a wave owns 64 consecutive rows, whose values are ONE contiguous range of
// the array in either format; the wave walks that range linearly in slabs of FCAMD_CG_SLAB doubles that start on multiples of 6
// (the 16-byte grid, and no run of D values straddles two slabs): coalesced 16-byte non-temporal loads into registers, all issued
// before the first is stored to the wave's LDS region; then the wave forms the products together, a lane per run of D values
// (one row of one block: one column index, D gathered entries of p), each product rounded and left where its value lay; then
// every lane whose chain has entries inside the slab goes on adding them from LDS in the chain's order.  The column index of a
// run is indices[g / D] in block CSR (g the run's number in the array) and comes from a table of one int per run in scalar CSR.
// The values are read once (the rows of a node split between two waves share their range in block CSR: those are read twice).
//
// Update kernel (mode "start": r = b - q or b, z, p = z, the partials of r.r, r.z and b.b; mode "iterate": alpha = rz / pq,
// x = x + alpha * p, r = r - alpha * q, z = M^-1 r, the partials of r.r and r.z), a segment per block at a time: the new r passes
// through LDS so that z[D v + r] = 0.0; z = z + inv[v][r][s] * r_[D v + s], s ascending, reads the node's other entries.  Its last
// block ends the iteration: counts it, rr <= thr2 -> converged, a non-finite rr -> nonfinite, the count at maxiter -> maxiter.
// Direction kernel: beta = rz / rz_old, p = z + beta * p.  Inverse kernel: the explicit inverses of the nodes' own blocks, once
// per solve; a zero or non-finite determinant sets the status singular_block.  D = 6: Gauss-Jordan in place, in registers, pivots
// in the order 0 .. 5 without a search: p = m[k][k]; m[k][k] = 1.0; m[k][j] = m[k][j] / p, j ascending; then for the rows i != k
// ascending: f = m[i][k]; m[i][k] = 0.0; m[i][j] = m[i][j] - f * m[k][j], j ascending; a zero or non-finite pivot sets
// singular_block.  Dot kernel: the ordered dot of two vectors.
// No floating-point atomics, no MFMA; every product is rounded before its sum (-ffp-contract=off); division is a division.
#pragma once
#include "tile_io.h"

namespace fcamd_cg {
using namespace fcamd;

constexpr int D = FCAMD_CG_D, DD = D * D;
constexpr bool kPrecond = FCAMD_CG_PRECOND == 1;
constexpr bool kExternal = FCAMD_CG_PRECOND == 2;
constexpr int kSeg = 3072;
constexpr int kPerLane = kSeg / kBlock;  // 12
constexpr int kSlab = FCAMD_CG_SLAB;
constexpr int kChunks = kSlab / (2 * kWave);  // 16-byte loads of a lane per slab
constexpr int kGrid = 6;                      // slabs start on multiples of 2 (16 bytes) and of D: a run of D values never straddles
constexpr int kStep = kSlab / kGrid * kGrid;  // doubles of a slab that are used
static_assert(((D >= 1 && D <= 3) || D == 6) && kSeg % D == 0 && kSeg % kBlock == 0, "shape");
static_assert(kSlab % (2 * kWave) == 0 && kSlab >= 2 * kWave, "slab");
// solver.py (lds_bytes, LDS_CAP) refuses such a slab before it gets here
static_assert((kWavesPerBlock * kSlab + kBlock + 2) * 8 <= 64 * 1024, "slab too large for the LDS of a block");

enum Status : int { kRunning = 0, kConverged = 1, kMaxiter = 2, kIndefinite = 3, kSingular = 4, kNonfinite = 5 };
enum Mode : int { kStart = 0, kIterate = 1, kPlain = 2, kQuiet = 3 };

// the control block in device memory; solver.py mirrors the layout
struct Control {
    double rr, bb;  // with the four ints: the 32 bytes the host reads at a look
    int status, iterations, maxiter;
    unsigned int counter;
    double rz, rz_old, pq, thr2, rtol, atol, dot, spare;
};

// the only parameter of every kernel; solver.py mirrors the layout
struct Args {
    const double* values;
    const int* indptr;   // [n_nodes + 1]
    const int* indices;  // [nnzb]
    const int* diag;     // [n_nodes] the node's own block
    const int* groups;   // scalar CSR: [D * nnzb] the node of the columns of the values D g .. D g + D - 1
    const double* b;
    double* x;
    double* r;
    double* z;
    double* p;
    double* q;
    double* inv;          // [n_nodes][D][D]
    const double* va;     // the product's vector; the dot's first
    const double* vb;     // the dot's second
    double* partials;     // [3][nseg]
    Control* sc;
    long long n;          // D * n_nodes
    long long nnz;        // D * D * nnzb
    long long nseg;
    long long n_nodes;
    int csr;              // 1: scalar CSR, 0: block CSR
    int mode;
    int has_x0;
    int pad;
};

// red[0 .. 255]: the tree; red[256]: the last-block flag
__device__ __forceinline__ double block_tree(double acc, double* red, int t) {
    red[t] = acc;
    __syncthreads();
#pragma unroll
    for (int h = kBlock / 2; h >= 1; h >>= 1) {
        if (t < h) red[t] = red[t] + red[t + h];
        __syncthreads();
    }
    const double total = red[0];
    __syncthreads();
    return total;
}

// true in every thread of the block that finishes last (its partials and everyone else's are visible to it)
__device__ __forceinline__ bool last_block(Control* sc, double* red, int t) {
    if (t == 0) {
        __threadfence();
        const unsigned int done = atomicAdd(&sc->counter, 1u);
        const bool last = done == gridDim.x - 1u;
        if (last) atomicExch(&sc->counter, 0u);
        red[kBlock] = last ? 1.0 : 0.0;
    }
    __syncthreads();
    const bool last = red[kBlock] != 0.0;
    __syncthreads();
    if (last) __threadfence();
    return last;
}

__device__ __forceinline__ double final_sum(const double* partials, long long nseg, double* red, int t) {
    const volatile double* part = partials;
    double acc = 0.0;
    for (long long s = t; s < nseg; s += kBlock) acc = acc + part[s];
    return block_tree(acc, red, t);
}

// the rows g0 .. g0 + live - 1 (live <= 64) of q = K va, the lane's row returned (lanes past `live`: nothing)
__device__ __forceinline__ double wave_rows(const Args& a, double* region, long long g0, int live, int lane) {
    const bool on = lane < live;
    const long long e = g0 + (on ? lane : live - 1);
    const long long v = e / D;
    const int r = (int)(e - v * D);
    const int k0 = a.indptr[v];
    const int nb = a.indptr[v + 1] - k0;
    // (a row without blocks sits at its block row's start in both formats: after the last block that is nnz, never past it)
    const long long rowbase = (a.csr || nb == 0) ? (long long)DD * k0 + (long long)r * D * nb : (long long)DD * k0 + D * r;
    const int kstep = a.csr ? D : DD;
    const long long end = nb > 0 ? rowbase + (long long)(nb - 1) * kstep + D : rowbase;
    long long lo = rowbase, hi = end;
#pragma unroll
    for (int off = kWave / 2; off >= 1; off >>= 1) {
        const long long lo2 = __shfl_xor(lo, off, kWave), hi2 = __shfl_xor(hi, off, kWave);
        lo = lo2 < lo ? lo2 : lo;
        hi = hi2 > hi ? hi2 : hi;
    }
    hi = hi < a.nnz ? hi : a.nnz;  // (it is: the end of a row's last block)
    lo = lo / kGrid * kGrid;       // the 16-byte grid and the blocks' grid at once
    double acc = 0.0;
    int j = 0;
    long long pos = rowbase;
#pragma unroll 1
    for (long long cur = lo; cur < hi; cur += kStep) {
        d2 c[kChunks];
#pragma unroll
        for (int k = 0; k < kChunks; ++k) {
            const long long idx = cur + 2 * (k * kWave + lane);
            c[k].x = 0.0;
            c[k].y = 0.0;
            if (idx < hi) {
                if (idx + 1 < a.nnz)
                    c[k] = load16<true>(a.values + idx);
                else
                    c[k].x = __builtin_nontemporal_load(a.values + idx);
            }
        }
#pragma unroll
        for (int k = 0; k < kChunks; ++k) reinterpret_cast<d2*>(region)[k * kWave + lane] = c[k];
        wave_sync();
        // the products, the wave together: a lane per run of D values (one row of one block), each rounded where it lies
#pragma unroll 2
        for (int gi = lane; gi < kStep / D; gi += kWave) {
            const long long p0 = cur + (long long)D * gi;
            if (p0 < hi) {
                const long long g = p0 / D;
                const int col = a.csr ? a.groups[g] : a.indices[g / D];
                const double* pv = a.va + (long long)D * col;
                double* val = region + D * gi;
#pragma unroll
                for (int s = 0; s < D; ++s) val[s] = val[s] * pv[s];
            }
        }
        wave_sync();
        // the sums: every lane goes on with the chain of its row
        const long long slab_end = cur + kStep;
        if (on) {
            while (j < nb && pos < slab_end) {
                const double* val = region + (pos - cur);
#pragma unroll
                for (int s = 0; s < D; ++s) acc = acc + val[s];
                ++j;
                pos += kstep;
            }
        }
        wave_sync();
    }
    return acc;
}

}  // namespace fcamd_cg

// q = K va; mode kIterate: the status is honoured and pq <= 0 (or NaN) ends the solve; kPlain: the product and sc->dot = va . q;
// kQuiet: the status is honoured and the product is all (no dot, no counter: the products of the multilevel cycle)
extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_cg_matvec_kernel(const fcamd_cg::Args a) {
    using namespace fcamd_cg;
    __shared__ __attribute__((aligned(16))) double slab[kWavesPerBlock][kSlab];
    __shared__ double red[kBlock + 2];
    Control* sc = a.sc;
    if (a.mode == kIterate && sc->status != kRunning) return;
    if (a.mode == kQuiet && sc->status != kRunning) return;
    const int t = (int)threadIdx.x;
    const int lane = t & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(t / kWave);
    for (long long seg = blockIdx.x; seg < a.nseg; seg += gridDim.x) {
        double acc = 0.0;
#pragma unroll 1
        for (int i = 0; i < kPerLane; ++i) {
            const long long g0 = seg * kSeg + (long long)i * kBlock + wave * kWave;
            if (g0 >= a.n) break;  // (the same for the whole wave)
            const long long left = a.n - g0;
            const int live = left < kWave ? (int)left : kWave;
            const double qv = wave_rows(a, slab[wave], g0, live, lane);
            if (lane < live) {
                a.q[g0 + lane] = qv;
                acc = acc + a.va[g0 + lane] * qv;
            }
        }
        if (a.mode == kQuiet) continue;  // (the same for the whole grid: no tree, no partial)
        const double total = block_tree(acc, red, t);
        if (t == 0) a.partials[seg] = total;
    }
    if (a.mode == kQuiet) return;
    if (last_block(sc, red, t)) {
        const double pq = final_sum(a.partials, a.nseg, red, t);
        if (t == 0) {
            if (a.mode == kIterate) {
                sc->pq = pq;
                if (!(pq > 0.0)) sc->status = kIndefinite;
            } else {
                sc->dot = pq;
            }
        }
    }
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_cg_update_kernel(const fcamd_cg::Args a) {
    using namespace fcamd_cg;
    __shared__ double rs[kSeg];
    __shared__ double red[kBlock + 2];
    Control* sc = a.sc;
    const bool start = a.mode == kStart;
    if (!start && sc->status != kRunning) return;
    const int t = (int)threadIdx.x;
    const double alpha = start ? 0.0 : sc->rz / sc->pq;
    for (long long seg = blockIdx.x; seg < a.nseg; seg += gridDim.x) {
        const long long base = seg * kSeg;
        double arr = 0.0, arz = 0.0, abb = 0.0;
#pragma unroll 1
        for (int i = 0; i < kPerLane; ++i) {
            const int l = t + kBlock * i;
            const long long e = base + l;
            if (e < a.n) {
                double rn;
                if (start) {
                    const double be = a.b[e];
                    rn = be;
                    if (a.has_x0) rn = be - a.q[e];
                    abb = abb + be * be;
                    if (!kPrecond && !kExternal) a.p[e] = rn;
                } else {
                    a.x[e] = a.x[e] + alpha * a.p[e];
                    rn = a.r[e] - alpha * a.q[e];
                }
                a.r[e] = rn;
                rs[l] = rn;
                arr = arr + rn * rn;
            }
        }
        if constexpr (kPrecond) {
            __syncthreads();
#pragma unroll 1
            for (int i = 0; i < kPerLane; ++i) {
                const int l = t + kBlock * i;
                const long long e = base + l;
                if (e < a.n) {
                    const int node = l / D;
                    const double* m = a.inv + (long long)D * e;  // inv[v][r][.]
                    double z = 0.0;
#pragma unroll
                    for (int s = 0; s < D; ++s) z = z + m[s] * rs[node * D + s];
                    a.z[e] = z;
                    if (start) a.p[e] = z;
                    arz = arz + rs[l] * z;
                }
            }
            __syncthreads();
        }
        const double rr = block_tree(arr, red, t);
        if (t == 0) a.partials[seg] = rr;
        if constexpr (kPrecond) {
            const double rz = block_tree(arz, red, t);
            if (t == 0) a.partials[a.nseg + seg] = rz;
        }
        if (start) {
            const double bb = block_tree(abb, red, t);
            if (t == 0) a.partials[2 * a.nseg + seg] = bb;
        }
    }
    if (last_block(sc, red, t)) {
        const double rr = final_sum(a.partials, a.nseg, red, t);
        double rz = rr;
        if constexpr (kPrecond) rz = final_sum(a.partials + a.nseg, a.nseg, red, t);
        double bb = 0.0;
        if (start) bb = final_sum(a.partials + 2 * a.nseg, a.nseg, red, t);
        if (t == 0) {
            sc->rr = rr;
            if (start) {
                const double r2 = sc->rtol * sc->rtol * bb, a2 = sc->atol * sc->atol;
                sc->bb = bb;
                sc->thr2 = r2 > a2 ? r2 : a2;
                if (!kExternal) sc->rz = rz;
            } else {
                if (!kExternal) {
                    sc->rz_old = sc->rz;
                    sc->rz = rz;
                }
                sc->iterations = sc->iterations + 1;
            }
            if (sc->status == kRunning) {
                if (rr <= sc->thr2)
                    sc->status = kConverged;
                else if (!__builtin_isfinite(rr))
                    sc->status = kNonfinite;
                else if (sc->iterations >= sc->maxiter)
                    sc->status = kMaxiter;
            }
        }
    }
}

// p = z + beta * p (z is r without the preconditioner)
extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_cg_direction_kernel(const fcamd_cg::Args a) {
    using namespace fcamd_cg;
    const Control* sc = a.sc;
    if (sc->status != kRunning) return;
    const double beta = sc->rz / sc->rz_old;
    const double* z = (kPrecond || kExternal) ? a.z : a.r;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < a.n; e += stride) a.p[e] = z[e] + beta * a.p[e];
}

// inv[v] = (the node's own block)^-1 by the explicit formulas, a lane per node
extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_cg_inverse_kernel(const fcamd_cg::Args a) {
    using namespace fcamd_cg;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < a.n_nodes; v += stride) {
        const int k = a.diag[v];
        const int k0 = a.indptr[v];
        const int nb = a.indptr[v + 1] - k0;
        const long long base = a.csr ? (long long)DD * k0 + (long long)D * (k - k0) : (long long)DD * k;
        const long long rstride = a.csr ? (long long)D * nb : D;
        double m[D][D];
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int s = 0; s < D; ++s) m[r][s] = a.values[base + r * rstride + s];
        double* inv = a.inv + DD * v;
        double det;
        if constexpr (D == 6) {
            det = 1.0;  // (stands for the pivots: 0.0 once one of them is zero or not finite)
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double p = m[k][k];
                if (!(p != 0.0) || !__builtin_isfinite(p)) det = 0.0;
                m[k][k] = 1.0;
#pragma unroll
                for (int j = 0; j < 6; ++j) m[k][j] = m[k][j] / p;
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    if (i == k) continue;
                    const double f = m[i][k];
                    m[i][k] = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; ++j) m[i][j] = m[i][j] - f * m[k][j];
                }
            }
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = 0; j < 6; ++j) inv[6 * i + j] = m[i][j];
        } else if constexpr (D == 1) {
            det = m[0][0];
            inv[0] = 1.0 / det;
        } else if constexpr (D == 2) {
            det = m[0][0] * m[1][1] - m[0][1] * m[1][0];
            inv[0] = m[1][1] / det;
            inv[1] = -m[0][1] / det;
            inv[2] = -m[1][0] / det;
            inv[3] = m[0][0] / det;
        } else {
            double c[3][3];
            c[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1];
            c[0][1] = m[1][2] * m[2][0] - m[1][0] * m[2][2];
            c[0][2] = m[1][0] * m[2][1] - m[1][1] * m[2][0];
            c[1][0] = m[0][2] * m[2][1] - m[0][1] * m[2][2];
            c[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0];
            c[1][2] = m[0][1] * m[2][0] - m[0][0] * m[2][1];
            c[2][0] = m[0][1] * m[1][2] - m[0][2] * m[1][1];
            c[2][1] = m[0][2] * m[1][0] - m[0][0] * m[1][2];
            c[2][2] = m[0][0] * m[1][1] - m[0][1] * m[1][0];
            det = m[0][0] * c[0][0] + m[0][1] * c[0][1] + m[0][2] * c[0][2];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) inv[3 * i + j] = c[j][i] / det;
        }
        if (!(det != 0.0) || !__builtin_isfinite(det)) a.sc->status = kSingular;
    }
}

// sc->dot = va . vb in the fixed order
extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_cg_dot_kernel(const fcamd_cg::Args a) {
    using namespace fcamd_cg;
    __shared__ double red[kBlock + 2];
    const int t = (int)threadIdx.x;
    for (long long seg = blockIdx.x; seg < a.nseg; seg += gridDim.x) {
        double acc = 0.0;
#pragma unroll 1
        for (int i = 0; i < kPerLane; ++i) {
            const long long e = seg * kSeg + t + (long long)kBlock * i;
            if (e < a.n) acc = acc + a.va[e] * a.vb[e];
        }
        const double total = block_tree(acc, red, t);
        if (t == 0) a.partials[seg] = total;
    }
    if (last_block(a.sc, red, t)) {
        const double total = final_sum(a.partials, a.nseg, red, t);
        if (t == 0) a.sc->dot = total;
    }
}
