// Right-preconditioned BiCGStab on the assembled tangent stiffness (bicgstab.py: BiCGStab): K x = b for a K that need not be
// symmetric, K the values a TangentMatrix wrote.  Read at run time and compiled with hiprtc behind the definitions of
// conjugate_gradient.hip -- FCAMD_CG_D, FCAMD_CG_PRECOND (0: y is p and z is s; 1: y = M^-1 p and z = M^-1 s with the inverses of
// the nodes' own blocks; 2: y and z come from outside, the multilevel cycle's launches run between the kernels) and FCAMD_CG_SLAB.
// The program holds that file's kernels too: its matrix-vector kernel forms K x0, its inverse kernel the block inverses, and the
// pieces of the ordered dot (wave_rows, block_tree, last_block, final_sum) are used as they stand there.
//
// Five kernels, 256-thread blocks, all on one stream; every one but the start returns at once when the status of the control
// block is not "running".  One iteration is  product("v"), half step, product("t"), full step, direction:
//   product   q = K va by wave_rows (the segment, wave and slab walk of fcamd_cg_matvec_kernel) and, added in the dot's lane order
//             as the rows complete, the partials of q . vb ("v": q is v, vb is rhat) or of q . vb and q . q ("t": q is t, vb is
//             s), two trees one after the other on the same array.  Its last block writes rv, or ts, tt and omega = ts / tt; a
//             zero or non-finite rv, tt or omega: status breakdown.
//   start     r = b - q (q = K x0) or b, rhat = r, p = r, y = M^-1 p (block-Jacobi), the partials of r . r and b . b; the last
//             block: rr, bb, thr2, rho = rr and the status of a solve that ends at its start.
//   half      alpha = rho / rv; x = x + alpha * y; s = r - alpha * v written over r; z = M^-1 s through LDS (block-Jacobi); the
//             partials of s . s.  Its last block: rr = ss, alpha for the direction kernel; ss <= thr2: counted, converged.
//   full      x = x + omega * z; r = s - omega * t; the partials of r . r and rhat . r.  Its last block ends the iteration:
//             rr, rho_old = rho, rho = rhat . r, the count; rr <= thr2: converged, else a non-finite rr: nonfinite, else a zero or
//             non-finite rho: breakdown, else the count at maxiter: maxiter.
//   direction beta = (rho / rho_old) * (alpha / omega); p = r + beta * (p - omega * v); y = M^-1 p (block-Jacobi: every lane forms
//             the D entries of its node in registers, a barrier between the loads of the old p and the stores of the new).
// A scalar the lanes of a kernel read (rho, rv, alpha's and omega's operands) is never written by a block of the same kernel.
// No floating-point atomics, no MFMA; every product is rounded before its sum (-ffp-contract=off); division is a division.
#pragma once
#include "conjugate_gradient.hip"

namespace fcamd_bcg {
using namespace fcamd_cg;

constexpr int kBreakdown = 6;        // behind the statuses of fcamd_cg::Status
constexpr int kChunk = 3 * kBlock;   // entries of a block's trip in the direction kernel: whole nodes for D = 1, 2, 3
enum Dots : int { kDotV = 0, kDotT = 1 };

// the control block in device memory; bicgstab.py mirrors the layout.  The first 32 bytes, thr2, rtol, atol and dot lie where
// fcamd_cg::Control has them: the host's look, the multilevel kernels' status test and the kernels of conjugate_gradient.hip
// work on it unchanged.
struct Block {
    double rr, bb;
    int status, iterations, maxiter;
    unsigned int counter;
    double rho, rho_old, rv, thr2, rtol, atol, dot, ts, tt, alpha, omega, spare;
};
static_assert(__builtin_offsetof(Block, status) == __builtin_offsetof(Control, status) && __builtin_offsetof(Block, counter) == __builtin_offsetof(Control, counter) &&
                  __builtin_offsetof(Block, thr2) == __builtin_offsetof(Control, thr2) && __builtin_offsetof(Block, rtol) == __builtin_offsetof(Control, rtol) &&
                  __builtin_offsetof(Block, atol) == __builtin_offsetof(Control, atol) && __builtin_offsetof(Block, dot) == __builtin_offsetof(Control, dot),
              "the control block's shared part");

// the only parameter of every kernel here; bicgstab.py mirrors the layout
struct Params {
    Args cg;       // the matrix, b, x, r (s is written over it), z, p, inv, the partials and the control block; q: the product's
                   // output (the start: K x0); va: the product's vector; vb: the product's dot vector; mode: Dots
    double* rhat;
    double* v;
    double* t;
    double* y;     // p itself without a preconditioner (as cg.z is r)
};

__device__ __forceinline__ Block* scalars(const Params& a) { return reinterpret_cast<Block*>(a.cg.sc); }
__device__ __forceinline__ bool unusable(double d) { return !(d != 0.0) || !__builtin_isfinite(d); }

}  // namespace fcamd_bcg

// q = K va and the ordered q . vb (kDotV: into rv) or q . vb and q . q (kDotT: into ts and tt, omega = ts / tt)
extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_bcg_product_kernel(const fcamd_bcg::Params a) {
    using namespace fcamd_bcg;
    __shared__ __attribute__((aligned(16))) double slab[kWavesPerBlock][kSlab];
    __shared__ double red[kBlock + 2];
    Block* sc = scalars(a);
    if (sc->status != kRunning) return;
    const bool both = a.cg.mode == kDotT;
    const int t = (int)threadIdx.x;
    const int lane = t & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(t / kWave);
    for (long long seg = blockIdx.x; seg < a.cg.nseg; seg += gridDim.x) {
        double acc = 0.0, acc2 = 0.0;
#pragma unroll 1
        for (int i = 0; i < kPerLane; ++i) {
            const long long g0 = seg * kSeg + (long long)i * kBlock + wave * kWave;
            if (g0 >= a.cg.n) break;  // (the same for the whole wave)
            const long long left = a.cg.n - g0;
            const int live = left < kWave ? (int)left : kWave;
            const double qv = wave_rows(a.cg, slab[wave], g0, live, lane);
            if (lane < live) {
                a.cg.q[g0 + lane] = qv;
                acc = acc + qv * a.cg.vb[g0 + lane];
                if (both) acc2 = acc2 + qv * qv;
            }
        }
        const double total = block_tree(acc, red, t);
        if (t == 0) a.cg.partials[seg] = total;
        if (both) {  // (the same for the whole grid)
            const double total2 = block_tree(acc2, red, t);
            if (t == 0) a.cg.partials[a.cg.nseg + seg] = total2;
        }
    }
    if (last_block(a.cg.sc, red, t)) {
        const double first = final_sum(a.cg.partials, a.cg.nseg, red, t);
        double second = 0.0;
        if (both) second = final_sum(a.cg.partials + a.cg.nseg, a.cg.nseg, red, t);
        if (t == 0) {
            if (both) {
                const double omega = first / second;
                sc->ts = first;
                sc->tt = second;
                sc->omega = omega;
                if (unusable(second) || unusable(omega)) sc->status = kBreakdown;
            } else {
                sc->rv = first;
                if (unusable(first)) sc->status = kBreakdown;
            }
        }
    }
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_bcg_start_kernel(const fcamd_bcg::Params a) {
    using namespace fcamd_bcg;
    __shared__ double red[kBlock + 2];
    Block* sc = scalars(a);
    const int t = (int)threadIdx.x;
    for (long long seg = blockIdx.x; seg < a.cg.nseg; seg += gridDim.x) {
        double arr = 0.0, abb = 0.0;
#pragma unroll 1
        for (int i = 0; i < kPerLane; ++i) {
            const long long e = seg * kSeg + t + (long long)kBlock * i;
            if (e < a.cg.n) {
                const double be = a.cg.b[e];
                double rn = be;
                if (a.cg.has_x0) rn = be - a.cg.q[e];
                abb = abb + be * be;
                a.cg.r[e] = rn;
                a.rhat[e] = rn;
                a.cg.p[e] = rn;
                arr = arr + rn * rn;
                if constexpr (kPrecond) {
                    const long long v = e / D;
                    const double* m = a.cg.inv + (long long)D * e;  // inv[v][r][.]
                    double y = 0.0;
#pragma unroll
                    for (int s = 0; s < D; ++s) {
                        const long long g = v * D + s;
                        double d = a.cg.b[g];
                        if (a.cg.has_x0) d = d - a.cg.q[g];
                        y = y + m[s] * d;
                    }
                    a.y[e] = y;
                }
            }
        }
        const double rr = block_tree(arr, red, t);
        if (t == 0) a.cg.partials[seg] = rr;
        const double bb = block_tree(abb, red, t);
        if (t == 0) a.cg.partials[a.cg.nseg + seg] = bb;
    }
    if (last_block(a.cg.sc, red, t)) {
        const double rr = final_sum(a.cg.partials, a.cg.nseg, red, t);
        const double bb = final_sum(a.cg.partials + a.cg.nseg, a.cg.nseg, red, t);
        if (t == 0) {
            const double r2 = sc->rtol * sc->rtol * bb, a2 = sc->atol * sc->atol;
            sc->rr = rr;
            sc->bb = bb;
            sc->thr2 = r2 > a2 ? r2 : a2;
            sc->rho = rr;
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

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_bcg_half_kernel(const fcamd_bcg::Params a) {
    using namespace fcamd_bcg;
    __shared__ double rs[kSeg];
    __shared__ double red[kBlock + 2];
    Block* sc = scalars(a);
    if (sc->status != kRunning) return;
    const int t = (int)threadIdx.x;
    const double alpha = sc->rho / sc->rv;
    for (long long seg = blockIdx.x; seg < a.cg.nseg; seg += gridDim.x) {
        const long long base = seg * kSeg;
        double ass = 0.0;
#pragma unroll 1
        for (int i = 0; i < kPerLane; ++i) {
            const int l = t + kBlock * i;
            const long long e = base + l;
            if (e < a.cg.n) {
                a.cg.x[e] = a.cg.x[e] + alpha * a.y[e];
                const double sn = a.cg.r[e] - alpha * a.v[e];
                a.cg.r[e] = sn;
                if constexpr (kPrecond) rs[l] = sn;
                ass = ass + sn * sn;
            }
        }
        if constexpr (kPrecond) {
            __syncthreads();
#pragma unroll 1
            for (int i = 0; i < kPerLane; ++i) {
                const int l = t + kBlock * i;
                const long long e = base + l;
                if (e < a.cg.n) {
                    const int node = l / D;
                    const double* m = a.cg.inv + (long long)D * e;  // inv[v][r][.]
                    double z = 0.0;
#pragma unroll
                    for (int s = 0; s < D; ++s) z = z + m[s] * rs[node * D + s];
                    a.cg.z[e] = z;
                }
            }
            __syncthreads();
        }
        const double ss = block_tree(ass, red, t);
        if (t == 0) a.cg.partials[seg] = ss;
    }
    if (last_block(a.cg.sc, red, t)) {
        const double ss = final_sum(a.cg.partials, a.cg.nseg, red, t);
        if (t == 0) {
            sc->rr = ss;
            sc->alpha = alpha;
            if (ss <= sc->thr2) {
                sc->iterations = sc->iterations + 1;
                sc->status = kConverged;
            }
        }
    }
}

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_bcg_full_kernel(const fcamd_bcg::Params a) {
    using namespace fcamd_bcg;
    __shared__ double red[kBlock + 2];
    Block* sc = scalars(a);
    if (sc->status != kRunning) return;
    const int t = (int)threadIdx.x;
    const double omega = sc->omega;
    for (long long seg = blockIdx.x; seg < a.cg.nseg; seg += gridDim.x) {
        double arr = 0.0, arh = 0.0;
#pragma unroll 1
        for (int i = 0; i < kPerLane; ++i) {
            const long long e = seg * kSeg + t + (long long)kBlock * i;
            if (e < a.cg.n) {
                a.cg.x[e] = a.cg.x[e] + omega * a.cg.z[e];
                const double rn = a.cg.r[e] - omega * a.t[e];
                a.cg.r[e] = rn;
                arr = arr + rn * rn;
                arh = arh + a.rhat[e] * rn;
            }
        }
        const double rr = block_tree(arr, red, t);
        if (t == 0) a.cg.partials[seg] = rr;
        const double rh = block_tree(arh, red, t);
        if (t == 0) a.cg.partials[a.cg.nseg + seg] = rh;
    }
    if (last_block(a.cg.sc, red, t)) {
        const double rr = final_sum(a.cg.partials, a.cg.nseg, red, t);
        const double rho = final_sum(a.cg.partials + a.cg.nseg, a.cg.nseg, red, t);
        if (t == 0) {
            sc->rr = rr;
            sc->rho_old = sc->rho;
            sc->rho = rho;
            sc->iterations = sc->iterations + 1;
            if (rr <= sc->thr2)
                sc->status = kConverged;
            else if (!__builtin_isfinite(rr))
                sc->status = kNonfinite;
            else if (unusable(rho))
                sc->status = kBreakdown;
            else if (sc->iterations >= sc->maxiter)
                sc->status = kMaxiter;
        }
    }
}

// p = r + beta * (p - omega * v); block-Jacobi: y = M^-1 p, else y is p (or comes from the multilevel cycle)
extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_bcg_direction_kernel(const fcamd_bcg::Params a) {
    using namespace fcamd_bcg;
    const Block* sc = scalars(a);
    if (sc->status != kRunning) return;
    const double beta = (sc->rho / sc->rho_old) * (sc->alpha / sc->omega);
    const double omega = sc->omega;
    if constexpr (kPrecond) {
        // a trip of kChunk entries (whole nodes) per block: every lane forms the new p at the D entries of its node from the old,
        // all lanes of the block have read the old before any stores the new
        const long long chunks = (a.cg.n + kChunk - 1) / kChunk;
        for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
            double pn[kChunk / kBlock], y[kChunk / kBlock];
#pragma unroll
            for (int i = 0; i < kChunk / kBlock; ++i) {
                const long long e = c * kChunk + threadIdx.x + (long long)kBlock * i;
                pn[i] = 0.0;
                y[i] = 0.0;
                if (e < a.cg.n) {
                    const long long v = e / D;
                    const int own = (int)(e - v * D);
                    const double* m = a.cg.inv + (long long)D * e;  // inv[v][r][.]
#pragma unroll
                    for (int s = 0; s < D; ++s) {
                        const long long g = v * D + s;
                        const double pg = a.cg.r[g] + beta * (a.cg.p[g] - omega * a.v[g]);
                        if (s == own) pn[i] = pg;
                        y[i] = y[i] + m[s] * pg;
                    }
                }
            }
            if constexpr (D > 1) __syncthreads();
#pragma unroll
            for (int i = 0; i < kChunk / kBlock; ++i) {
                const long long e = c * kChunk + threadIdx.x + (long long)kBlock * i;
                if (e < a.cg.n) {
                    a.cg.p[e] = pn[i];
                    a.y[e] = y[i];
                }
            }  // (the next trip's chunk shares no node with this one)
        }
    } else {
        // two entries per lane, 16-byte loads and stores (the work vectors start on the 16-byte grid); an odd last entry alone
        const long long pairs = a.cg.n / 2;
        const long long stride = (long long)gridDim.x * kBlock;
        const long long first = (long long)blockIdx.x * kBlock + threadIdx.x;
        for (long long j = first; j < pairs; j += stride) {
            const d2 rv = load16<false>(a.cg.r + 2 * j), pv = load16<false>(a.cg.p + 2 * j), vv = load16<false>(a.v + 2 * j);
            d2 pn;
            pn.x = rv.x + beta * (pv.x - omega * vv.x);
            pn.y = rv.y + beta * (pv.y - omega * vv.y);
            store16<false>(a.cg.p + 2 * j, pn);
        }
        if (first == 0 && (a.cg.n & 1)) {
            const long long e = a.cg.n - 1;
            a.cg.p[e] = a.cg.r[e] + beta * (a.cg.p[e] - omega * a.v[e]);
        }
    }
}
