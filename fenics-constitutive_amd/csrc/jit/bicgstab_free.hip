// BiCGStab on the matrix-free tangent operator (bicgstab_free.py: MatrixFreeBiCGStab): the product q = A va of
// tangent_operator.hip with BiCGStab's dots behind it.  Read at run time and compiled with hiprtc as a program of its own behind
// the FCAMD_TO_* definitions of tangent_operator.hip, which sets FCAMD_CG_D, FCAMD_CG_PRECOND 0 and FCAMD_CG_SLAB and pulls in
// conjugate_gradient.hip; bicgstab.hip gives the control block (fcamd_bcg::Block), kBreakdown, unusable and Dots.  (The five
// kernels of bicgstab.hip and those of conjugate_gradient.hip are compiled along; this program launches none of them: the
// solver's start, half-step, full-step and direction kernels come from the program of bicgstab.py.)
//
// The product is two launches, one behind the other on one stream: the unchanged fcamd_tangent_operator_element_kernel in its mode
// kIterate (it reads the status alone, which lies in Block where Control has it: the static assertion of bicgstab.hip) and the one
// kernel added here.
//
// fcamd_tangent_operator_node_dots_kernel: the layout and the row of fcamd_tangent_operator_node_kernel -- 256-thread blocks, the
// block of a segment of kSeg = 3072 dofs, a grid-stride loop over the segments, thread t the dofs e = seg * 3072 + t + 256 i, i
// ascending; a constrained dof: y = va[e]; else y = 0.0; y = y + fe[adj[k] * D + r] over the node's CSR entries ascending (a node of
// no cell: 0.0); q[e] = y.  That is the lane order of fcamd_bcg_product_kernel, so what is added as the rows complete,
//   acc = acc + y * vb[e]      and with dots == kDotT      acc2 = acc2 + y * y,
// are the partials of the ordered q . vb and q . q: the tree, the second tree on the same array behind it, the second partial
// array at partials + nseg, the last block and the final sums are those of fcamd_bcg_product_kernel, and so are the statements of
// the last block: kDotV: rv = first, a zero or non-finite rv: breakdown; kDotT: ts, tt, omega = ts / tt, a zero or non-finite tt
// or omega: breakdown.  Both launches return at once when the status is not "running".  The second dot reads nothing: y is in the
// lane's register.
//
// No floating-point atomics, no MFMA; every product is rounded before its sum (-ffp-contract=off); dead lanes load nothing; index
// arithmetic is 64-bit.
#pragma once
#include "tangent_operator.hip"
#include "bicgstab.hip"

namespace fcamd_to {

// the node-dots kernel's only parameter: NodeArgs (the control pointer typed as BiCGStab's block; the mode is not read) with the
// dot vector and the dots behind it; bicgstab_free.py mirrors the layout (NodeDotsArgs)
struct NodeDotsArgs {
    const double* fe;           // [C][A][D]
    const int* node_ptr;        // [n_nodes + 1]
    const int* adj;             // entries c*A + a, ascending within a node
    const double* v;            // [D n_nodes]: va, the product's vector
    const unsigned char* mask;  // or null
    double* out;                // [D n_nodes]: q
    double* partials;           // [2 nseg] (the control block's has 3 nseg)
    fcamd_bcg::Block* sc;
    long long n_dofs;
    long long nseg;
    int mode;
    int pad;
    const double* vb;           // [D n_nodes]: the dot vector (rhat, or s)
    int dots;                   // fcamd_bcg::Dots
    int pad2;
};
static_assert(sizeof(NodeDotsArgs) == sizeof(NodeArgs) + 16 && __builtin_offsetof(NodeDotsArgs, vb) == sizeof(NodeArgs), "NodeArgs plus vb and dots");

}  // namespace fcamd_to

extern "C" __global__ void __launch_bounds__(fcamd::kBlock) fcamd_tangent_operator_node_dots_kernel(const fcamd_to::NodeDotsArgs a) {
    using namespace fcamd_to;
    __shared__ double red[kBlock + 2];
    fcamd_bcg::Block* sc = a.sc;
    if (sc->status != fcamd_cg::kRunning) return;
    const bool both = a.dots == fcamd_bcg::kDotT;
    const int t = (int)threadIdx.x;
    for (long long seg = blockIdx.x; seg < a.nseg; seg += gridDim.x) {
        double acc = 0.0, acc2 = 0.0;
#pragma unroll 1
        for (int i = 0; i < kPerLane; ++i) {
            const long long e = seg * kSeg + t + (long long)kBlock * i;
            if (e < a.n_dofs) {
                double y;
                if (a.mask == nullptr || !a.mask[e]) {
                    const long long node = e / D;
                    const int r = (int)(e - node * D);
                    y = 0.0;
                    const int last = a.node_ptr[node + 1];
                    for (int k = a.node_ptr[node]; k < last; ++k) y = y + a.fe[(long long)a.adj[k] * D + r];
                } else {
                    y = a.v[e];
                }
                a.out[e] = y;
                acc = acc + y * a.vb[e];
                if (both) acc2 = acc2 + y * y;
            }
        }
        const double total = fcamd_cg::block_tree(acc, red, t);
        if (t == 0) a.partials[seg] = total;
        if (both) {  // (the same for the whole grid)
            const double total2 = fcamd_cg::block_tree(acc2, red, t);
            if (t == 0) a.partials[a.nseg + seg] = total2;
        }
    }
    if (fcamd_cg::last_block(reinterpret_cast<fcamd_cg::Control*>(sc), red, t)) {
        const double first = fcamd_cg::final_sum(a.partials, a.nseg, red, t);
        double second = 0.0;
        if (both) second = fcamd_cg::final_sum(a.partials + a.nseg, a.nseg, red, t);
        if (t == 0) {
            if (both) {
                const double omega = first / second;
                sc->ts = first;
                sc->tt = second;
                sc->omega = omega;
                if (fcamd_bcg::unusable(second) || fcamd_bcg::unusable(omega)) sc->status = fcamd_bcg::kBreakdown;
            } else {
                sc->rv = first;
                if (fcamd_bcg::unusable(first)) sc->status = fcamd_bcg::kBreakdown;
            }
        }
    }
}
