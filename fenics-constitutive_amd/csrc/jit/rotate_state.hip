// Array-level objective-rate rotation (objective.py: JaumannRate around a law without a fused kernel): the committed stress
// and the rotated history blocks of every point, rotated by the Hughes-Winget rotation of its gradient (rotation.h) and
// written to the arrays the law then evaluates in place.  Read at run time and compiled with hiprtc behind the generated
//   FCAMD_ROT_NFIELDS                  number of history fields passed (those with a rotated block)
//   FCAMD_ROT_FIELDS(X)                X(index, name, doubles per point) for each of them
//   FCAMD_USER_ROTATE(X)               X(name, offset) for every rotated Mandel block
//   struct RotHistory                  one double array per field
//
// One thread per point, a grid-stride loop; every access of a point stays inside its own row.  A point whose spin is zero
// is copied (out of place) or left untouched (in place).
#pragma once
#include "rotation.h"

namespace fcamd_rotk {
constexpr int kBlock = 256;
constexpr int kNF = FCAMD_ROT_NFIELDS > 0 ? FCAMD_ROT_NFIELDS : 1;

// the only kernel parameter; objective.py mirrors the layout (_rotate_args_type)
struct RotateArgs {
    const double* grad;      // [9 n]
    const double* s_in;      // [6 n] committed stress (may alias s_out)
    double* s_out;           // [6 n]
    const double* h_in[kNF]; // committed history fields (may alias h_out)
    double* h_out[kNF];
    long long n;             // points
};
}  // namespace fcamd_rotk

extern "C" __global__ void __launch_bounds__(fcamd_rotk::kBlock) fcamd_rotate_state_kernel(const fcamd_rotk::RotateArgs a) {
    using namespace fcamd_rotk;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < a.n; p += stride) {
        double g[9], s[6];
        RotHistory h;
#pragma unroll
        for (int i = 0; i < 9; ++i) g[i] = a.grad[9 * p + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i] = a.s_in[6 * p + i];
#define FCAMD_X(k, name, dim) \
    _Pragma("unroll") for (int i = 0; i < (dim); ++i) h.name[i] = a.h_in[k][(dim) * p + i];
        FCAMD_ROT_FIELDS(FCAMD_X)
#undef FCAMD_X
        const bool rotated = fcamd_user_rotate(g, s, h);
        if (rotated || a.s_out != a.s_in) {
#pragma unroll
            for (int i = 0; i < 6; ++i) a.s_out[6 * p + i] = s[i];
        }
#define FCAMD_X(k, name, dim)                                                                  \
    if (rotated || a.h_out[k] != a.h_in[k]) {                                                  \
        _Pragma("unroll") for (int i = 0; i < (dim); ++i) a.h_out[k][(dim) * p + i] = h.name[i]; \
    }
        FCAMD_ROT_FIELDS(FCAMD_X)
#undef FCAMD_X
    }
}
