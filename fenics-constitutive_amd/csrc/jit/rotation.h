// Objective-rate rotation of the committed state (objective.py: JaumannRate).  From the increment's displacement gradient
// G (row-major 3x3) the incremental spin W = (G - G^T) / 2 and its Hughes-Winget rotation
//
//   R = (I - W / 2)^-1 (I + W / 2) = I + 2 / (1 + |a|^2) (A + A^2),   A = W / 2, a the axial vector of A,
//
// which rotates a symmetric tensor S to R S R^T.  The tensors here are Mandel 6-vectors [xx, yy, zz, r xy, r xz, r yz],
// r = sqrt(2); the rotation acts on them as the 6x6 matrix Q(R) of mandel_row, so no 3x3 tensor is formed (dividing the
// shear entries by r and multiplying them back does not round-trip).  A point whose spin is exactly zero is left as it is:
// hughes_winget returns false and nothing is rotated, so a symmetric G gives the unrotated law bit for bit.
//
// Used by the tile prologue of the user-law templates (user_law_tile.h, both tangent modes) behind the generated list
//   FCAMD_USER_ROTATE(X)   X(history field, offset) for every rotated Mandel block of the history
// and by the array-level kernel rotate_state.hip.  Compiled with -ffp-contract=off, like every program of the package.
#pragma once

namespace fcamd_rot {

// the Mandel index m -> tensor index pair (i, j), i <= j
__device__ __forceinline__ constexpr int mandel_i(int m) { return m < 3 ? m : (m < 5 ? 0 : 1); }
__device__ __forceinline__ constexpr int mandel_j(int m) { return m < 3 ? m : (m == 3 ? 1 : 2); }

// R of the increment gradient g (row-major); false (R untouched) when the spin is exactly zero
__device__ __forceinline__ bool hughes_winget(const double (&g)[9], double (&R)[9]) {
    // A = W / 2 = (G - G^T) / 4 = [[0, -a3, a2], [a3, 0, -a1], [-a2, a1, 0]]
    const double a1 = 0.25 * (g[7] - g[5]);
    const double a2 = 0.25 * (g[2] - g[6]);
    const double a3 = 0.25 * (g[3] - g[1]);
    if (a1 == 0.0 && a2 == 0.0 && a3 == 0.0) return false;
    const double s1 = a1 * a1, s2 = a2 * a2, s3 = a3 * a3;
    const double c = 2.0 / (1.0 + ((s1 + s2) + s3));
    // A^2 = a a^T - |a|^2 I
    R[0] = 1.0 - c * (s2 + s3);
    R[1] = c * (a1 * a2 - a3);
    R[2] = c * (a1 * a3 + a2);
    R[3] = c * (a1 * a2 + a3);
    R[4] = 1.0 - c * (s1 + s3);
    R[5] = c * (a2 * a3 - a1);
    R[6] = c * (a1 * a3 - a2);
    R[7] = c * (a2 * a3 + a1);
    R[8] = 1.0 - c * (s1 + s2);
    return true;
}

// row m of Q(R), the 6x6 matrix with Mandel(R S R^T) = Q Mandel(S) for every symmetric S.  Row m = (i, j), column n = (k, l):
//   normal m, normal n:  R_ik^2                       normal m, shear n:  r R_ik R_il
//   shear m,  normal n:  r R_ik R_jk                  shear m,  shear n:  R_ik R_jl + R_il R_jk
// Q(I) = I exactly.
__device__ __forceinline__ void mandel_row(const double (&R)[9], int m, double (&q)[6]) {
    const double r = 1.4142135623730951;  // sqrt(2), correctly rounded
    const int i = mandel_i(m), j = mandel_j(m);
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        const int k = mandel_i(n), l = mandel_j(n);
        if (m < 3 && n < 3)
            q[n] = R[3 * i + k] * R[3 * i + k];
        else if (m < 3)
            q[n] = r * (R[3 * i + k] * R[3 * i + l]);
        else if (n < 3)
            q[n] = r * (R[3 * i + k] * R[3 * j + k]);
        else
            q[n] = R[3 * i + k] * R[3 * j + l] + R[3 * i + l] * R[3 * j + k];
    }
}

// q . x[OFF, OFF + 6): an ascending-n FMA chain
template <int OFF, int N>
__device__ __forceinline__ double mandel_dot(const double (&q)[6], const double (&x)[N]) {
    static_assert(OFF >= 0 && OFF + 6 <= N, "rotated block runs past the end of its field");
    double acc = q[0] * x[OFF];
#pragma unroll
    for (int n = 1; n < 6; ++n) acc = __builtin_fma(q[n], x[OFF + n], acc);
    return acc;
}

}  // namespace fcamd_rot

#ifdef FCAMD_USER_ROTATE
// the committed stress and the listed history blocks of one point, rotated in registers before the law sees them; false
// (nothing changed) when the spin is zero.  Q is formed one row at a time and applied to every block at once: only R, one row
// and the blocks' results are live (the whole Q would take 72 VGPRs)
template <class H>
__device__ __forceinline__ bool fcamd_user_rotate(const double (&g)[9], double (&s)[6], H& h) {
    double R[9];
    if (!fcamd_rot::hughes_winget(g, R)) return false;
    double ys[6];
#define FCAMD_X(name, off) double y_##name##_##off[6];
    FCAMD_USER_ROTATE(FCAMD_X)
#undef FCAMD_X
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        double q[6];
        fcamd_rot::mandel_row(R, m, q);
        ys[m] = fcamd_rot::mandel_dot<0>(q, s);
#define FCAMD_X(name, off) y_##name##_##off[m] = fcamd_rot::mandel_dot<off>(q, h.name);
        FCAMD_USER_ROTATE(FCAMD_X)
#undef FCAMD_X
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        s[m] = ys[m];
#define FCAMD_X(name, off) h.name[(off) + m] = y_##name##_##off[m];
        FCAMD_USER_ROTATE(FCAMD_X)
#undef FCAMD_X
    }
    return true;
}
#endif
