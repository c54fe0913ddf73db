// The point-function contract of user-defined laws (fenics_constitutive_amd.UserLaw, userlaw.py).  Compiled at run time with
// hiprtc for gfx950, together with the structs generated from the law's Python dicts, the user's source and the kernel template
// user_law.hip, whose tile code (user_law_tile.h) does all the memory work.  The user writes ONE function:
//
//   struct UserParams  { double E, nu; };                             // generated: one double per parameter, in the given order
//   struct UserHistory { double eps_p[6]; double alpha[1]; };          // generated: one array per history field (tuple: product)
//
//   __device__ int fcamd_user_point(const UserParams& p, double t, double del_t,
//                                   const double (&grad)[9],   // grad_del_u of the point, row-major
//                                   const double (&eps)[6],    // its Mandel strain increment (strain_from_grad_u, FULL)
//                                   double (&sigma)[6],        // in: committed stress, out: new stress
//                                   double (&D)[36],           // in: zeros, out: tangent, row-major (not stored when tangent is None)
//                                   UserHistory& h);           // in: committed history, out: trial history
//   // return 0 = converged; any other value counts the point as not converged
//
// Per-point parameter fields (UserLaw(..., fields=...), user_law_fields.h): a parameter given as a field is a double member of
// UserParams like a scalar -- the scalars first, in their order, then the fields, in theirs -- and holds the value of the lane's
// own point; the point function does not change.  UserParams is then built per lane and tile instead of once per kernel, and in
// the Dual passes of the other two modes a field value is a constant (zero partials), as a scalar is.
//
// `eps` comes from the mandel_strain call of the built-in kernels with the factor of the Python laws: it is bit-identical to
// theirs.  The program is compiled with -ffp-contract=off, like the library: a * b + c is two roundings; write
// __builtin_fma(a, b, c) where one rounding is meant.  Everything below lives in the global namespace of the program.
#pragma once
#include "tile_io.h"
#include "param_source.h"

// --- helpers the built-in laws use, for users who want to reproduce their expression order ---------------------------------

// The four distinct entries {[i][i] (i < 3), [i][j] (i != j < 3), [i][i] (i >= 3), the rest} of the isotropic elastic matrix of
// LinearElasticityModel from E and nu, with the library's expressions (lame, elastic_tangent_full).
using fcamd::ElasticEntries;
using fcamd::le_entries;
// entry [i][j] of the matrix whose four distinct entries are d (le_entries(...).d)
using fcamd::elastic_entry;
// y_i = sum_k x_k * M[6 k + i] as an ascending-k FMA chain: "strain @ D" of the NumPy laws, as the built-in kernels evaluate it
using fcamd::row_times_matrix_fma;
// Mandel strain increment from a row-major 3x3 gradient with the off-diagonal factor f
using fcamd::mandel_strain;

// the full 6x6 row-major matrix of four distinct entries
__device__ __forceinline__ void fcamd_elastic_matrix(const ElasticEntries& e, double (&D)[36]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) D[6 * i + j] = elastic_entry(e.d, i, j);
}
