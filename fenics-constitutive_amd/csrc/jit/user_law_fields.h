// Per-point parameter fields of user-defined laws (userlaw.py: UserLaw(..., fields=...)).  The generated definitions of a law with
// fields include this header -- a law without fields never reaches it -- behind
//   FCAMD_USER_NFIELDS            number of fields
//   FCAMD_USER_FIELDS(X)          X(index, name) for every field, in the order of UserArgs.fields
// and define, after it, the per-lane overload
//   UserParams fcamd_user_params(const double* v, const fcamd_user::UserFieldValues& f)
// which fills the law's struct from the parameter values of the launch (the scalars, first in UserParams) and the lane's field
// values (the fields, behind them).  user_law_tile.h builds the UserParams of every tile from it (user_lane_params), so the point
// functions see the const UserParams& they always saw.
//
// A field is one double per point: per 64-point tile one contiguous run of 64 doubles, of which lane l loads field[p0 + l] as one
// 8-byte load -- 512 bytes per wave, coalesced, no transposition.  The loads are issued before the tile's other loads and their
// values are first used in the point function, behind every transposition.  In the ragged last tile the lanes past its end
// take the values of the tile's first point: they run on a valid parameter set (their results are not stored and not counted)
// and no load goes past the end of the field.
//
// Parity rule (param_source.h): the values enter the point function as the scalars do -- plain doubles, constants of every
// Dual pass -- and the program is compiled without FP contraction, so a field whose values all equal v gives the bits of the
// law with the scalar v.
#pragma once
#include "tile_io.h"

namespace fcamd_user {
using namespace fcamd;

constexpr int kNF = FCAMD_USER_NFIELDS;
static_assert(kNF >= 1, "user_law_fields.h is for laws with at least one field");

// the field values of one lane's point, in the order of FCAMD_USER_FIELDS
struct UserFieldValues {
    double v[kNF];
};

template <bool NT>
__device__ __forceinline__ double load8(const double* p) {
    if constexpr (NT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}

// the field values of the lane's point in the tile starting at p0 (npts points; FULL: 64)
template <bool FULL, bool NT>
__device__ __forceinline__ void user_fields_load(const double* const (&fields)[kNF], long long p0, int npts, int lane,
                                                 UserFieldValues& f) {
    const long long i = p0 + ((FULL || lane < npts) ? lane : 0);
#pragma unroll
    for (int k = 0; k < kNF; ++k) f.v[k] = load8<NT>(fields[k] + i);
}

}  // namespace fcamd_user
