// Kernel template of user-defined laws (userlaw.py): the point step of a FULL law around the user's fcamd_user_point
// (user_law_api.h), inside the tile code of user_law_tile.h, whose header lists the generated definitions it is compiled behind.
#pragma once
#include "user_law_tile.h"

namespace fcamd_user {

template <bool FULL, bool NT>
__device__ __forceinline__ unsigned long long user_tile(const UserArgs& a, const UserParams& p, double* region, long long p0,
                                                        int npts, int lane) {
    double g[9], s[6], e[6], D[36];
    UserHistory h;
    user_tile_in<FULL, NT>(a, region, p0, npts, lane, g, s, e, h);
#pragma unroll
    for (int i = 0; i < 36; ++i) D[i] = 0.0;
    const int rc = fcamd_user_point(p, a.t, a.del_t, g, e, s, D, h);
    const unsigned long long bad = __builtin_amdgcn_ballot_w64((FULL || lane < npts) && rc != 0);
    transpose_out<6, FULL, NT>(s, region, lane, a.stress_out + p0 * 6, npts * 6);
#define FCAMD_X(k, name, dim) user_out<dim, FULL, NT>(h.name, region, lane, a.h_out[k] + p0 * (dim), npts * (dim));
    FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
    if (a.tangent != nullptr) user_out<36, FULL, NT>(D, region, lane, a.tangent + p0 * 36, npts * 36);
    return (unsigned long long)__popcll(bad);
}

}  // namespace fcamd_user
