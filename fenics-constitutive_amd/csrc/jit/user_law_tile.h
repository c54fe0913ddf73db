// The tile code of the kernel templates of user-defined laws (userlaw.py): user_law.hip (explicit tangent) and user_law_ad.hip
// (autodiff) include this header and define user_tile, the point step of one tile between the prologue below and its stores.
// Read at run time and compiled with hiprtc behind the generated definitions:
//   FCAMD_USER_WAVES                     waves per SIMD the register budget is cut for (the kernel entry below)
//   FCAMD_USER_NHIST                     number of history fields
//   FCAMD_USER_HISTORY_FIELDS(X)         X(index, name, doubles per point) for every history field
//   UserParams fcamd_user_params(const double* v)   the law's struct from the parameter values of the launch
//   FCAMD_USER_ROTATE(X)                 only with an objective rate (objective.py: JaumannRate), rotation.h included
//   FCAMD_USER_FIELDS(X)                 only with per-point parameter fields, user_law_fields.h included (which lists the rest)
// and the user's source.
//
// Shape of the built-in evaluate kernels (fcamd_kernels.hip): 256-thread blocks, one wave per 64-point tile, a grid-stride loop
// over the tiles.  Full tiles move 16-byte non-temporal chunks (tile_load / transpose_in / transpose_out of tile_io.h), the
// ragged last tile guarded 8-byte accesses.  Arrays of more than 18 doubles per point (the tangent: 36) pass the wave's LDS
// region in two halves of 32 points; each half is a contiguous run of the AoS array, so the chunks stay coalesced.
#pragma once

namespace fcamd_user {
using namespace fcamd;

constexpr int kMaxParams = 32;
constexpr int kNH = FCAMD_USER_NHIST > 0 ? FCAMD_USER_NHIST : 1;
// doubles per point that one pass through the wave's region holds: 64 x 18 doubles = 9 KiB per wave, 36 KiB per block -- four
// blocks (16 waves) still fit a CU's 160 KiB
constexpr int kUserWide = 18;
constexpr int kUserRegion = kWave * kUserWide;
// arrays of up to this many doubles per point (two halves of 32 points)
constexpr int kUserMaxDim = 2 * kUserWide;

// the only kernel parameter; userlaw.py mirrors the layout (_args_type)
struct UserArgs {
    const double* grad;          // [9 n]
    const double* stress_in;     // [6 n] committed stress (may alias stress_out)
    double* stress_out;          // [6 n]
    double* tangent;             // [36 n] or nullptr
    const double* h_in[kNH];     // committed history fields (may alias h_out)
    double* h_out[kNH];          // trial history fields
    unsigned long long* nonconv; // one word: points whose point function returned non-zero (zeroed by the caller)
    long long n;                 // points
    double t, del_t;
    double factor;               // Mandel factor of the off-diagonal strains (the Python laws')
    double params[kMaxParams];   // UserParams, in order
#ifdef FCAMD_USER_FIELDS
    const double* fields[kNF];   // [n] each: the per-point parameter fields, in the order of FCAMD_USER_FIELDS
#endif
};

#ifdef FCAMD_USER_FIELDS
// the UserParams of the lane's point in the tile starting at p0: the launch's scalars and the lane's field values
// (user_law_fields.h).  The loads are the first of the tile; nothing waits for them before the point function.
template <bool FULL, bool NT>
__device__ __forceinline__ UserParams user_lane_params(const UserArgs& a, long long p0, int npts, int lane) {
    UserFieldValues f;
    user_fields_load<FULL, NT>(a.fields, p0, npts, lane, f);
    return fcamd_user_params(a.params, f);
}
#endif

// AoS tile (registers) -> per-lane values; NC <= kUserWide through one pass, else two halves of 32 points
template <int NC>
__device__ __forceinline__ void user_in(const Chunks<NC>& c, double* region, int lane, double (&x)[NC]) {
    static_assert(NC <= kUserMaxDim, "history field wider than the LDS region");
    if constexpr (NC <= kUserWide) {
        transpose_in<NC>(c, region, lane, x);
    } else {
        constexpr int kHalf = 16 * NC;  // chunks of 32 points
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int k = 0; k < Chunks<NC>::K; ++k) {
                const int q = k * kWave + lane - h * kHalf;
                if (q >= 0 && q < kHalf && chunk_live<NC>(k, lane)) reinterpret_cast<d2*>(region)[q] = c.v[k];
            }
            wave_sync();
            if ((lane >> 5) == h) {
#pragma unroll
                for (int i = 0; i < NC; ++i) x[i] = region[(lane & 31) * NC + i];
            }
            wave_sync();
        }
    }
}

// per-lane values -> AoS tile in global memory (dst: the tile's first point, nelem: valid doubles of the tile)
template <int NC, bool FULL, bool NT>
__device__ __forceinline__ void user_out(const double (&x)[NC], double* region, int lane, double* dst, int nelem) {
    static_assert(NC <= kUserMaxDim, "history field wider than the LDS region");
    if constexpr (NC <= kUserWide) {
        transpose_out<NC, FULL, NT>(x, region, lane, dst, nelem);
    } else {
        constexpr int kHalf = 16 * NC;                      // chunks of 32 points
        constexpr int kPer = (kHalf + kWave - 1) / kWave;   // per lane
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if ((lane >> 5) == h) {
#pragma unroll
                for (int i = 0; i < NC; ++i) region[(lane & 31) * NC + i] = x[i];
            }
            wave_sync();
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const int q = k * kWave + lane;
                if (q < kHalf) {
                    const d2 v = reinterpret_cast<const d2*>(region)[q];
                    const int e = 2 * (q + h * kHalf);
                    if constexpr (FULL) {
                        store16<NT>(dst + e, v);
                    } else {
                        if (e < nelem) dst[e] = v.x;
                        if (e + 1 < nelem) dst[e + 1] = v.y;
                    }
                }
            }
            wave_sync();
        }
    }
}

// the committed state of the lane's point in the tile starting at p0 (gradient g, stress s, history h: double arrays), rotated
// when the law has an objective rate, and its Mandel strain increment e
template <bool FULL, bool NT, class H>
__device__ __forceinline__ void user_tile_in(const UserArgs& a, double* region, long long p0, int npts, int lane, double (&g)[9],
                                             double (&s)[6], double (&e)[6], H& h) {
    // every load of the tile is issued before the first transposition
    Chunks<9> cg;
    Chunks<6> cs;
    tile_load<9, FULL, NT>(cg, a.grad + p0 * 9, npts * 9, lane);
    tile_load<6, FULL, NT>(cs, a.stress_in + p0 * 6, npts * 6, lane);
#define FCAMD_X(k, name, dim) \
    Chunks<dim> c_##name;     \
    tile_load<dim, FULL, NT>(c_##name, a.h_in[k] + p0 * (dim), npts * (dim), lane);
    FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
    transpose_in<9>(cg, region, lane, g);
    transpose_in<6>(cs, region, lane, s);
#define FCAMD_X(k, name, dim) user_in<dim>(c_##name, region, lane, h.name);
    FCAMD_USER_HISTORY_FIELDS(FCAMD_X)
#undef FCAMD_X
#ifdef FCAMD_USER_ROTATE
    fcamd_user_rotate(g, s, h);  // objective rate (rotation.h): the committed state, before the point step sees it
#endif
    mandel_strain(g, a.factor, e);
}

// one 64-point tile (FULL) or the ragged last one (npts < 64); returns the tile's non-converged points (wave-uniform).  Defined
// by the template that includes this header.
template <bool FULL, bool NT>
__device__ __forceinline__ unsigned long long user_tile(const UserArgs& a, const UserParams& p, double* region, long long p0,
                                                        int npts, int lane);

}  // namespace fcamd_user

#if !defined(FCAMD_USER_PATH) && !defined(FCAMD_USER_WRAP)  // user_law_path.hip and user_law_wrapped.hip have kernels of their own around the helpers above
// FCAMD_USER_WAVES (generated): waves per SIMD the register budget is cut for -- 4 (128 VGPRs, what the LDS allows), or fewer
// for a law that spills at 4 (userlaw.py recompiles it)
extern "C" __global__ void __launch_bounds__(fcamd::kBlock, FCAMD_USER_WAVES) fcamd_user_law_kernel(const fcamd_user::UserArgs a) {
    using namespace fcamd_user;
    __shared__ __attribute__((aligned(16))) double scratch[kWavesPerBlock][kUserRegion];
    const int lane = (int)threadIdx.x & (kWave - 1);
    // wave index as a scalar: tile index and the tile base pointers live in SGPRs
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    double* region = scratch[wave];
#ifndef FCAMD_USER_FIELDS
    const UserParams p = fcamd_user_params(a.params);
#endif
    const long long nfull = a.n / kWave;
    const long long wstride = (long long)gridDim.x * kWavesPerBlock;
    unsigned long long bad = 0;
    long long tile = (long long)blockIdx.x * kWavesPerBlock + wave;
#ifdef FCAMD_USER_FIELDS  // UserParams per lane and tile
    for (; tile < nfull; tile += wstride)
        bad += user_tile<true, true>(a, user_lane_params<true, true>(a, tile * kWave, kWave, lane), region, tile * kWave, kWave, lane);
    if (tile == nfull && a.n > nfull * kWave) {
        const int npts = (int)(a.n - tile * kWave);
        bad += user_tile<false, false>(a, user_lane_params<false, false>(a, tile * kWave, npts, lane), region, tile * kWave, npts, lane);
    }
#else
    for (; tile < nfull; tile += wstride) bad += user_tile<true, true>(a, p, region, tile * kWave, kWave, lane);
    if (tile == nfull && a.n > nfull * kWave) bad += user_tile<false, false>(a, p, region, tile * kWave, (int)(a.n - tile * kWave), lane);
#endif
    if (bad != 0 && lane == 0) atomicAdd(a.nonconv, bad);
}
#endif  // FCAMD_USER_PATH, FCAMD_USER_WRAP
