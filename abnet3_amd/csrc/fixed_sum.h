// fixed_sum.h -- the two sum reductions of the forward-backward kernels (hmm_fb_kernel of hmm.hip, hmm_dense_kernel of
// hmm_dense.hip), each in ONE fixed order: the bits of c_t, of the log-likelihood and of the stays do not depend on who
// calls them or on the grid.  Both take and return values only -- no LDS array of the kernel's is handed in beyond the
// block sum's own scratch --, and moving them here left the device code of both files byte for byte what it was.
#pragma once
#include "common.h"

namespace abn {

// One DPP exchange inside the rows of 16 lanes (every lane has a source under these controls) and the sum of the two:
// both partners add the same two numbers, so they hold the same bits.
template <int CTRL>
__device__ __forceinline__ float fixed_dpp_add(float v)
{
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// The sum over the wave, in every lane, in one fixed order: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror,
// row_mirror leave the row's sum in its 16 lanes; the four rows' sums are read with v_readlane and added row 0 first.
// All 64 lanes must be active.
__device__ __forceinline__ float fixed_wave_sum(float v)
{
    v = fixed_dpp_add<0xB1>(v);
    v = fixed_dpp_add<0x4E>(v);
    v = fixed_dpp_add<0x141>(v);
    v = fixed_dpp_add<0x140>(v);
    float r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
#pragma unroll
    for (int i = 1; i < 4; ++i) r += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16 * i));
    return r;
}

// 256 doubles summed in a fixed tree; the result is returned to every thread.
__device__ __forceinline__ double fixed_block_sum(double v, double* sh)
{
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

}  // namespace abn
