// dtw_tiles.h -- what the wavefront-per-pair DTW kernels share (abx.hip: dtw_cost_kernel; search.hip:
// dtw_search_kernel): the DPP wave shift of the sweep, the LDS hand-off inside one wavefront, and the 2 x 2 tiles of
// frame distances (the fmaf chain of the cosine cell, the float32 sums of the symmetrised-KL cell).  Every translation
// unit that includes this file is compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace abn {

// lane l receives lane l-1's value (lane 0: overridden by the caller)
__device__ __forceinline__ double shr1_f64(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);      // wave_shr:1
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ int shr1_i32(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

// LDS hand-off inside ONE wavefront: its LDS operations complete in order, so keeping the compiler from moving
// accesses across is all that is needed
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// the four dot products of rows x0, x1 against rows y0, y1, each ONE fmaf chain in k order (what the oracle's loop and
// the MFMA path of abn_dtw_batched compute): a 2 x 2 tile shares its loads, one load per fma instead of two
template <bool VEC>
__device__ __forceinline__ void dot_tile(const float* __restrict__ x0, const float* __restrict__ x1,
                                         const float* __restrict__ y0, const float* __restrict__ y1, int D, float (&acc)[4])
{
    float a00 = 0.0f, a01 = 0.0f, a10 = 0.0f, a11 = 0.0f;
    if (VEC) {
        for (int k = 0; k < D; k += 4) {
            const float4 p = *reinterpret_cast<const float4*>(x0 + k), q = *reinterpret_cast<const float4*>(x1 + k);
            const float4 u = *reinterpret_cast<const float4*>(y0 + k), v = *reinterpret_cast<const float4*>(y1 + k);
            a00 = fmaf(p.x, u.x, a00); a01 = fmaf(p.x, v.x, a01); a10 = fmaf(q.x, u.x, a10); a11 = fmaf(q.x, v.x, a11);
            a00 = fmaf(p.y, u.y, a00); a01 = fmaf(p.y, v.y, a01); a10 = fmaf(q.y, u.y, a10); a11 = fmaf(q.y, v.y, a11);
            a00 = fmaf(p.z, u.z, a00); a01 = fmaf(p.z, v.z, a01); a10 = fmaf(q.z, u.z, a10); a11 = fmaf(q.z, v.z, a11);
            a00 = fmaf(p.w, u.w, a00); a01 = fmaf(p.w, v.w, a01); a10 = fmaf(q.w, u.w, a10); a11 = fmaf(q.w, v.w, a11);
        }
    } else {
        for (int k = 0; k < D; ++k) {
            const float p = x0[k], q = x1[k], u = y0[k], v = y1[k];
            a00 = fmaf(p, u, a00); a01 = fmaf(p, v, a01); a10 = fmaf(q, u, a10); a11 = fmaf(q, v, a11);
        }
    }
    acc[0] = a00; acc[1] = a01; acc[2] = a10; acc[3] = a11;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// the four symmetrised-KL sums of rows x0, x1 against rows y0, y1 (P and L tables): per k and cell a subtraction of
// the P's, one of the L's, their product and the addition to the cell's sum, each rounded to float32 (the file is
// compiled without fma contraction).  Two cells to a float2, so the compiler may issue v_pk_add_f32 / v_pk_mul_f32;
// packed or not, every lane of every operation is the IEEE result.  The eight loads of a k step serve four cells.
template <bool VEC>
__device__ __forceinline__ void kl_tile(const float* __restrict__ px0, const float* __restrict__ px1,
                                        const float* __restrict__ lx0, const float* __restrict__ lx1,
                                        const float* __restrict__ py0, const float* __restrict__ py1,
                                        const float* __restrict__ ly0, const float* __restrict__ ly1, int D, float (&acc)[4])
{
    f32x2 a0 = {0.0f, 0.0f}, a1 = {0.0f, 0.0f};        // (a00, a01), (a10, a11)
#define ABN_KL_STEP(P0, P1, L0, L1, PU, PV, LU, LV)                                     \
    do {                                                                                \
        const f32x2 pu_ = {PU, PV}, lu_ = {LU, LV};                                     \
        const f32x2 p0_ = {P0, P0}, l0_ = {L0, L0}, p1_ = {P1, P1}, l1_ = {L1, L1};     \
        a0 = a0 + ((p0_ - pu_) * (l0_ - lu_));                                          \
        a1 = a1 + ((p1_ - pu_) * (l1_ - lu_));                                          \
    } while (0)
    if (VEC) {
        for (int k = 0; k < D; k += 4) {
            const float4 p = *reinterpret_cast<const float4*>(px0 + k), q = *reinterpret_cast<const float4*>(px1 + k);
            const float4 lp = *reinterpret_cast<const float4*>(lx0 + k), lq = *reinterpret_cast<const float4*>(lx1 + k);
            const float4 u = *reinterpret_cast<const float4*>(py0 + k), v = *reinterpret_cast<const float4*>(py1 + k);
            const float4 lu = *reinterpret_cast<const float4*>(ly0 + k), lv = *reinterpret_cast<const float4*>(ly1 + k);
            ABN_KL_STEP(p.x, q.x, lp.x, lq.x, u.x, v.x, lu.x, lv.x);
            ABN_KL_STEP(p.y, q.y, lp.y, lq.y, u.y, v.y, lu.y, lv.y);
            ABN_KL_STEP(p.z, q.z, lp.z, lq.z, u.z, v.z, lu.z, lv.z);
            ABN_KL_STEP(p.w, q.w, lp.w, lq.w, u.w, v.w, lu.w, lv.w);
        }
    } else {
        for (int k = 0; k < D; ++k) ABN_KL_STEP(px0[k], px1[k], lx0[k], lx1[k], py0[k], py1[k], ly0[k], ly1[k]);
    }
#undef ABN_KL_STEP
    acc[0] = a0.x; acc[1] = a0.y; acc[2] = a1.x; acc[3] = a1.y;
}

}  // namespace abn
