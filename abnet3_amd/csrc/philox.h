// philox.h -- the counter-based generator and the range maps of the sampling kernels (sampler.hip, tcl.hip).
// Integer arithmetic only: a draw is a pure function of (counter, key), so a launch can be restated bit for bit on
// the host (tests/sampler_np.py, tests/tcl_np.py) and cut into shares that reproduce their slice of the whole.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace abn {

struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}

// floor(r M / 2^128) for the 128-bit r = (x + 2^32 y) 2^64 + (z + 2^32 w): a value in [0, M), each with
// floor(2^128 / M) or one more of the 2^128 values of r
__device__ __forceinline__ uint64_t map128(U4 r, uint64_t M)
{
    const uint64_t rh = ((uint64_t)r.y << 32) | r.x, rl = ((uint64_t)r.w << 32) | r.z;
    const uint64_t lo = rh * M, s = lo + __umul64hi(rl, M);
    return __umul64hi(rh, M) + (s < lo ? 1 : 0);
}

// floor(r M / 2^64) for a 64-bit r: a value in [0, M), each with floor(2^64 / M) or one more of the 2^64 values of r
__device__ __forceinline__ uint64_t map64(uint64_t r, uint64_t M) { return __umul64hi(r, M); }

}  // namespace abn
