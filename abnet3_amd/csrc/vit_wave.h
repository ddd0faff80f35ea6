// vit_wave.h -- the per-frame maximum and the traceback of the two max-product kernels, shared by kmeans.hip
// (km_viterbi_kernel: abn_kmeans_viterbi) and hmm.hip (hmm_viterbi_kernel: abn_hmm_viterbi): the (score, index) key
// whose unsigned order makes "the max and its lowest index" ONE max-reduction, its DPP reduction over a wave, and the
// wave that walks the stay bits backwards 64 frames at a time.
#pragma once
#include "common.h"

namespace abn {

// (score, index) as one integer whose unsigned order is: the greater score first, then the LOWER index -- so that the
// max and its lowest index are one max-reduction.  -0 is read as +0, as the float comparison reads it.
__device__ __forceinline__ unsigned long long vit_key(float v, int k)
{
    unsigned u = __float_as_uint(v == 0.0f ? 0.0f : v);
    u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
    return ((unsigned long long)u << 32) | (unsigned)~k;
}
__device__ __forceinline__ float vit_key_score(unsigned long long key)
{
    unsigned u = (unsigned)(key >> 32);
    u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
    return __uint_as_float(u);
}
// One DPP exchange inside the rows of 16 lanes (every lane has a source under these controls) and the max of the two.
template <int CTRL>
__device__ __forceinline__ unsigned long long vit_dpp_max(unsigned long long v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xf, 0xf, false);
    const unsigned long long o = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
    return o > v ? o : v;
}
// The max over the wave, in every lane: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror leave the
// row's max in its 16 lanes; the four rows' values are read with v_readlane.  All 64 lanes must be active.
__device__ __forceinline__ unsigned long long vit_wave_max(unsigned long long v)
{
    v = vit_dpp_max<0xB1>(v);
    v = vit_dpp_max<0x4E>(v);
    v = vit_dpp_max<0x141>(v);
    v = vit_dpp_max<0x140>(v);
    unsigned long long r = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 16 * i);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 16 * i);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        r = o > r ? o : r;
    }
    return r;
}

// The traceback of one utterance of L frames at rows o .., by ONE wave (all 64 lanes): jprev is the last good frame's
// j*; stay[g kw + (k >> 6)] bit k & 63 says that frame g keeps id k, prevj[g] is the previous good frame's j* (-1: g is
// the first good frame, -2: g is a BAD frame, which gets id -1 and is passed over).  Returns the changes of id.
__device__ __forceinline__ int vit_traceback(const unsigned long long* stay, const int* prevj, int kw, int* ids, int64_t o,
                                             int L, int jprev, int lane)
{
    int cur = jprev, te = L - 1, nsw = 0;
    while (te >= 0) {
        const int g = te - lane;
        int pj = -2;
        bool cleared = false;
        if (g >= 0) {
            pj = prevj[g];
            if (cur >= 0 && pj != -2) cleared = !((stay[(int64_t)g * kw + (cur >> 6)] >> (cur & 63)) & 1ull);
        }
        const unsigned long long mask = __ballot(cleared);
        const int l1 = mask ? __builtin_ctzll(mask) : 63;     // frames te .. te - l1 keep cur
        if (g >= 0 && lane <= l1) ids[o + g] = (pj == -2 || cur < 0) ? -1 : cur;
        if (mask) {
            const int nj = __shfl(pj, l1);                    // -1: that was the first good frame
            nsw += nj >= 0 && nj != cur;                      // (equal where the switch lands on the same id again)
            cur = nj;
        }
        te -= l1 + 1;
    }
    return nsw;
}

}  // namespace abn
