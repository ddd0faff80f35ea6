// vit_wave.h -- the per-frame maximum and the traceback of the two max-product kernels, shared by kmeans.hip
// (km_viterbi_kernel: abn_kmeans_viterbi) and hmm.hip (hmm_viterbi_kernel: abn_hmm_viterbi): the (score, index) key
// whose unsigned order makes "the max and its lowest index" ONE max-reduction, its DPP reduction over a wave, and the
// wave that walks the stay bits backwards 64 frames at a time.  Below them the same for the kernels with a minimum unit
// duration (km_viterbi_dur_kernel, hmm_viterbi_dur_kernel): the step of one unit's chain of states, the float max over a
// wave, the parking of the chains around a score tile, the final state's key and vit_traceback_dur.
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

// ---- minimum duration (km_viterbi_dur_kernel, hmm_viterbi_dur_kernel: abnx_kmeans_viterbi_dur, abnx_hmm_viterbi_dur) --------
// Unit k is a left-to-right chain of S states with tied emissions, of which only the last may repeat.  A lane keeps the
// chain of its unit in SC >= S registers: state i lives in slot e0 + i, e0 = SC - S, so the exit state is always slot
// SC - 1, the entry is injected at slot e0 by a uniform compare, and the slots below e0 hold -inf for good.
constexpr int VIT_DUR_MAX = 8;

// One good frame of one unit: V (the normalised previous values) becomes U.  ent is what enters state 0 (E + lr[k]; lw[k]
// at the first good frame, where V is all -inf), *st the stay bit of the exit state (strict: a tie goes to the advance).
// Returns the max of the unit's U; the exit state's U is V[SC - 1].  Every operation is one rounded add or a compare.
template <int SC>
__device__ __forceinline__ float vit_dur_step(float (&V)[SC], float s, float ent, float ls, int e0, bool* st)
{
    const float a = V[SC - 1] + ls;
    float prev = ent;
    if constexpr (SC > 1) prev = e0 == SC - 1 ? ent : V[SC - 2];
    *st = a > prev;
    const float ue = s + (*st ? a : prev);
    float m = ue;
#pragma unroll
    for (int j = SC - 2; j >= 0; --j) {                               // (downwards: V[j - 1] is still the previous frame's)
        const float below = j > 0 ? V[j > 0 ? j - 1 : 0] : -INFINITY;
        V[j] = s + (j == e0 ? ent : below);
        m = fmaxf(m, V[j]);
    }
    V[SC - 1] = ue;
    return m;
}

// The max of a float over the wave, in every lane: vit_wave_max's exchanges.  All 64 lanes must be active.
template <int CTRL>
__device__ __forceinline__ float vit_dpp_fmax(float v)
{
    const float o = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
    return fmaxf(o, v);
}
__device__ __forceinline__ float vit_wave_fmax(float v)
{
    v = vit_dpp_fmax<0xB1>(v);
    v = vit_dpp_fmax<0x4E>(v);
    v = vit_dpp_fmax<0x141>(v);
    v = vit_dpp_fmax<0x140>(v);
    float r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
#pragma unroll
    for (int i = 1; i < 4; ++i) r = fmaxf(r, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16 * i)));
    return r;
}

// The chains across a block's score phase.  The score tile takes most of the register file, so the kernels whose slab is
// in the workspace (K > 128) put the first PARK = min(NQ SC, VIT_DUR_PARK) of a thread's NQ SC values into LDS behind the
// operand tiles before the tile and read them back after it; every thread reads what it wrote itself, so no barrier is
// needed for that.  80 KiB of LDS at most: with the 72 KiB of operand tiles it fits the CU's 160.
constexpr int VIT_DUR_PARK = 80;
constexpr size_t VIT_DUR_PARK_BYTES = sizeof(float) * 256 * VIT_DUR_PARK;
template <int NQ, int SC>
constexpr int vit_dur_parked(bool ldss) { return ldss ? 0 : (NQ * SC < VIT_DUR_PARK ? NQ * SC : VIT_DUR_PARK); }
template <int PARK, int NQ, int SC>
__device__ __forceinline__ void vit_dur_park(const float (&V)[NQ][SC], float* park, int t)
{
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int j = 0; j < SC; ++j)
            if (SC * q + j < PARK) park[256 * (SC * q + j) + t] = V[q][j];
}
template <int PARK, int NQ, int SC>
__device__ __forceinline__ void vit_dur_unpark(float (&V)[NQ][SC], const float* park, int t)
{
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int j = 0; j < SC; ++j)
            if (SC * q + j < PARK) V[q][j] = park[256 * (SC * q + j) + t];
}

// The final state of an utterance: the lowest k, then the largest slot, with V == 0 (the normalised maximum).  A lane
// first finds its own -- code = SC q + slot over its q descending, so the lowest q stands last, -1: none; small constants
// only, nothing per (q, slot) that would be kept in a register for the whole kernel -- and then forms one key whose max
// over the workgroup is the state (0: this lane holds none).
template <int SC>
__device__ __forceinline__ int vit_dur_final_code(const float (&V)[SC], int q, int code)
{
#pragma unroll
    for (int j = 0; j < SC; ++j) code = V[j] == 0.0f ? SC * q + j : code;
    return code;
}
template <int SC>
__device__ __forceinline__ unsigned long long vit_dur_final_key(int code, int t)
{
    if (code < 0) return 0;
    const int k = 256 * (code / SC) + t;
    return (1ull << 40) | ((unsigned long long)(0xFFFFFu - (unsigned)k) << 8) | (unsigned)(code % SC);
}
__device__ __forceinline__ int vit_dur_final_k(unsigned long long key) { return (int)(0xFFFFFu - (unsigned)((key >> 8) & 0xFFFFFu)); }
__device__ __forceinline__ int vit_dur_final_slot(unsigned long long key) { return (int)(key & 0xFFu); }

// vit_traceback with a minimum duration of S frames, by ONE wave (all 64 lanes), 64 frames per round.  The last good
// frame is in state (cur, i): forced = 0 if i == S - 1, otherwise i + 1 -- the number of good frames, counted backwards
// from the last, to the frame in state 0.  (No good frame: cur = -1, forced = 0.)  In the exit state a set bit keeps
// (cur, S - 1); a cleared bit means that this frame and the S - 1 good frames before it were the forced advance through
// cur -- BAD frames (prevj == -2) are not counted --, and the frame in state 0 holds the previous good frame's exit j* in
// prevj (-1: it is the first good frame).  Returns the changes of id.
__device__ __forceinline__ int vit_traceback_dur(const unsigned long long* stay, const int* prevj, int kw, int* ids, int64_t o,
                                                 int L, int S, int cur, int forced, int lane)
{
    int te = L - 1, nsw = 0;
    while (te >= 0) {
        const int g = te - lane;
        const int pj = g >= 0 ? prevj[g] : -2;
        const bool good = pj != -2;
        const unsigned long long gmask = __ballot(good);
        int l1 = -1, f = forced;
        if (forced == 0) {                                            // (uniform) in the exit state: look for a cleared bit
            bool cleared = false;
            if (good && cur >= 0) cleared = !((stay[(int64_t)g * kw + (cur >> 6)] >> (cur & 63)) & 1ull);
            const unsigned long long mask = __ballot(cleared);
            if (!mask) {                                              // frames te .. te - 63 keep cur
                if (g >= 0) ids[o + g] = (!good || cur < 0) ? -1 : cur;
                te -= 64;
                continue;
            }
            l1 = __builtin_ctzll(mask);
            f = S - 1;
        }
        // the frame in state 0 is the f-th good frame behind lane l1 (f == 0: lane l1 itself)
        unsigned long long behind = 0;
        int l2 = l1;
        bool found = f == 0;
        if (f > 0) {
            behind = l1 >= 0 ? gmask & ~((2ull << l1) - 1ull) : gmask;
            const int rank = __popcll(behind & ((2ull << lane) - 1ull));
            const unsigned long long hit = __ballot(good && lane > l1 && rank == f);
            found = hit != 0;
            l2 = found ? __builtin_ctzll(hit) : 63;
        }
        if (g >= 0 && lane <= l2) ids[o + g] = (!good || cur < 0) ? -1 : cur;
        if (found) {
            const int nj = __shfl(pj, l2);                            // -1: that was the first good frame
            nsw += nj >= 0 && nj != cur;
            cur = nj;
            forced = 0;
            te -= l2 + 1;
        } else {
            forced = f - __popcll(behind);
            te -= 64;
        }
    }
    return nsw;
}

}  // namespace abn
