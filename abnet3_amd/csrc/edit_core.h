// edit_core.h -- the Levenshtein distance of one pair as a bit-vector recurrence (Myers 1999 in Hyyro's 2003 form for the
// GLOBAL distance, the block carry as in Myers' multi-word version).  Plain C++ with no dependency: edit.hip runs it one
// lane per pair, a host program can include it as it stands.
//
// The SHORT side (the pattern, m symbols, 1 <= m <= BITS x W) lies along the bits: bit i of word w stands for row
// 64 w + i + 1 of the DP matrix.  Pv / Mv hold the vertical differences D[r][c] - D[r-1][c] = +1 / -1 of the current
// column, and one step per symbol of the LONG side (the text, n symbols, unbounded) moves them one column on:
//     Xv = Eq | Mv;  Eq |= (hin < 0);  Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;  Ph = Mv | ~(Xh | Pv);  Mh = Pv & Xh;
//     hout = Ph[top] - Mh[top];  Ph = Ph << 1 | (hin > 0);  Mh = Mh << 1 | (hin < 0);  Pv = Mh | ~(Xv | Ph);  Mv = Ph & Xv
// Eq has bit i set where pattern symbol i equals the text symbol.  hin is the horizontal difference that enters the word
// from below: +1 for word 0 (row 0 of the matrix is 0, 1, 2, ...: the global distance), the word below's hout otherwise.
// Ph / Mh bit m - 1 (before the shift) is D[m][c] - D[m][c-1]: the score starts at m and follows it.
//
// Word edges.  Information only travels from low bits to high bits (the addition's carry, the shift, the block carry), so
// the bits above m - 1 in the last word may hold anything and words beyond ceil(m / BITS) are never computed.  The score
// bit is read at (m - 1) % BITS of word (m - 1) / BITS -- bit 63 when m is a multiple of 64 -- and the block carry at
// BITS - 1: no shift count ever reaches BITS.
//
// Eq is built by comparing the text symbol with every pattern symbol (symbols are arbitrary int32: no alphabet table),
// TEXT_BLOCK text symbols at a time so that one read of a pattern symbol serves TEXT_BLOCK compares, and always in
// 32-bit pieces (a compare, a select, an or per cell) whatever the recurrence's word is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ABN_EDIT_HD __host__ __device__ __forceinline__
#else
#define ABN_EDIT_HD inline
#endif

namespace abn {

constexpr int EDIT_TEXT_BLOCK = 4;

// pat[j * STRIDE], j < m: the short side (edit.hip: lane-interleaved LDS, STRIDE = the block's lanes).
template <typename Word, int W, int STRIDE>
ABN_EDIT_HD int32_t edit_pair(const int32_t* pat, int m, const int32_t* text, int n)
{
    constexpr int BITS = (int)sizeof(Word) * 8;
    constexpr int H = BITS * W / 32;                        // 32-bit pieces of Eq
    constexpr int K = EDIT_TEXT_BLOCK;
    Word Pv[W], Mv[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        Pv[w] = ~(Word)0;
        Mv[w] = 0;
    }
    const int lastw = (m - 1) / BITS, lastbit = (m - 1) % BITS;
    int32_t score = m;
    for (int i = 0; i < n; i += K) {
        int32_t c[K];
#pragma unroll
        for (int k = 0; k < K; ++k) c[k] = text[i + k < n ? i + k : n - 1];
        uint32_t e[K][H];
#pragma unroll
        for (int h = 0; h < H; ++h) {
#pragma unroll
            for (int k = 0; k < K; ++k) e[k][h] = 0;
            const int cnt = m - 32 * h < 32 ? m - 32 * h : 32;
            uint32_t bit = 1;
            for (int j = 0; j < cnt; ++j) {
                const int32_t s = pat[(32 * h + j) * STRIDE];
#pragma unroll
                for (int k = 0; k < K; ++k) e[k][h] |= s == c[k] ? bit : 0u;
                bit <<= 1;
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (i + k < n) {
                int hin = 1;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    if (W == 1 || w <= lastw) {
                        Word Eq;
                        if constexpr (sizeof(Word) == 8) Eq = (Word)e[k][2 * w] | ((Word)e[k][2 * w + 1] << 32);
                        else Eq = e[k][w];
                        const Word pv = Pv[w], mv = Mv[w];
                        const Word Xv = Eq | mv;
                        if (W > 1) Eq |= (Word)(hin < 0);
                        const Word Xh = (((Eq & pv) + pv) ^ pv) | Eq;
                        Word Ph = mv | ~(Xh | pv);
                        Word Mh = pv & Xh;
                        if (W == 1 || w == lastw) score += (int32_t)((Ph >> lastbit) & 1) - (int32_t)((Mh >> lastbit) & 1);
                        const int hout = (int)(Ph >> (BITS - 1)) - (int)(Mh >> (BITS - 1));
                        Ph = (Ph << 1) | (Word)(hin > 0);
                        Mh = (Mh << 1) | (Word)(hin < 0);
                        Pv[w] = Mh | ~(Xv | Ph);
                        Mv[w] = Ph & Xv;
                        hin = hout;
                    }
                }
            }
        }
    }
    return score;
}

}  // namespace abn
