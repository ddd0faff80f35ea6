// kmeans_tile.h -- the fp32 score tile of the k-means kernels, shared by kmeans.hip (abn_kmeans_assign,
// abn_kmeans_viterbi) and eskmeans.hip (abn_esk_score): the 128 x 128 tile of s = [xc | 1] . [m | b] on the matrix cores,
// ka ascending, and the operand loaders that form the augmented rows on the way into LDS.  km_score_tile_with takes the
// A-operand loader as a parameter (issue / commit, as below), so that a caller whose rows do not lie in a table --
// the candidate segments of eskmeans.hip -- runs the SAME MFMA sequence and depth order over them.
#pragma once
#include "common.h"
#include "gemm_f32.h"

#include <limits.h>
#include <math.h>

namespace abn {

constexpr int KM_B = 128;                  // frame block = centroid tile of the assign pass (2 x 2 waves of 2 x 2 MFMA blocks)
constexpr int KM_MAX_D = 512;
constexpr int KM_MAX_K = 4096;
constexpr int KM_PT = KM_B * BK / 256;     // elements per thread of a 128 x 32 operand tile (scalar loads: D = 39 rows are not 16-byte aligned)
constexpr int KM_LST = KM_B + 1;           // a thread walks its frame's row of the staged scores, 129 dwords apart = conflict-free
using KmTile = TileShape<KM_B, true>;
constexpr size_t KM_TILE_BYTES = sizeof(float) * 4 * KmTile::floats;      // two stages of each operand
static_assert(KM_TILE_BYTES >= sizeof(float) * KM_B * KM_LST, "the score tile is staged in the operand buffers");

struct KmP {
    const float* x; const float* shift;
    const float* m; const float* b;
    int T, K, D;
    int* ids; const int* prev; float* best; int* changed;
    int tiles_k;
};

// 128 x 32 tiles, K-contiguous in LDS ([row][36]).  Thread t owns column k0 + (t & 31) of rows (t >> 5) + 8 i; column
// ka < D is xc / m, column D the ones column / b, the rest the zero fill up to the k-tile.  Branch-free issue from
// clamped addresses, validity applied at commit (gemm_f32.h's tile_issue / tile_commit).
__device__ __forceinline__ void km_x_issue(float* r, const KmP& p, int m0, int k0)
{
    const int t = threadIdx.x, ka = k0 + (t & 31);
#pragma unroll
    for (int i = 0; i < KM_PT; ++i) {
        const int row = m0 + (t >> 5) + 8 * i;
        r[i] = p.x[(ka < p.D && row < p.T) ? (int64_t)row * p.D + ka : 0];
    }
}
// A non-finite value contributes 0 (its frame is BAD: the kernel marks it and nobody uses its scores).
__device__ __forceinline__ void km_x_commit(const float* r, float* __restrict__ lds, const KmP& p, int m0, int k0)
{
    const int t = threadIdx.x, ka = k0 + (t & 31);
    const float sh = p.shift[ka < p.D ? ka : 0];
#pragma unroll
    for (int i = 0; i < KM_PT; ++i) {
        const int rl = (t >> 5) + 8 * i;
        const float xc = r[i] - sh;
        float v = ka < p.D ? (__builtin_isfinite(xc * xc) ? xc : 0.0f) : ka == p.D ? 1.0f : 0.0f;
        lds[rl * KmTile::stride + (t & 31)] = m0 + rl < p.T ? v : 0.0f;
    }
}
__device__ __forceinline__ void km_w_issue(float* r, const KmP& p, int n0, int k0)
{
    const int t = threadIdx.x, ka = k0 + (t & 31);
    const float* const base = ka < p.D ? p.m : p.b;
#pragma unroll
    for (int i = 0; i < KM_PT; ++i) {
        const int comp = n0 + (t >> 5) + 8 * i;
        const int64_t off = ka < p.D ? (int64_t)comp * p.D + ka : (int64_t)comp;
        r[i] = base[(ka <= p.D && comp < p.K) ? off : 0];
    }
}
__device__ __forceinline__ void km_w_commit(const float* r, float* __restrict__ lds, const KmP& p, int n0, int k0)
{
    const int t = threadIdx.x, ka = k0 + (t & 31);
#pragma unroll
    for (int i = 0; i < KM_PT; ++i) {
        const int rl = (t >> 5) + 8 * i;
        lds[rl * KmTile::stride + (t & 31)] = (ka <= p.D && n0 + rl < p.K) ? r[i] : 0.0f;
    }
}

// The 128 x 128 score tile of frames m0 .. and centroids n0 ..: rows = frames, columns = centroids, wave w owns the
// 64 x 64 block ((w >> 1) 64, (w & 1) 64).  The caller guarantees that nobody still reads the operand buffers; on
// return every wave has passed the last barrier, so the buffers are free again.  Depth runs in BK chunks, so D up to
// 512 needs no larger accumulator.
// The A operand comes from `al`: al.issue(r, k0) loads this thread's KM_PT elements of the k-tile at k0 into registers,
// al.commit(r, lds, k0) writes them (augmented, validity applied) to the stage.
template <class AL>
__device__ __forceinline__ void km_score_tile_with(const AL& al, const KmP& p, int n0, float* As, float* Bs, f32x16 (&acc)[2][2])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    const int nkt = (p.D + 1 + BK - 1) / BK;
    float ra[KM_PT], rb[KM_PT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    al.issue(ra, 0);
    km_w_issue(rb, p, n0, 0);
    al.commit(ra, As, 0);
    km_w_commit(rb, Bs, p, n0, 0);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nkt;
        const float* as = As + cur * KmTile::floats;
        const float* bs = Bs + cur * KmTile::floats;
        if (more) {
            al.issue(ra, (kt + 1) * BK);
            km_w_issue(rb, p, n0, (kt + 1) * BK);
        }
#pragma unroll
        for (int g = 0; g < BK / 8; ++g) {
            f32x4 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = frag_read<KM_B, true>(as, wm0 + 32 * i, g, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = frag_read<KM_B, true>(bs, wn0 + 32 * j, g, lane);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
        }
        if (more) {
            al.commit(ra, As + (cur ^ 1) * KmTile::floats, (kt + 1) * BK);
            km_w_commit(rb, Bs + (cur ^ 1) * KmTile::floats, p, n0, (kt + 1) * BK);
        }
        __syncthreads();
    }
}

// The frames of a table as the A operand: rows m0 .. of p.x, centred on load.
struct KmFrameRows {
    const KmP& p; int m0;
    __device__ __forceinline__ void issue(float* r, int k0) const { km_x_issue(r, p, m0, k0); }
    __device__ __forceinline__ void commit(const float* r, float* __restrict__ lds, int k0) const { km_x_commit(r, lds, p, m0, k0); }
};
__device__ __forceinline__ void km_score_tile(const KmP& p, int m0, int n0, float* As, float* Bs, f32x16 (&acc)[2][2])
{
    km_score_tile_with(KmFrameRows{p, m0}, p, n0, As, Bs, acc);
}

// The sweep of the centroid tiles with a running (best score, lowest index) per row: two threads per row (row = t & 127,
// half = t >> 7: 64 centroids of every tile each, ascending k, strict >: equal scores go to the lowest k), the score
// tile staged in the operand buffers, the two halves merged through red_s / red_i [128].  On return the threads of
// half 0 hold their row's result.  (Half 0 always owns centroid 0: its index starts there, so that a row whose scores
// never compare greater than -inf still gets an id inside 0 .. K - 1.)  smem: KM_TILE_BYTES of dynamic LDS.
template <class AL>
__device__ __forceinline__ void km_sweep_argmax(const AL& al, const KmP& p, float* smem, float* red_s, int* red_i, float& bs, int& bi)
{
    float* const As = smem;
    float* const Bs = smem + 2 * KmTile::floats;
    float* const stage = smem;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    const int row = t & (KM_B - 1), half = t >> 7;
    bs = -INFINITY;
    bi = half ? INT_MAX : 0;
    for (int ct = 0; ct < p.tiles_k; ++ct) {
        const int n0 = ct * KM_B;
        f32x16 acc[2][2];
        km_score_tile_with(al, p, n0, As, Bs, acc);
        {   // accumulator register r of lane l: row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of its block
            const int col_l = lane & 31, rsub = 4 * (lane >> 5);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        stage[(wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub) * KM_LST + wn0 + 32 * j + col_l] = acc[i][j][r];
        }
        __syncthreads();
        {
            const float* const rp = stage + row * KM_LST + 64 * half;
            const int c0 = n0 + 64 * half;
            const int nv = min(64, p.K - c0);                      // <= 0: nothing of this tile is mine
            for (int c = 0; c < nv; ++c) {
                const float v = rp[c];
                if (v > bs) { bs = v; bi = c0 + c; }
            }
        }
        __syncthreads();
    }
    if (half) { red_s[row] = bs; red_i[row] = bi; }
    __syncthreads();
    if (!half) {
        const float s1 = red_s[row];
        const int i1 = red_i[row];
        if (s1 > bs || (s1 == bs && i1 < bi)) { bs = s1; bi = i1; }
    }
}

}  // namespace abn
