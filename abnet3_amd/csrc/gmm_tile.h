// gmm_tile.h -- the fp32 score tile of the mixture kernels, shared by gmm.hip (abn_gmm_posteriors, abn_gmm_accumulate)
// and hmm.hip (abn_hmm_forward_backward): the 128 x 128 tile of s = [xc | xc^2 | 1] . [A | B | c] on the matrix cores,
// ka ascending, and the operand loaders that form the augmented rows on the way into LDS.  A caller that passes another
// third table for c (hmm.hip: c without the log weight) runs the SAME MFMA sequence and depth order over it.
// Also shared: the k-major X~ loaders of the statistics GEMM, the float64 slab sum and the (tile, range) grid with its
// workspace size (gmm.hip's abn_gmm_accumulate / abn_gmm_mstep, hmm.hip's abn_hmm_accumulate), and the score-only GmmP
// of every HMM entry (hmm_score_params: hmm.hip, hmm_dense.hip, hmm_dense_vit.hip).
#pragma once
#include "common.h"
#include "gemm_f32.h"

#include <math.h>

namespace abn {

constexpr int GM_B = 128;                  // frame block = component tile (2 x 2 waves of 2 x 2 MFMA blocks)
constexpr int GM_MAX_D = 127;              // 2 D + 1 <= 256 columns of statistics in one workgroup's accumulators
constexpr int GM_MAX_K = 4096;
constexpr int GM_MAX_RANGES = 256;
constexpr int GM_PT = GM_B * BK / 256;     // elements per thread of a 128 x 32 operand tile (scalar loads: D = 39 rows are not 16-byte aligned)
constexpr int GM_LST = GM_B + 1;           // likelihood pass: a thread walks its frame's row, 129 dwords apart = conflict-free
constexpr int GM_GST = GM_B + MPAD;        // accumulate pass: the staged tile IS a k-major operand (TileShape<128, false>::stride)
using GmTile = TileShape<GM_B, true>;
constexpr size_t GM_TILE_BYTES = sizeof(float) * 4 * GmTile::floats;      // two stages of each operand
static_assert(GM_TILE_BYTES >= sizeof(float) * GM_B * GM_GST, "the score tile is staged in the operand buffers");
static_assert(GM_GST == TileShape<GM_B, false>::stride, "frag_read<128, false> reads the staged responsibilities");
template <int BN> constexpr size_t gmm_accum_lds() { return GM_TILE_BYTES + sizeof(float) * 2 * TileShape<BN, false>::floats; }

struct GmmP {
    const float* x; const float* shift;
    const float* A; const float* B; const float* c;
    int T, K, D;
    float* lse;                 // likelihood pass: written; accumulate pass: read
    float* post;                // [T][K] or nullptr
    float* slabs;               // [tiles_k][n_ranges][128][2 D + 1]
    int tiles_k, fblocks, n_ranges, blocks_per_range;
};

// A GmmP for the score tile alone (the HMM kernels' emissions, c = c0): the likelihood and accumulate passes' fields are
// unused.
static inline GmmP hmm_score_params(const float* x, int64_t T, int64_t D, const float* shift, const float* A, const float* B,
                                    const float* c0, int64_t K)
{
    GmmP g;
    g.x = x; g.shift = shift; g.A = A; g.B = B; g.c = c0;
    g.T = (int)T; g.K = (int)K; g.D = (int)D;
    g.lse = nullptr; g.post = nullptr; g.slabs = nullptr;
    g.tiles_k = (int)((K + GM_B - 1) / GM_B); g.fblocks = 0; g.n_ranges = 0; g.blocks_per_range = 0;
    return g;
}

// Column ka of an augmented operand: 0 xc / A, 1 xc^2 / B, 2 the ones column / c, 3 the zero fill up to the k-tile.
__device__ __forceinline__ int aug_kind(int ka, int D) { return ka < D ? 0 : ka < 2 * D ? 1 : ka == 2 * D ? 2 : 3; }
__device__ __forceinline__ int aug_col(int ka, int D) { return ka < D ? ka : ka < 2 * D ? ka - D : 0; }

// One element of X~ from the raw value: centred in fp32, squared in fp32, a non-finite value contributes 0 (its
// frame is BAD: the likelihood pass marks it and nobody uses its scores).
__device__ __forceinline__ float aug_value(float raw, float sh, int kind, bool row_ok)
{
    const float xc = raw - sh, sq = xc * xc;
    float v = kind == 0 ? xc : kind == 1 ? sq : kind == 2 ? 1.0f : 0.0f;
    if (kind < 2 && !__builtin_isfinite(sq)) v = 0.0f;
    return row_ok ? v : 0.0f;
}

// 128 x 32 tiles, K-contiguous in LDS ([row][36]).  Thread t owns column k0 + (t & 31) of rows (t >> 5) + 8 i.
// Branch-free issue from clamped addresses, validity applied at commit (gemm_f32.h's tile_issue / tile_commit).
__device__ __forceinline__ void gmm_x_issue(float* r, const GmmP& p, int m0, int k0)
{
    const int t = threadIdx.x, ka = k0 + (t & 31), col = aug_col(ka, p.D);
    const bool kv = ka < 2 * p.D;
#pragma unroll
    for (int i = 0; i < GM_PT; ++i) {
        const int row = m0 + (t >> 5) + 8 * i;
        r[i] = p.x[(kv && row < p.T) ? (int64_t)row * p.D + col : 0];
    }
}
__device__ __forceinline__ void gmm_x_commit(const float* r, float* __restrict__ lds, const GmmP& p, int m0, int k0)
{
    const int t = threadIdx.x, ka = k0 + (t & 31), kind = aug_kind(ka, p.D);
    const float sh = p.shift[aug_col(ka, p.D)];
#pragma unroll
    for (int i = 0; i < GM_PT; ++i) {
        const int rl = (t >> 5) + 8 * i;
        lds[rl * GmTile::stride + (t & 31)] = aug_value(r[i], sh, kind, m0 + rl < p.T);
    }
}
__device__ __forceinline__ void gmm_w_issue(float* r, const GmmP& p, int n0, int k0)
{
    const int t = threadIdx.x, ka = k0 + (t & 31), kind = aug_kind(ka, p.D), col = aug_col(ka, p.D);
    const float* const base = kind == 0 ? p.A : kind == 1 ? p.B : p.c;
#pragma unroll
    for (int i = 0; i < GM_PT; ++i) {
        const int comp = n0 + (t >> 5) + 8 * i;
        const int64_t off = kind == 2 ? (int64_t)comp : (int64_t)comp * p.D + col;
        r[i] = base[(kind < 3 && comp < p.K) ? off : 0];
    }
}
__device__ __forceinline__ void gmm_w_commit(const float* r, float* __restrict__ lds, const GmmP& p, int n0, int k0)
{
    const int t = threadIdx.x, kind = aug_kind(k0 + (t & 31), p.D);
#pragma unroll
    for (int i = 0; i < GM_PT; ++i) {
        const int rl = (t >> 5) + 8 * i;
        lds[rl * GmTile::stride + (t & 31)] = (kind < 3 && n0 + rl < p.K) ? r[i] : 0.0f;
    }
}

// The 128 x 128 score tile of frames m0 .. and components n0 ..: rows = frames, columns = components, wave w owns
// the 64 x 64 block ((w >> 1) 64, (w & 1) 64).  The caller guarantees that nobody still reads the operand buffers;
// on return every wave has passed the last barrier, so the buffers are free again.
__device__ __forceinline__ void gmm_score_tile(const GmmP& p, int m0, int n0, float* As, float* Bs, f32x16 (&acc)[2][2])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    const int nkt = (2 * p.D + 1 + BK - 1) / BK;
    float ra[GM_PT], rb[GM_PT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    gmm_x_issue(ra, p, m0, 0);
    gmm_w_issue(rb, p, n0, 0);
    gmm_x_commit(ra, As, p, m0, 0);
    gmm_w_commit(rb, Bs, p, n0, 0);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nkt;
        const float* as = As + cur * GmTile::floats;
        const float* bs = Bs + cur * GmTile::floats;
        if (more) {
            gmm_x_issue(ra, p, m0, (kt + 1) * BK);
            gmm_w_issue(rb, p, n0, (kt + 1) * BK);
        }
#pragma unroll
        for (int g = 0; g < BK / 8; ++g) {
            f32x4 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = frag_read<GM_B, true>(as, wm0 + 32 * i, g, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = frag_read<GM_B, true>(bs, wn0 + 32 * j, g, lane);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
        }
        if (more) {
            gmm_x_commit(ra, As + (cur ^ 1) * GmTile::floats, p, m0, (kt + 1) * BK);
            gmm_w_commit(rb, Bs + (cur ^ 1) * GmTile::floats, p, n0, (kt + 1) * BK);
        }
        __syncthreads();
    }
}

// Second GEMM's B operand: 32 frames x BN columns of X~, k-major in LDS ([frame][BN + 4]); thread t owns column
// t % BN of frames t / BN + (256 / BN) i.
template <int BN>
__device__ __forceinline__ void gmm_xk_issue(float* r, const GmmP& p, int f0)
{
    constexpr int PT = 32 * BN / 256, FS = 256 / BN > 0 ? 256 / BN : 1;
    const int t = threadIdx.x, ka = t % BN, col = aug_col(ka, p.D);
    const bool kv = ka < 2 * p.D;
#pragma unroll
    for (int i = 0; i < PT; ++i) {
        const int f = f0 + (BN >= 256 ? i : t / BN + FS * i);
        r[i] = p.x[(kv && f < p.T) ? (int64_t)f * p.D + col : 0];
    }
}
template <int BN>
__device__ __forceinline__ void gmm_xk_commit(const float* r, float* __restrict__ lds, const GmmP& p, int f0)
{
    constexpr int PT = 32 * BN / 256, FS = 256 / BN > 0 ? 256 / BN : 1, ST = TileShape<BN, false>::stride;
    const int t = threadIdx.x, ka = t % BN, kind = aug_kind(ka, p.D);
    const float sh = p.shift[aug_col(ka, p.D)];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
        const int fl = BN >= 256 ? i : t / BN + FS * i;
        lds[fl * ST + ka] = aug_value(r[i], sh, kind, f0 + fl < p.T);
    }
}

// Column threadIdx.x of component k's statistics = its slabs [tile][range][128][nc] summed in range order, in float64
// (gmm.hip's gmm_reduce_kernel and hmm.hip's hmm_sums_kernel: one workgroup of at least nc threads per component).
__device__ __forceinline__ void gmm_sum_slabs(const float* __restrict__ slabs, int k, int nc, int n_ranges,
                                              double* __restrict__ sums)
{
    const int t = threadIdx.x;
    if (t >= nc) return;
    const float* src = slabs + ((int64_t)(k / GM_B) * n_ranges * GM_B + (k % GM_B)) * nc + t;
    double a = 0.0;
    for (int r = 0; r < n_ranges; ++r) a += (double)src[(int64_t)r * GM_B * nc];
    sums[(int64_t)k * nc + t] = a;
}

// The accumulate passes' grid: component tiles x frame ranges (gmm.hip, hmm.hip's abn_hmm_accumulate).
struct GmmGrid { int tiles_k, fblocks, n_ranges, blocks_per_range; };
static GmmGrid gmm_grid(int64_t T, int64_t K, int n_ranges)
{
    GmmGrid g;
    g.tiles_k = (int)((K + GM_B - 1) / GM_B);
    g.fblocks = (int)((T + GM_B - 1) / GM_B);
    int r = n_ranges;
    if (r <= 0) r = (1024 + g.tiles_k - 1) / g.tiles_k;      // auto: four workgroups per CU's worth of (tile, range) pairs
    if (r > GM_MAX_RANGES) r = GM_MAX_RANGES;
    if (r > g.fblocks) r = g.fblocks;
    g.blocks_per_range = (g.fblocks + r - 1) / r;
    g.n_ranges = (g.fblocks + g.blocks_per_range - 1) / g.blocks_per_range;
    return g;
}

// Workspace: one slab per (component tile, range).  Sized by a bound on the pairs that does not shrink when T or K grow
// (the ranges themselves do, where one more frame block tips blocks_per_range over).
static int64_t gmm_slab_bytes(const GmmGrid& g, int64_t D, int n_ranges)
{
    int64_t pairs;
    if (n_ranges > 0) pairs = (int64_t)g.tiles_k * (n_ranges < g.fblocks ? n_ranges : g.fblocks);
    else {
        pairs = 1024 + g.tiles_k;
        if (pairs > (int64_t)g.tiles_k * GM_MAX_RANGES) pairs = (int64_t)g.tiles_k * GM_MAX_RANGES;
        if (pairs > (int64_t)g.tiles_k * g.fblocks) pairs = (int64_t)g.tiles_k * g.fblocks;
    }
    return pairs * GM_B * (2 * D + 1) * (int64_t)sizeof(float);
}

}  // namespace abn
