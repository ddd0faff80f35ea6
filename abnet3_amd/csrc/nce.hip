// nce.hip -- the in-batch contrastive pair loss (InfoNCE / NT-Xent) and its gradient (abnt_nce_loss).
// abnet3_amd/loss.py (InfoNCELoss) states the definition, tests/nce_np.py restates it, DESIGN.md section 3.4k has the
// shape and the error derivation.
//
// s[i][j] = <a^_i, b^_j> over unit rows is the 128 x 128 exact-fp32 MFMA tile of knn.hip (v_mfma_f32_32x32x2_f32, k
// ascending, gemm_f32.h's K-contiguous tiles and loaders); the B x B matrix never reaches memory.  The tile's operands are
// the unit rows LESS THEIR MEAN mu (alpha_i = a^_i - mu, beta_j = b^_j - mu): s = |mu|^2 + <alpha_i, mu> + <mu, beta_j> +
// <alpha_i, beta_j>, the first term shifts every logit alike and drops out of every term and gradient, the two row terms
// are float64 dots rounded once, and only the last is an fp32 chain -- over short vectors where the embeddings are nearly
// parallel (sigmoid outputs: cosines 0.9 .. 1), which is where a chain that sums to 1 loses the digits the loss lives on.
// Nine launches, none of which waits for another workgroup:
//   * nce_norm_kernel (a wave per row: the norm in float64, 1 / max(norm, 1e-6), r[i] = (y[i] == 1)), nce_colsum_kernel +
//     nce_mu_kernel (mu in float64, fixed order, each side summed on its own so that swapping the sides changes nothing),
//     nce_center_kernel (a wave per row: alpha in float64, rounded once, zeros up to a multiple of four columns for the
//     tiles' 16-byte loads; <alpha, mu>).
//   * nce_lse_kernel: a workgroup owns a direction, 128 rows and a range of candidate tiles.  Direction 0 is a^ against
//     every b^ (la), direction 1 the SAME code with the sides swapped (lb): a product of two floats does not depend on
//     their order and k ascends either way, so the tile of (b^, a^) holds the transposed bits of the tile of (a^, b^).
//     Each tile goes through LDS as z = (tile + (row term + column term)) / tau (nce_logit: the inner sum is the same
//     float in either order, one correctly rounded division); two threads per row fold 64 columns each into a running (max, sum).
//     Padding columns and excluded cells are skipped, never weighted.  z[i][i] is kept from the tile that holds it.
//   * nce_merge_kernel: a thread per row merges the ranges' partials in range order, la = m + log(S), and forms
//     l[i] = ((la - z_ii) + (lb - z_ii)) / 2 with each bracket clamped at 0: z_ii is the very float that went into both
//     sums, so a bracket can only be negative by the rounding of expf / logf.
//   * nce_sum_kernel: one workgroup, the anchors counted and their terms summed in float64 in a fixed order.
//   * nce_grad_kernel (per side, the same code with the sides swapped): a workgroup owns 128 rows rho of its side and a
//     range of candidate tiles kappa.  Each tile is recomputed with the candidates as the tile's ROWS (the same bits,
//     transposed), G = c (r[rho] exp(z - L_row[rho]) + r[kappa] exp(z - L_cand[kappa]) - 2 r[rho] [rho == kappa]) is
//     written to LDS as the k-major operand of the second GEMM, g[rho][.] += sum_kappa G[kappa][rho] c^[kappa][.]
//     (gmm_accum_kernel's mechanism) over the centred candidates; the [128][D] accumulators stay in registers over the
//     range and leave as one slab, with the rows' sums of G (the weight of mu in g) beside it.
//   * nce_finish_kernel: one wave per row sums the slabs in range order and applies the normalisation's derivative,
//     d e = (g - u <u, g>) inv (the projection only where norm >= 1e-6), and the 1 / n of `avg`, in float64.
// No floating-point atomics, every sum has one fixed order: two calls give the same bits.
#include "common.h"
#include "gemm_f32.h"
#include "../../include/abnet3_hip_next.h"

#include <math.h>
#include <stdlib.h>

namespace abn {

constexpr int NC_B = 128;                   // row block = candidate tile (2 x 2 waves of 2 x 2 MFMA blocks)
constexpr int NC_SST = NC_B + 1;            // lse sweep: a thread walks its row, 129 dwords apart = conflict-free
constexpr int NC_GST = NC_B + MPAD;         // gradient sweep: the staged G IS a k-major operand
constexpr int NC_MAX_D = 256;               // the gradient accumulators: [128][256] over four waves = 128 registers a lane
constexpr int NC_MAX_SPLIT = 16;
constexpr int64_t NC_MAX_B = 1 << 20;
constexpr double NC_EPS = 1e-6;
using NcTile = TileShape<NC_B, true>;
constexpr size_t NC_TILE_BYTES = sizeof(float) * 4 * NcTile::floats;           // two stages of each operand
static_assert(NC_TILE_BYTES >= sizeof(float) * NC_B * NC_SST, "the similarity tile is staged in the operand buffers");
static_assert(NC_TILE_BYTES >= sizeof(float) * NC_B * NC_GST, "G is staged in the operand buffers");
static_assert(NC_GST == TileShape<NC_B, false>::stride, "frag_read<128, false> reads the staged G");
template <int BN> constexpr size_t nce_grad_lds() { return NC_TILE_BYTES + sizeof(float) * 2 * TileShape<BN, false>::floats; }

struct NceP {
    const float* e[2]; const void* y; int y_dtype;
    const int32_t* grp;
    int B, D, dp;
    float tau, c0; int avg;
    int rblocks, tiles, split, tiles_per_split;
    float* U[2];                 // [B][dp] unit rows less their common shift mu
    double* invd; float* prj;    // [2][B]
    float* rc;                   // [2][B] <row, mu>
    double* mu;                  // [dp]
    double* cpart;               // [cblk][2][dp] column sums of the unit rows, per block of crows rows
    int cblk, crows;
    double* wsl;                 // [2][split][B] row sums of G
    float* rv;                   // [B]
    float* part;                 // [2][split][B][2]
    float* diag;                 // [B]
    float* L;                    // [2][B]
    float* tws;                  // [B]
    float* scale;                // [1]
    float* slabs;                // [2][split][B][dp]
    float* loss; float* terms; float* de[2];
};

__device__ __forceinline__ bool nce_is_anchor(const void* y, int dt, int64_t i)
{
    switch (dt) {
    case 0: return static_cast<const int8_t*>(y)[i] == 1;
    case 1: return static_cast<const int32_t*>(y)[i] == 1;
    case 2: return static_cast<const int64_t*>(y)[i] == 1;
    case 3: return static_cast<const float*>(y)[i] == 1.0f;
    default: return static_cast<const double*>(y)[i] == 1.0;
    }
}

// One wave per row: the norm in float64, 1 / max(norm, eps), the projection flag, the anchor flag.
__global__ __launch_bounds__(256) void nce_norm_kernel(NceP p)
{
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= 2 * (int64_t)p.B) return;
    const int side = w >= p.B, i = (int)(w - (int64_t)side * p.B), lane = threadIdx.x & 63;
    const float* const src = p.e[side] + (int64_t)i * p.D;
    double ss = 0.0;
    for (int d = lane; d < p.D; d += 64) ss += (double)src[d] * (double)src[d];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const double nrm = sqrt(ss);
    if (lane == 0) {
        p.invd[(int64_t)side * p.B + i] = 1.0 / fmax(nrm, NC_EPS);
        p.prj[(int64_t)side * p.B + i] = nrm >= NC_EPS ? 1.0f : 0.0f;
        if (side == 0) p.rv[i] = nce_is_anchor(p.y, p.y_dtype, i) ? 1.0f : 0.0f;
    }
}

// Block b: the column sums of both sides' unit rows over rows b crows .., thread t column t, rows in order, float64.
__global__ __launch_bounds__(256) void nce_colsum_kernel(NceP p)
{
    const int t = threadIdx.x, b = (int)blockIdx.x;
    if (t >= p.dp) return;
    const int i0 = b * p.crows, i1 = min(p.B, i0 + p.crows);
    double sa = 0.0, sb = 0.0;
    if (t < p.D)
        for (int i = i0; i < i1; i += 8) {                       // eight rows' loads in flight, added in row order
            double va[8], vb[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int r = min(i + k, i1 - 1);
                va[k] = (double)p.e[0][(int64_t)r * p.D + t] * p.invd[r];
                vb[k] = (double)p.e[1][(int64_t)r * p.D + t] * p.invd[(int64_t)p.B + r];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (i + k < i1) { sa += va[k]; sb += vb[k]; }
        }
    p.cpart[((int64_t)b * 2) * p.dp + t] = sa;
    p.cpart[((int64_t)b * 2 + 1) * p.dp + t] = sb;
}

// mu = the mean of all 2 B unit rows: each side's partials in block order, then the two sides added (either order: the same).
__global__ __launch_bounds__(256) void nce_mu_kernel(NceP p)
{
    const int t = threadIdx.x;
    if (t >= p.dp) return;
    double sa = 0.0, sb = 0.0;
    for (int b = 0; b < p.cblk; b += 8) {                        // eight blocks' loads in flight, added in block order
        double va[8], vb[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int r = min(b + k, p.cblk - 1);
            va[k] = p.cpart[((int64_t)r * 2) * p.dp + t];
            vb[k] = p.cpart[((int64_t)r * 2 + 1) * p.dp + t];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (b + k < p.cblk) { sa += va[k]; sb += vb[k]; }
    }
    p.mu[t] = (sa + sb) / (2.0 * (double)p.B);
}

// One wave per row: the row less mu, formed in float64 and rounded once, zeros up to dp; rc = <the rounded row, mu>.
__global__ __launch_bounds__(256) void nce_center_kernel(NceP p)
{
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= 2 * (int64_t)p.B) return;
    const int side = w >= p.B, i = (int)(w - (int64_t)side * p.B), lane = threadIdx.x & 63;
    const float* const src = p.e[side] + (int64_t)i * p.D;
    const double inv = p.invd[(int64_t)side * p.B + i];
    float* const dst = p.U[side] + (int64_t)i * p.dp;
    double dot = 0.0;
    for (int d = lane; d < p.dp; d += 64) {
        const double m = p.mu[d];
        const float a = d < p.D ? (float)((double)src[d] * inv - m) : 0.0f;
        dst[d] = a;
        dot += (double)a * m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    if (lane == 0) p.rc[(int64_t)side * p.B + i] = (float)dot;
}

// The logit of a cell from its tile entry <alpha, beta> and the two rows' <., mu>: the similarity less |mu|^2, which shifts
// every logit alike and so changes neither a term nor a gradient.  x + y is the same float in either order, so the transposed
// tile gives the same bits; one correctly rounded division.
__device__ __forceinline__ float nce_logit(float acc, float x, float y, float tau) { return __fdiv_rn(acc + (x + y), tau); }

// The 128 x 128 tile of <X[m0 + .], Y[n0 + .]> over unit rows [n][dp]: rows = X, columns = Y, wave w owns the 64 x 64 block
// ((w >> 1) 64, (w & 1) 64); one MFMA chain over k = 0, 2, 4, ... per cell.  The caller guarantees that nobody still reads
// the operand buffers; on return every wave has passed the last barrier, so the buffers are free again.
__device__ __forceinline__ void nce_score_tile(const float* __restrict__ X, const float* __restrict__ Y, int n, int dp, int m0,
                                               int n0, float* As, float* Bs, f32x16 (&acc)[2][2])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    const int nkt = (dp + BK - 1) / BK;
    f32x4 ra[NcTile::per_thread], rb[NcTile::per_thread];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    tile_issue<NC_B, true, true, false>(ra, X, dp, n, m0, 0, dp);
    tile_issue<NC_B, true, true, false>(rb, Y, dp, n, n0, 0, dp);
    tile_commit<NC_B, true, false>(ra, As, n, m0, 0, dp, -1);
    tile_commit<NC_B, true, false>(rb, Bs, n, n0, 0, dp, -1);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nkt;
        const float* as = As + cur * NcTile::floats;
        const float* bs = Bs + cur * NcTile::floats;
        if (more) {
            tile_issue<NC_B, true, true, false>(ra, X, dp, n, m0, (kt + 1) * BK, dp);
            tile_issue<NC_B, true, true, false>(rb, Y, dp, n, n0, (kt + 1) * BK, dp);
        }
#pragma unroll
        for (int g = 0; g < BK / 8; ++g) {
            f32x4 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = frag_read<NC_B, true>(as, wm0 + 32 * i, g, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = frag_read<NC_B, true>(bs, wn0 + 32 * j, g, lane);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
        }
        if (more) {
            tile_commit<NC_B, true, false>(ra, As + (cur ^ 1) * NcTile::floats, n, m0, (kt + 1) * BK, dp, -1);
            tile_commit<NC_B, true, false>(rb, Bs + (cur ^ 1) * NcTile::floats, n, n0, (kt + 1) * BK, dp, -1);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void nce_lse_kernel(NceP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const As = smem;
    float* const Bs = smem + 2 * NcTile::floats;
    float* const stage = smem;
    __shared__ float red_m[256], red_s[256];
    __shared__ int32_t gcol[NC_B];
    __shared__ float xrow[NC_B], xcol[NC_B];                 // <row, mu> of the tile's rows and columns

    const int per_dir = p.rblocks * p.split;
    const int dir = (int)blockIdx.x / per_dir, w = (int)blockIdx.x % per_dir;
    const int rb = w / p.split, s = w % p.split;
    const float* const X = p.U[dir];
    const float* const Y = p.U[dir ^ 1];
    const int m0 = rb * NC_B;
    const int t0 = s * p.tiles_per_split, t1 = min(p.tiles, t0 + p.tiles_per_split);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    const int row = t & (NC_B - 1), half = t >> 7;       // this thread's row and its 64 columns of every tile
    const int i = m0 + row;
    const bool masked = p.grp != nullptr;
    const int32_t gi = (masked && i < p.B) ? p.grp[i] : 0;

    float m = -INFINITY, sum = 0.0f;
    for (int ct = t0; ct < t1; ++ct) {
        const int n0 = ct * NC_B;
        if (masked && t < NC_B) gcol[t] = (n0 + t < p.B) ? p.grp[n0 + t] : 0;      // (its readers are barriers behind)
        if (t < NC_B) {
            xcol[t] = (n0 + t < p.B) ? p.rc[(int64_t)(dir ^ 1) * p.B + n0 + t] : 0.0f;
            if (ct == t0) xrow[t] = (m0 + t < p.B) ? p.rc[(int64_t)dir * p.B + m0 + t] : 0.0f;
        }
        f32x16 acc[2][2];
        nce_score_tile(X, Y, p.B, p.dp, m0, n0, As, Bs, acc);
        {   // accumulator register r of lane l: row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of its block
            const int col_l = lane & 31, rsub = 4 * (lane >> 5);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int rl = wm0 + 32 * a + (r & 3) + 8 * (r >> 2) + rsub, cl = wn0 + 32 * b + col_l;
                        stage[rl * NC_SST + cl] = nce_logit(acc[a][b][r], xrow[rl], xcol[cl], p.tau);
                    }
        }
        __syncthreads();
        {
            const int c0 = 64 * half, j0 = n0 + c0;
            const float* const rp = stage + row * NC_SST + c0;
            const int nv = min(64, p.B - j0);                          // <= 0: nothing of this tile is mine
            float tm = -INFINITY;
            for (int c = 0; c < nv; ++c) {
                const bool ok = !masked || j0 + c == i || gcol[c0 + c] != gi;
                if (ok) tm = fmaxf(tm, rp[c]);
            }
            if (tm > -INFINITY) {
                const float mn = fmaxf(m, tm);
                float a = 0.0f;
                for (int c = 0; c < nv; ++c) {
                    const bool ok = !masked || j0 + c == i || gcol[c0 + c] != gi;
                    if (ok) a += expf(rp[c] - mn);
                }
                sum = sum * expf(m - mn) + a;
                m = mn;
            }
            if (dir == 0 && i < p.B && i >= j0 && i < j0 + 64) p.diag[i] = rp[i - j0];
        }
        __syncthreads();
    }
    red_m[t] = m;
    red_s[t] = sum;
    __syncthreads();
    if (t < NC_B && i < p.B) {
        const float m1 = red_m[t], m2 = red_m[t + NC_B], mn = fmaxf(m1, m2);
        float S = 0.0f;
        if (mn > -INFINITY) S = red_s[t] * expf(m1 - mn) + red_s[t + NC_B] * expf(m2 - mn);
        float* const dst = p.part + (((int64_t)dir * p.split + s) * p.B + i) * 2;
        dst[0] = mn;
        dst[1] = S;
    }
}

__global__ __launch_bounds__(256) void nce_merge_kernel(NceP p)
{
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.B) return;
    float l[2];
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        float m = -INFINITY, S = 0.0f;
        for (int s = 0; s < p.split; ++s) {
            const float* const src = p.part + (((int64_t)dir * p.split + s) * p.B + i) * 2;
            const float pm = src[0], ps = src[1];
            if (pm > -INFINITY) {
                const float mn = fmaxf(m, pm);
                S = S * expf(m - mn) + ps * expf(pm - mn);
                m = mn;
            }
        }
        l[dir] = m + logf(S);
        p.L[(int64_t)dir * p.B + i] = l[dir];
    }
    const float z = p.diag[i];
    const float term = 0.5f * (fmaxf(l[0] - z, 0.0f) + fmaxf(l[1] - z, 0.0f));
    p.tws[i] = term;
    if (p.terms) p.terms[i] = term;
}

// 256 doubles of LDS summed in a fixed tree; the result is returned to every thread.
__device__ __forceinline__ double nce_block_sum(double v, double* sh)
{
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(256) void nce_sum_kernel(NceP p)
{
    __shared__ double sh[256];
    double n = 0.0, a = 0.0;
    for (int i = threadIdx.x; i < p.B; i += 256)
        if (p.rv[i] != 0.0f) { n += 1.0; a += (double)p.tws[i]; }
    n = nce_block_sum(n, sh);
    a = nce_block_sum(a, sh);
    if (threadIdx.x == 0) {
        const bool mean = p.avg && n > 0.0;
        p.loss[0] = n > 0.0 ? (float)(mean ? a / n : a) : 0.0f;
        p.scale[0] = n > 0.0 ? (float)(mean ? 1.0 / n : 1.0) : 0.0f;
    }
}

template <int BN>
__global__ __launch_bounds__(256) void nce_grad_kernel(NceP p)
{
    constexpr int TN = BN / 64;
    using XT = TileShape<BN, false>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const As = smem;
    float* const Bs = smem + 2 * NcTile::floats;
    float* const G = smem;                                  // [128 candidates][132]: four k-major tiles of 32 candidates
    float* const Xk = smem + 4 * NcTile::floats;            // two stages of [32][BN + 4]
    __shared__ float lrow_s[NC_B], rrow_s[NC_B], lc_s[NC_B], rc_s[NC_B], xrow_s[NC_B], xc_s[NC_B];
    __shared__ int32_t grow_s[NC_B], gc_s[NC_B];
    __shared__ double wsum_s[2 * NC_B];                         // thread t's sum over the range of G[.][rho = n0 + t] (LDS: no registers to spare)

    const int per_side = p.rblocks * p.split;
    const int side = (int)blockIdx.x / per_side, w = (int)blockIdx.x % per_side;
    const int rb = w / p.split, s = w % p.split;
    const float* const X = p.U[side];                        // the owned rows rho: the tile's columns
    const float* const Y = p.U[side ^ 1];                    // the candidates kappa: the tile's rows, the second GEMM's depth
    const float* const Lrow = p.L + (int64_t)side * p.B;
    const float* const Lcand = p.L + (int64_t)(side ^ 1) * p.B;
    const int n0 = rb * NC_B;
    const int t0 = s * p.tiles_per_split, t1 = min(p.tiles, t0 + p.tiles_per_split);
    const bool masked = p.grp != nullptr;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;         // score tile: candidates x owned rows
    const int wc0 = (wave >> 1) * 64, wx0 = (wave & 1) * (BN / 2);   // gradient tile: owned rows x columns
    const int col_l = lane & 31, rsub = 4 * (lane >> 5);

    if (t < NC_B) {
        const int rho = n0 + t;
        const bool in = rho < p.B;
        lrow_s[t] = in ? Lrow[rho] : 0.0f;
        xrow_s[t] = in ? p.rc[(int64_t)side * p.B + rho] : 0.0f;
        rrow_s[t] = in ? p.rv[rho] : 0.0f;
        grow_s[t] = (in && masked) ? p.grp[rho] : 0;
    }

    wsum_s[t] = 0.0;
    f32x16 st[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[i][j][r] = 0.0f;

    for (int ct = t0; ct < t1; ++ct) {
        const int m0 = ct * NC_B;
        if (t < NC_B) {                                              // (its readers are barriers behind)
            const int kap = m0 + t;
            const bool in = kap < p.B;
            lc_s[t] = in ? Lcand[kap] : 0.0f;
            xc_s[t] = in ? p.rc[(int64_t)(side ^ 1) * p.B + kap] : 0.0f;
            rc_s[t] = in ? p.rv[kap] : 0.0f;
            gc_s[t] = (in && masked) ? p.grp[kap] : 0;
        }
        f32x16 acc[2][2];
        nce_score_tile(Y, X, p.B, p.dp, m0, n0, As, Bs, acc);
        f32x4 rx[XT::per_thread];
        tile_issue<BN, false, true, false>(rx, Y, p.dp, p.dp, 0, m0, p.B);
        // G: exactly 0 past the last row of either side and in an excluded cell
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kl = wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub, cl = wn0 + 32 * j + col_l;
                    const int kap = m0 + kl, rho = n0 + cl;
                    const bool ok = kap < p.B && rho < p.B && (!masked || kap == rho || gc_s[kl] != grow_s[cl]);
                    const float z = nce_logit(acc[i][j][r], xc_s[kl], xrow_s[cl], p.tau);
                    const float rr = rrow_s[cl], rk = rc_s[kl];
                    float v = rr * expf(z - lrow_s[cl]) + rk * expf(z - lc_s[kl]);
                    if (kap == rho) v -= 2.0f * rr;
                    G[kl * NC_GST + cl] = ok ? p.c0 * v : 0.0f;
                    if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // (four cells at a time: the exps of all 64 in flight cost registers the accumulators need)
                }
        tile_commit<BN, false, false>(rx, Xk, p.dp, 0, m0, p.B, -1);
        __syncthreads();
        {   // row (t & 127)'s sum of G over this tile's candidates: each half of them in order, the halves added below
            const int k0 = (t >> 7) * (NC_B / 2);
            double a = 0.0;
#pragma unroll 8
            for (int k = k0; k < k0 + NC_B / 2; ++k) a += (double)G[k * NC_GST + (t & (NC_B - 1))];
            wsum_s[t] += a;
        }
        for (int q = 0; q < NC_B / BK; ++q) {
            const float* const gs = G + q * BK * NC_GST;
            const float* const xs = Xk + (q & 1) * XT::floats;
            const bool more = q + 1 < NC_B / BK;
            if (more) tile_issue<BN, false, true, false>(rx, Y, p.dp, p.dp, 0, m0 + (q + 1) * BK, p.B);
#pragma unroll
            for (int g = 0; g < BK / 8; ++g) {
                f32x4 fa[2], fx[TN];
#pragma unroll
                for (int i = 0; i < 2; ++i) fa[i] = frag_read<NC_B, false>(gs, wc0 + 32 * i, g, lane);
#pragma unroll
                for (int j = 0; j < TN; ++j) fx[j] = frag_read<BN, false>(xs, wx0 + 32 * j, g, lane);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            st[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fx[j][e], st[i][j], 0, 0, 0);
            }
            if (more) tile_commit<BN, false, false>(rx, Xk + ((q + 1) & 1) * XT::floats, p.dp, 0, m0 + (q + 1) * BK, p.B, -1);
            __syncthreads();
        }
    }

    if (t < NC_B && n0 + t < p.B) p.wsl[((int64_t)side * p.split + s) * p.B + n0 + t] = wsum_s[t] + wsum_s[t + NC_B];
    // the workgroup's one slab: its 128 rows of [B][dp]
    float* const slab = p.slabs + ((int64_t)side * p.split + s) * p.B * p.dp;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rho = n0 + wc0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub, col = wx0 + 32 * j + col_l;
                if (rho < p.B && col < p.dp) slab[(int64_t)rho * p.dp + col] = st[i][j][r];
            }
}

// One wave per (side, row): the slabs in range order, <u, g> over the lanes in a fixed tree, the projection, inv and 1 / n.
// In float64, rounded once at the end: where the candidates are nearly parallel to the row (sigmoid embeddings), g is nearly
// parallel to u and g - u <u, g> cancels most of it -- a rounded fp32 dot would be the largest error of the whole gradient.
__global__ __launch_bounds__(256) void nce_finish_kernel(NceP p)
{
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= 2 * (int64_t)p.B) return;
    const int side = w >= p.B, i = (int)(w - (int64_t)side * p.B), lane = threadIdx.x & 63;
    const float* const al = p.U[side] + (int64_t)i * p.dp;
    double ws = 0.0;                                                 // sum_j G[i][j]: the weight of mu in g
    for (int s = 0; s < p.split; ++s) ws += p.wsl[((int64_t)side * p.split + s) * p.B + i];
    double g[NC_MAX_D / 64], u[NC_MAX_D / 64];
    double dot = 0.0;
#pragma unroll
    for (int k = 0; k < NC_MAX_D / 64; ++k) {
        const int d = lane + 64 * k;
        double a = 0.0, uu = 0.0;
        if (d < p.D) {
            const float* src = p.slabs + ((int64_t)side * p.split * p.B + i) * p.dp + d;
            for (int s = 0; s < p.split; ++s) a += (double)src[(int64_t)s * p.B * p.dp];
            const double m = p.mu[d];
            a += ws * m;
            uu = (double)al[d] + m;                                  // the unit row: the stored row plus mu
            dot += uu * a;
        }
        g[k] = a;
        u[k] = uu;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    const double f = p.invd[(int64_t)side * p.B + i] * (double)p.scale[0];
    dot *= (double)p.prj[(int64_t)side * p.B + i];
    float* const dst = p.de[side] + (int64_t)i * p.D;
#pragma unroll
    for (int k = 0; k < NC_MAX_D / 64; ++k) {
        const int d = lane + 64 * k;
        if (d < p.D) dst[d] = (float)((g[k] - u[k] * dot) * f);
    }
}

// The candidate split and the workspace's layout, shared by the sizing query and the entry.  ABN_NCE_SPLIT (1 .. 16) forces
// the split; it is read from the environment at every call (a host getenv, no kernel depends on when), so a test that sets
// it needs no reload.  0 / unset: by the grid -- one workgroup per CU over both directions where the tiles allow it.
struct NceGrid { int rblocks, tiles, split, tiles_per_split, dp, cblk, crows; int64_t off[14], bytes; };
static NceGrid nce_grid(int64_t B, int64_t D)
{
    NceGrid g;
    g.rblocks = g.tiles = (int)((B + NC_B - 1) / NC_B);
    g.dp = (int)align_up(D, 4);
    const char* v = getenv("ABN_NCE_SPLIT");
    int s = v ? atoi(v) : 0;
    if (s <= 0) s = (256 + 2 * g.rblocks - 1) / (2 * g.rblocks);
    if (s > NC_MAX_SPLIT) s = NC_MAX_SPLIT;
    if (s > g.tiles) s = g.tiles;
    g.tiles_per_split = (g.tiles + s - 1) / s;
    g.split = (g.tiles + g.tiles_per_split - 1) / g.tiles_per_split;
    const int64_t row = align_up(B * 4, 16);
    g.cblk = (int)((B + 63) / 64 < 64 ? (B + 63) / 64 : 64);      // blocks of the column sums, whole rows each
    g.crows = (int)((B + g.cblk - 1) / g.cblk);
    const int64_t sizes[14] = {B * g.dp * 4, B * g.dp * 4, 2 * B * 8, 2 * row, row, align_up(2 * g.split * B * 8, 16), row, 2 * row,
                               row, 16, 2 * row, (int64_t)g.dp * 8, (int64_t)g.cblk * 2 * g.dp * 8, align_up(2 * g.split * B * 8, 16)};
    int64_t o = 0;
    for (int k = 0; k < 14; ++k) { g.off[k] = o; o += sizes[k]; }
    g.bytes = o + 2 * g.split * B * g.dp * 4;                 // the slabs come last
    return g;
}

static int nce_check_sizes(int64_t B, int64_t D, const char* what)
{
    ABN_REQUIRE(B >= 1 && D >= 1, "%s: B = %lld, D = %lld out of range", what, (long long)B, (long long)D);
    if (D > NC_MAX_D || B > NC_MAX_B) {
        set_error("%s: B = %lld, D = %lld, supported D <= %d (abnt_nce_max_d), B <= %lld", what, (long long)B, (long long)D,
                  NC_MAX_D, (long long)NC_MAX_B);
        return ABN_E_UNSUPPORTED;
    }
    return ABN_OK;
}

}  // namespace abn

using namespace abn;

extern "C" int64_t abnt_nce_max_d(void) { return NC_MAX_D; }

extern "C" int64_t abnt_nce_ws_bytes(int64_t B, int64_t D)
{
    if (nce_check_sizes(B, D, "abnt_nce_ws_bytes") != ABN_OK) return -1;
    return nce_grid(B, D).bytes;
}

extern "C" int abnt_nce_loss(const float* e1, const float* e2, const void* y, int y_dtype, const int32_t* groups, int64_t B,
                             int64_t D, float tau, int avg, float* loss, float* terms, float* de1, float* de2, void* ws,
                             void* stream)
{
    const int rc = nce_check_sizes(B, D, "abnt_nce_loss");
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(e1 && e2 && y && loss && ws, "abnt_nce_loss: null pointer");
    ABN_REQUIRE(y_dtype >= 0 && y_dtype <= 4, "abnt_nce_loss: y_dtype = %d, supported 0 .. 4", y_dtype);
    const float inv_tau = (float)(1.0 / (double)tau);
    ABN_REQUIRE(__builtin_isfinite(tau) && tau > 0.0f && __builtin_isfinite(inv_tau), "abnt_nce_loss: tau = %g must be finite and > 0",
                (double)tau);
    ABN_REQUIRE((de1 != nullptr) == (de2 != nullptr), "abnt_nce_loss: de1 and de2 go together (both null: forward only)");
    ABN_REQUIRE(aligned16(ws), "abnt_nce_loss: the workspace must be 16-byte aligned");

    const NceGrid g = nce_grid(B, D);
    char* const base = static_cast<char*>(ws);
    NceP p;
    p.e[0] = e1; p.e[1] = e2; p.y = y; p.y_dtype = y_dtype; p.grp = groups;
    p.B = (int)B; p.D = (int)D; p.dp = g.dp;
    p.tau = tau; p.c0 = (float)(0.5 / (double)tau); p.avg = avg != 0;
    p.rblocks = g.rblocks; p.tiles = g.tiles; p.split = g.split; p.tiles_per_split = g.tiles_per_split;
    p.U[0] = reinterpret_cast<float*>(base + g.off[0]);
    p.U[1] = reinterpret_cast<float*>(base + g.off[1]);
    p.invd = reinterpret_cast<double*>(base + g.off[2]);
    p.prj = reinterpret_cast<float*>(base + g.off[3]);
    p.rv = reinterpret_cast<float*>(base + g.off[4]);
    p.part = reinterpret_cast<float*>(base + g.off[5]);
    p.diag = reinterpret_cast<float*>(base + g.off[6]);
    p.L = reinterpret_cast<float*>(base + g.off[7]);
    p.tws = reinterpret_cast<float*>(base + g.off[8]);
    p.scale = reinterpret_cast<float*>(base + g.off[9]);
    p.rc = reinterpret_cast<float*>(base + g.off[10]);
    p.mu = reinterpret_cast<double*>(base + g.off[11]);
    p.cpart = reinterpret_cast<double*>(base + g.off[12]);
    p.wsl = reinterpret_cast<double*>(base + g.off[13]);
    p.cblk = g.cblk; p.crows = g.crows;
    p.slabs = reinterpret_cast<float*>(base + g.off[13] + align_up(2 * g.split * B * 8, 16));
    p.loss = loss; p.terms = terms; p.de[0] = de1; p.de[1] = de2;

    hipStream_t st = static_cast<hipStream_t>(stream);
    static bool attr_set[16] = {};
    if (first_use_on_device(attr_set)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nce_lse_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)NC_TILE_BYTES);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nce_grad_kernel<128>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)nce_grad_lds<128>());
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nce_grad_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)nce_grad_lds<256>());
    }
    const dim3 rows((unsigned)((2 * B + 3) / 4)), sweep((unsigned)(2 * g.rblocks * g.split));
    hipLaunchKernelGGL(nce_norm_kernel, rows, dim3(256), 0, st, p);
    ABN_CHECK_LAUNCH("abnt_nce_loss (norm)");
    hipLaunchKernelGGL(nce_colsum_kernel, dim3((unsigned)g.cblk), dim3(256), 0, st, p);
    ABN_CHECK_LAUNCH("abnt_nce_loss (column sums)");
    hipLaunchKernelGGL(nce_mu_kernel, dim3(1), dim3(256), 0, st, p);
    ABN_CHECK_LAUNCH("abnt_nce_loss (mean)");
    hipLaunchKernelGGL(nce_center_kernel, rows, dim3(256), 0, st, p);
    ABN_CHECK_LAUNCH("abnt_nce_loss (centre)");
    hipLaunchKernelGGL(nce_lse_kernel, sweep, dim3(256), NC_TILE_BYTES, st, p);
    ABN_CHECK_LAUNCH("abnt_nce_loss (lse)");
    hipLaunchKernelGGL(nce_merge_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, p);
    ABN_CHECK_LAUNCH("abnt_nce_loss (merge)");
    hipLaunchKernelGGL(nce_sum_kernel, dim3(1), dim3(256), 0, st, p);
    ABN_CHECK_LAUNCH("abnt_nce_loss (sum)");
    if (!de1) return ABN_OK;
    if (g.dp <= 128) hipLaunchKernelGGL(nce_grad_kernel<128>, sweep, dim3(256), nce_grad_lds<128>(), st, p);
    else hipLaunchKernelGGL(nce_grad_kernel<256>, sweep, dim3(256), nce_grad_lds<256>(), st, p);
    ABN_CHECK_LAUNCH("abnt_nce_loss (gradient)");
    hipLaunchKernelGGL(nce_finish_kernel, rows, dim3(256), 0, st, p);
    ABN_CHECK_LAUNCH("abnt_nce_loss (finish)");
    return ABN_OK;
}
