// gmm.hip -- EM for a diagonal-covariance Gaussian mixture and its posteriorgrams (abn_gmm_posteriors,
// abn_gmm_accumulate, abn_gmm_mstep).  abnet3_amd/gmm.py states the definition; DESIGN.md section 3.4c the shape.
//
// The score of frame t under component k is one row of a GEMM of depth 2D + 1,
//   s[t][k] = sum_ka X~[t][ka] W~[k][ka],   X~ = [xc | xc^2 | 1],  W~ = [A | B | c],  xc = x - shift (fp32),
// formed on the matrix cores in exact fp32 (v_mfma_f32_32x32x2_f32, ka ascending; the 128 x 32 operand tiles, the
// fragment reads and the register-staged double buffering of gemm_f32.h).  Neither augmented operand exists in
// memory: the loaders below build them on the way into LDS.  The T x K responsibilities never exist either:
//   * gmm_like_kernel: a workgroup owns 128 frames and sweeps the component tiles with a running max / sum
//     (two threads per frame, 64 components of the tile each), writes lse[t]; with an output pointer it sweeps
//     once more and writes exp(s - lse) -- the transform, the only code that ever writes the matrix;
//   * gmm_accum_kernel: a workgroup owns one tile of 128 components and a range of frame blocks.  Per block it
//     recomputes the score tile, stages g = exp(s - lse) through LDS as the k-major operand of a second GEMM,
//     [N | S1 | S2][k][.] += sum_t g[t][k] X~[t][.]  (gemm_f32.h's wgrad orientation, ones column included),
//     whose accumulators stay in registers for the whole range; one slab per workgroup is written at the end;
//   * gmm_reduce_kernel sums the slabs in index order in float64 (and lse over the frames); gmm_mstep_kernel applies
//     the M-step in float64 and emits the next tables.
// No floating-point atomics anywhere: every sum has one fixed order, two calls give the same bits.
#include "common.h"
#include "gemm_f32.h"
#include "gmm_tile.h"

#include <math.h>

namespace abn {

__global__ __launch_bounds__(256) void gmm_like_kernel(GmmP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const As = smem;
    float* const Bs = smem + 2 * GmTile::floats;
    float* const stage = smem;
    __shared__ float red_m[256], red_s[256], lse_s[GM_B];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    const int m0 = (int)blockIdx.x * GM_B;
    const int row = t & (GM_B - 1), half = t >> 7;       // this thread's frame and its 64 components of every tile
    const int fr = m0 + row;

    float m = -INFINITY, s = 0.0f;
    for (int ct = 0; ct < p.tiles_k; ++ct) {
        const int n0 = ct * GM_B;
        f32x16 acc[2][2];
        gmm_score_tile(p, m0, n0, As, Bs, acc);
        {   // accumulator register r of lane l: row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of its block
            const int col_l = lane & 31, rsub = 4 * (lane >> 5);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        stage[(wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub) * GM_LST + wn0 + 32 * j + col_l] = acc[i][j][r];
        }
        __syncthreads();
        {
            const float* const rp = stage + row * GM_LST + 64 * half;
            const int nv = min(64, p.K - n0 - 64 * half);          // <= 0: nothing of this tile is mine
            float tm = -INFINITY;
            for (int c = 0; c < nv; ++c) tm = fmaxf(tm, rp[c]);
            if (tm > -INFINITY) {
                const float mn = fmaxf(m, tm);
                float a = 0.0f;
                for (int c = 0; c < nv; ++c) a += expf(rp[c] - mn);
                s = s * expf(m - mn) + a;
                m = mn;
            }
        }
        __syncthreads();
    }
    red_m[t] = m;
    red_s[t] = s;
    __syncthreads();
    if (t < GM_B) {
        bool bad = false;
        if (fr < p.T)
            for (int d = 0; d < p.D; ++d) {
                const float xc = p.x[(int64_t)fr * p.D + d] - p.shift[d];
                bad |= !__builtin_isfinite(xc * xc);
            }
        const float m1 = red_m[t], m2 = red_m[t + GM_B], mn = fmaxf(m1, m2);
        float l = -INFINITY;
        if (mn > -INFINITY) l = mn + logf(red_s[t] * expf(m1 - mn) + red_s[t + GM_B] * expf(m2 - mn));
        if (bad) l = NAN;
        lse_s[t] = l;
        if (fr < p.T) p.lse[fr] = l;
    }
    if (!p.post) return;
    __syncthreads();
    for (int ct = 0; ct < p.tiles_k; ++ct) {
        const int n0 = ct * GM_B;
        f32x16 acc[2][2];
        gmm_score_tile(p, m0, n0, As, Bs, acc);
        {
            const int col_l = lane & 31, rsub = 4 * (lane >> 5);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        stage[(wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub) * GM_LST + wn0 + 32 * j + col_l] = acc[i][j][r];
        }
        __syncthreads();
        for (int u = t; u < GM_B * GM_B; u += 256) {            // a wave writes 64 consecutive components of a frame
            const int rl = u >> 7, cl = u & (GM_B - 1);
            if (m0 + rl >= p.T || n0 + cl >= p.K) continue;
            const float l = lse_s[rl];
            p.post[(int64_t)(m0 + rl) * p.K + n0 + cl] = (l == l) ? expf(stage[rl * GM_LST + cl] - l) : 0.0f;
        }
        __syncthreads();
    }
}

template <int BN>
__global__ __launch_bounds__(256) void gmm_accum_kernel(GmmP p)
{
    constexpr int TN = BN / 64, XPT = 32 * BN / 256;
    using XT = TileShape<BN, false>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const As = smem;
    float* const Bs = smem + 2 * GmTile::floats;
    float* const G = smem;                                  // [128 frames][132]: four k-major tiles of 32 frames
    float* const Xk = smem + 4 * GmTile::floats;            // two stages of [32][BN + 4]
    __shared__ float lse_s[GM_B];

    // Workgroups b, b + 8, ... share an XCD: give each XCD a contiguous run of (component tile, range) pairs, the
    // ranges of a component tile next to each other (they read the same 128 rows of the tables).
    const int total = p.tiles_k * p.n_ranges;
    const int w = xcd_tile_index((int)blockIdx.x, total);
    const int ct = w / p.n_ranges, rg = w % p.n_ranges;
    const int n0 = ct * GM_B;
    const int b0 = rg * p.blocks_per_range, b1 = min(p.fblocks, b0 + p.blocks_per_range);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;         // score tile: frames x components
    const int wc0 = (wave >> 1) * 64, wx0 = (wave & 1) * (BN / 2);   // statistics tile: components x columns
    const int col_l = lane & 31, rsub = 4 * (lane >> 5);

    f32x16 st[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[i][j][r] = 0.0f;

    for (int fb = b0; fb < b1; ++fb) {
        const int m0 = fb * GM_B;
        if (t < GM_B) lse_s[t] = (m0 + t < p.T) ? p.lse[m0 + t] : NAN;      // (its readers are barriers behind)
        f32x16 acc[2][2];
        gmm_score_tile(p, m0, n0, As, Bs, acc);
        float rx[XPT];
        gmm_xk_issue<BN>(rx, p, m0);
        // g = exp(s - lse); 0 for a BAD frame (lse is NaN), past the last frame and past the last component
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub, cl = wn0 + 32 * j + col_l;
                    const float l = lse_s[rl];
                    G[rl * GM_GST + cl] = (l == l && n0 + cl < p.K) ? expf(acc[i][j][r] - l) : 0.0f;
                }
        gmm_xk_commit<BN>(rx, Xk, p, m0);
        __syncthreads();
        for (int q = 0; q < GM_B / BK; ++q) {
            const float* const gs = G + q * BK * GM_GST;
            const float* const xs = Xk + (q & 1) * XT::floats;
            const bool more = q + 1 < GM_B / BK;
            if (more) gmm_xk_issue<BN>(rx, p, m0 + (q + 1) * BK);
#pragma unroll
            for (int g = 0; g < BK / 8; ++g) {
                f32x4 fa[2], fx[TN];
#pragma unroll
                for (int i = 0; i < 2; ++i) fa[i] = frag_read<GM_B, false>(gs, wc0 + 32 * i, g, lane);
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
            if (more) gmm_xk_commit<BN>(rx, Xk + ((q + 1) & 1) * XT::floats, p, m0 + (q + 1) * BK);
            __syncthreads();
        }
    }

    // the workgroup's one slab: [128 components][2 D + 1]
    const int nc = 2 * p.D + 1;
    float* const slab = p.slabs + ((int64_t)ct * p.n_ranges + rg) * GM_B * nc;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kl = wc0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub, col = wx0 + 32 * j + col_l;
                if (col < nc) slab[kl * nc + col] = st[i][j][r];
            }
}

// 256 doubles of LDS summed in a fixed tree; the result is returned to every thread.
__device__ __forceinline__ double block_sum_256(double v, double* sh)
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

// Block k < K: column t of component k's statistics = its slabs in range order, in float64.  Block K: the frames'
// log-likelihoods (thread t takes frames t, t + 256, ... in order, then the fixed tree) and the BAD count.
__global__ __launch_bounds__(256) void gmm_reduce_kernel(const float* __restrict__ slabs, const float* __restrict__ lse,
                                                          int T, int K, int D, int n_ranges, double* __restrict__ sums,
                                                          double* __restrict__ stats)
{
    __shared__ double sh[256];
    const int t = threadIdx.x, nc = 2 * D + 1, k = (int)blockIdx.x;
    if (k < K) {
        gmm_sum_slabs(slabs, k, nc, n_ranges, sums);
        return;
    }
    double ll = 0.0, bad = 0.0;
    for (int i = t; i < T; i += 256) {
        const float l = lse[i];
        if (l == l) ll += (double)l;
        else bad += 1.0;
    }
    ll = block_sum_256(ll, sh);
    bad = block_sum_256(bad, sh);
    if (t == 0) { stats[0] = ll; stats[1] = bad; stats[3] = (double)T - bad; }
}

// One workgroup per component.  Every workgroup first repeats the same two sums over all components in the same
// order (the weights' normaliser and the starved count: K <= 4096 doubles), so no grid-wide step is needed.
__global__ __launch_bounds__(256) void gmm_mstep_kernel(const double* __restrict__ sums, int K, int D,
                                                         const double* __restrict__ gv, double var_floor, double min_count,
                                                         double* __restrict__ w, double* __restrict__ mu, double* __restrict__ var,
                                                         float* __restrict__ A, float* __restrict__ B, float* __restrict__ c,
                                                         double* __restrict__ stats)
{
    __shared__ double sh[256];
    const int t = threadIdx.x, nc = 2 * D + 1, k = (int)blockIdx.x;
    const double tg = stats[3];
    double ws = 0.0, starved = 0.0;
    for (int j = t; j < K; j += 256) {
        const double n = sums[(int64_t)j * nc + 2 * D];
        ws += n / tg;
        if (n < min_count) starved += 1.0;
    }
    ws = block_sum_256(ws, sh);
    starved = block_sum_256(starved, sh);
    const double nk = sums[(int64_t)k * nc + 2 * D];
    const bool keep = nk < min_count;                    // a starved component keeps its mean and variance
    double term = 0.0;
    if (t < D) {
        const int64_t o = (int64_t)k * D + t;
        double m = mu[o], v = var[o];
        if (!keep) {
            m = sums[(int64_t)k * nc + t] / nk;
            v = fmax(sums[(int64_t)k * nc + D + t] / nk - m * m, var_floor * gv[t]);
            mu[o] = m;
            var[o] = v;
        }
        A[o] = (float)(m / v);
        B[o] = (float)(-0.5 / v);
        term = log(6.283185307179586476925286766559 * v) + m * m / v;
    }
    term = block_sum_256(term, sh);
    if (t == 0) {
        const double wk = (nk / tg) / ws;
        w[k] = wk;
        c[k] = (float)(log(wk) - 0.5 * term);
        if (k == 0) stats[2] = starved;
    }
}

static int gmm_check_sizes(int64_t T, int64_t K, int64_t D, int n_ranges, const char* what)
{
    ABN_REQUIRE(T >= 1 && T < (1LL << 31) - GM_B, "%s: T = %lld out of range", what, (long long)T);
    ABN_REQUIRE(K >= 1 && D >= 1, "%s: K = %lld, D = %lld out of range", what, (long long)K, (long long)D);
    ABN_REQUIRE(n_ranges >= 0 && n_ranges <= GM_MAX_RANGES, "%s: n_ranges = %d, supported 0 (by the grid) .. %d", what,
                n_ranges, GM_MAX_RANGES);
    if (D > GM_MAX_D || K > GM_MAX_K) {
        set_error("%s: D = %lld, K = %lld, supported D <= %d (abn_gmm_max_d), K <= %d (abn_gmm_max_k)", what, (long long)D,
                  (long long)K, GM_MAX_D, GM_MAX_K);
        return ABN_E_UNSUPPORTED;
    }
    return ABN_OK;
}

static void gmm_fill(GmmP& p, const float* x, int64_t T, int64_t D, const float* shift, const float* A, const float* B,
                     const float* c, int64_t K, const GmmGrid& g)
{
    p.x = x; p.shift = shift; p.A = A; p.B = B; p.c = c;
    p.T = (int)T; p.K = (int)K; p.D = (int)D;
    p.lse = nullptr; p.post = nullptr; p.slabs = nullptr;
    p.tiles_k = g.tiles_k; p.fblocks = g.fblocks; p.n_ranges = g.n_ranges; p.blocks_per_range = g.blocks_per_range;
}

}  // namespace abn

using namespace abn;

extern "C" int64_t abn_gmm_max_d(void) { return GM_MAX_D; }
extern "C" int64_t abn_gmm_max_k(void) { return GM_MAX_K; }

extern "C" int64_t abn_gmm_ws_bytes(int64_t T, int64_t K, int64_t D, int n_ranges)
{
    if (gmm_check_sizes(T, K, D, n_ranges, "abn_gmm_ws_bytes") != ABN_OK) return -1;
    return gmm_slab_bytes(gmm_grid(T, K, n_ranges), D, n_ranges);
}

extern "C" int abn_gmm_posteriors(const float* x, int64_t T, int64_t D, const float* shift, const float* A, const float* B,
                                  const float* c, int64_t K, float* lse, float* post, void* stream)
{
    const int rc = gmm_check_sizes(T, K, D, 0, "abn_gmm_posteriors");
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(x && shift && A && B && c && lse, "abn_gmm_posteriors: null pointer");
    static bool attr_set[16] = {};
    if (first_use_on_device(attr_set))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gmm_like_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)GM_TILE_BYTES);
    const GmmGrid g = gmm_grid(T, K, 0);
    GmmP p;
    gmm_fill(p, x, T, D, shift, A, B, c, K, g);
    p.lse = lse; p.post = post;
    hipLaunchKernelGGL(gmm_like_kernel, dim3((unsigned)g.fblocks), dim3(256), GM_TILE_BYTES, static_cast<hipStream_t>(stream), p);
    ABN_CHECK_LAUNCH("abn_gmm_posteriors");
    return ABN_OK;
}

extern "C" int abn_gmm_accumulate(const float* x, int64_t T, int64_t D, const float* shift, const float* A, const float* B,
                                  const float* c, int64_t K, const float* lse, int n_ranges, void* ws, int64_t ws_bytes,
                                  void* stream)
{
    const int rc = gmm_check_sizes(T, K, D, n_ranges, "abn_gmm_accumulate");
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(x && shift && A && B && c && lse, "abn_gmm_accumulate: null pointer");
    const GmmGrid g = gmm_grid(T, K, n_ranges);
    const int64_t need = gmm_slab_bytes(g, D, n_ranges);
    if (!ws || ws_bytes < need) {
        set_error("abn_gmm_accumulate: workspace of %lld bytes, %lld needed (abn_gmm_ws_bytes)", (long long)ws_bytes,
                  (long long)need);
        return ABN_E_WORKSPACE;
    }
    static bool attr_set[16] = {};
    if (first_use_on_device(attr_set)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gmm_accum_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)gmm_accum_lds<64>());
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gmm_accum_kernel<128>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)gmm_accum_lds<128>());
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gmm_accum_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)gmm_accum_lds<256>());
    }
    GmmP p;
    gmm_fill(p, x, T, D, shift, A, B, c, K, g);
    p.lse = const_cast<float*>(lse);
    p.slabs = static_cast<float*>(ws);
    const dim3 grid((unsigned)(g.tiles_k * g.n_ranges));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nc = 2 * (int)D + 1;
    if (nc <= 64) hipLaunchKernelGGL(gmm_accum_kernel<64>, grid, dim3(256), gmm_accum_lds<64>(), st, p);
    else if (nc <= 128) hipLaunchKernelGGL(gmm_accum_kernel<128>, grid, dim3(256), gmm_accum_lds<128>(), st, p);
    else hipLaunchKernelGGL(gmm_accum_kernel<256>, grid, dim3(256), gmm_accum_lds<256>(), st, p);
    ABN_CHECK_LAUNCH("abn_gmm_accumulate");
    return ABN_OK;
}

extern "C" int abn_gmm_mstep(const void* ws, int64_t ws_bytes, const float* lse, int64_t T, int64_t K, int64_t D, int n_ranges,
                             const double* gv, double var_floor, double min_count, double* sums, double* w, double* mu,
                             double* var, float* A, float* B, float* c, double* stats, void* stream)
{
    const int rc = gmm_check_sizes(T, K, D, n_ranges, "abn_gmm_mstep");
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(lse && gv && sums && w && mu && var && A && B && c && stats, "abn_gmm_mstep: null pointer");
    ABN_REQUIRE(var_floor >= 0.0 && min_count >= 0.0, "abn_gmm_mstep: var_floor = %g, min_count = %g must not be negative",
                var_floor, min_count);
    const GmmGrid g = gmm_grid(T, K, n_ranges);
    const int64_t need = gmm_slab_bytes(g, D, n_ranges);
    if (!ws || ws_bytes < need) {
        set_error("abn_gmm_mstep: workspace of %lld bytes, %lld needed (abn_gmm_ws_bytes)", (long long)ws_bytes, (long long)need);
        return ABN_E_WORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gmm_reduce_kernel, dim3((unsigned)K + 1), dim3(256), 0, st, static_cast<const float*>(ws), lse, (int)T,
                       (int)K, (int)D, g.n_ranges, sums, stats);
    ABN_CHECK_LAUNCH("abn_gmm_mstep (reduce)");
    hipLaunchKernelGGL(gmm_mstep_kernel, dim3((unsigned)K), dim3(256), 0, st, sums, (int)K, (int)D, gv, var_floor, min_count, w,
                       mu, var, A, B, c, stats);
    ABN_CHECK_LAUNCH("abn_gmm_mstep");
    return ABN_OK;
}
