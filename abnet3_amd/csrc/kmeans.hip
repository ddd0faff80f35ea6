// kmeans.hip -- k-means vector quantisation: hard assignment and a deterministic update (abn_kmeans_assign,
// abn_kmeans_accumulate, abn_kmeans_update), and the penalised segmentation of the ids (abn_kmeans_viterbi, at the end
// of the file; its host side is utt_chain.h's).  abnet3_amd/kmeans.py states the definitions; DESIGN.md
// sections 3.4d and 3.4e the shapes.
//
// The score of frame t under centroid k is one row of a GEMM of depth D + 1,
//   s[t][k] = sum_ka X~[t][ka] W~[k][ka],   X~ = [xc | 1],  W~ = [m | b],  xc = x - shift (fp32),  b = -|m|^2 / 2,
// so argmax_k s = argmin_k |xc - m[k]|^2.  It is formed on the matrix cores in exact fp32 (v_mfma_f32_32x32x2_f32, ka
// ascending; the 128 x 32 operand tiles, the fragment reads and the register-staged double buffering of gemm_f32.h, as
// gmm.hip's likelihood pass uses them).  Neither augmented operand exists in memory, and no T x K array either:
//   * km_assign_kernel: a workgroup owns 128 frames and sweeps the centroid tiles with a running (best score, best
//     index) per frame (two threads per frame, 64 centroids of the tile each, ascending k, strict >: equal scores go
//     to the lowest k), writes ids[t] (-1 for a BAD frame) and adds its count of changed ids to an integer counter;
//   * km_accum_kernel: the responsibilities are one-hot, so the statistics are D additions per frame, not a GEMM.  A
//     workgroup owns a tile of centroids and a range of frames; each of its four waves owns a quarter of the tile, scans
//     the range's ids 64 at a time and, for the frames that are its own, IN FRAME ORDER, adds the row (lanes over
//     columns) into its accumulators in LDS and the row's squared distance to its centroid into a float64 per lane.
//     Every row of x is loaded by exactly one wave; the ids are read once per centroid tile;
//   * km_reduce_kernel sums the partials in range order in float64; km_update_kernel applies the update in float64 and
//     emits the next tables.
// No floating-point atomics anywhere: every sum has one fixed order, two calls give the same bits.
#include "common.h"
#include "kmeans_tile.h"
#include "utt_chain.h"
#include "vit_wave.h"
#include "../../include/abnet3_hip_next.h"

#include <limits.h>
#include <math.h>

namespace abn {

constexpr int KM_MAX_RANGES = 1024;
constexpr int KM_ACC_FLOATS = 8192;        // accumulate pass: LDS accumulators of one workgroup (32 KiB)

__global__ __launch_bounds__(256) void km_assign_kernel(KmP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red_s[KM_B];
    __shared__ int red_i[KM_B], red_c[KM_B];

    const int t = threadIdx.x;
    const int m0 = (int)blockIdx.x * KM_B;
    const int row = t & (KM_B - 1), half = t >> 7;       // this thread's frame and its 64 centroids of every tile
    const int fr = m0 + row;

    float bs;
    int bi;
    km_sweep_argmax(KmFrameRows{p, m0}, p, smem, red_s, red_i, bs, bi);
    int diff = 0;
    if (!half) {
        if (fr < p.T) {
            bool bad = false;
            for (int d = 0; d < p.D; ++d) {
                const float xc = p.x[(int64_t)fr * p.D + d] - p.shift[d];
                bad |= !__builtin_isfinite(xc * xc);
            }
            const int id = bad ? -1 : bi;
            if (p.prev) diff = p.prev[fr] != id;                   // (prev may be ids itself: read before the write)
            p.ids[fr] = id;
            if (p.best) p.best[fr] = bad ? NAN : bs;
        }
        red_c[row] = diff;
    }
    if (!p.prev || !p.changed) return;
    __syncthreads();
    if (t == 0) {
        int n = 0;
        for (int i = 0; i < KM_B; ++i) n += red_c[i];
        if (n) atomicAdd(p.changed, n);                            // integer: any order gives the same count
    }
}

// ---- accumulate ----------------------------------------------------------------------------------------------------
struct KmGrid { int ct, tiles, fblocks, n_ranges, blocks_per_range; };

struct KmAccP {
    const float* x; const float* shift; const float* m; const int* ids;
    int T, K, D;
    float* S;                   // [n_ranges][K][D]
    int* N;                     // [n_ranges][K]
    double* E;                  // [n_ranges][tiles][4]
    KmGrid g;
};

// NP: column passes of a lane (columns lane, lane + 64, ...: NP 64 >= D); U: rows whose loads are in flight together.
template <int NP, int U>
__global__ __launch_bounds__(256) void km_accum_kernel(KmAccP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int cnt_s[KM_B];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ct = (int)blockIdx.x % p.g.tiles, rg = (int)blockIdx.x / p.g.tiles;
    const int cw = p.g.ct >> 2;                               // centroids of a wave
    const int lc0 = wave * cw, c0 = ct * p.g.ct + lc0;        // first of them: in the tile, in the table
    const int D = p.D;
    float* const acc = smem + lc0 * D;                        // [cw][D]: this wave's alone, so no barrier in the loop
    int* const cnt = cnt_s + lc0;

    for (int u = lane; u < cw * D; u += 64) acc[u] = 0.0f;
    if (lane < cw) cnt[lane] = 0;
    __syncthreads();

    float sh[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) sh[q] = p.shift[lane + 64 * q < D ? lane + 64 * q : 0];

    const int64_t f0 = (int64_t)rg * p.g.blocks_per_range * KM_B;
    const int64_t fe = f0 + (int64_t)p.g.blocks_per_range * KM_B;
    const int64_t f1 = fe < p.T ? fe : p.T;
    double e = 0.0;
    int idn = f0 + lane < f1 ? p.ids[f0 + lane] : -1;
    for (int64_t base = f0; base < f1; base += 64) {
        const int id = idn;
        idn = base + 64 + lane < f1 ? p.ids[base + 64 + lane] : -1;      // the next 64 ids travel behind this block's rows
        const bool mine = (unsigned)(id - c0) < (unsigned)cw && id < p.K;
        unsigned long long mask = __ballot(mine);
        while (mask) {                                        // set bits = this wave's frames of the block, ascending
            int lc[U];
            int64_t fr[U];
            bool on[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                on[u] = mask != 0;
                const int j = on[u] ? __builtin_ctzll(mask) : 0;
                if (on[u]) mask &= mask - 1;
                const int k = __shfl(id, j);                  // (j is wave-uniform)
                lc[u] = on[u] ? k - c0 : 0;
                fr[u] = on[u] ? base + j : f0;
            }
            float xv[U][NP], mv[U][NP];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const int d = lane + 64 * q < D ? lane + 64 * q : 0;
                    xv[u][q] = p.x[fr[u] * D + d];
                    mv[u][q] = p.m[(int64_t)(c0 + lc[u]) * D + d];
                }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!on[u]) continue;
                float qs = 0.0f;
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const int d = lane + 64 * q;
                    if (d < D) {
                        const float xc = xv[u][q] - sh[q];
                        acc[lc[u] * D + d] += xc;
                        const float df = xc - mv[u][q];
                        qs += df * df;
                    }
                }
                e += (double)qs;
                if (lane == 0) cnt[lc[u]] += 1;
            }
        }
    }

    // this wave's part of the range's partials: every (range, centroid < K) is written by exactly one wave
    __syncthreads();
    for (int u = lane; u < cw * D; u += 64) {
        const int k = c0 + u / D;
        if (k < p.K) p.S[((int64_t)rg * p.K + k) * D + u % D] = acc[u];
    }
    if (lane < cw && c0 + lane < p.K) p.N[(int64_t)rg * p.K + c0 + lane] = cnt[lane];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);   // a fixed tree
    if (lane == 0) p.E[((int64_t)rg * p.g.tiles + ct) * 4 + wave] = e;
}

// 256 doubles of LDS summed in a fixed tree; the result is returned to every thread.
__device__ __forceinline__ double km_block_sum(double v, double* sh)
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

// Block k < K: sums[k] = [S[k][0 .. D) | N[k]], the partials in range order in float64 (the counts in integers).
// Block K: the inertia partials in index order, the BAD frames (id < 0) and the empty centroids -> stats.
__global__ __launch_bounds__(256) void km_reduce_kernel(const float* __restrict__ S, const int* __restrict__ N,
                                                         const double* __restrict__ E, const int* __restrict__ ids, int T,
                                                         int K, int D, int n_ranges, int n_e, double* __restrict__ sums,
                                                         double* __restrict__ stats)
{
    __shared__ double sh[256];
    const int t = threadIdx.x, k = (int)blockIdx.x;
    if (k < K) {
        for (int d = t; d < D; d += 256) {
            double a = 0.0;
            for (int r = 0; r < n_ranges; ++r) a += (double)S[((int64_t)r * K + k) * D + d];
            sums[(int64_t)k * (D + 1) + d] = a;
        }
        if (t == 0) {
            long long n = 0;
            for (int r = 0; r < n_ranges; ++r) n += N[(int64_t)r * K + k];
            sums[(int64_t)k * (D + 1) + D] = (double)n;
        }
        return;
    }
    double in = 0.0, bad = 0.0, empty = 0.0;
    if (t == 0)
        for (int i = 0; i < n_e; ++i) in += E[i];
    for (int i = t; i < T; i += 256) bad += ids[i] < 0 ? 1.0 : 0.0;
    for (int j = t; j < K; j += 256) {
        long long n = 0;
        for (int r = 0; r < n_ranges; ++r) n += N[(int64_t)r * K + j];
        empty += n == 0 ? 1.0 : 0.0;
    }
    bad = km_block_sum(bad, sh);
    empty = km_block_sum(empty, sh);
    if (t == 0) { stats[0] = in; stats[1] = bad; stats[2] = empty; stats[3] = (double)T - bad; }
}

// One workgroup per centroid: mu = S / N in float64 (an empty centroid keeps its mu), the spherical variant
// renormalises mu to unit length; then m = fp32(mu) and b = fp32(-|m|^2 / 2) over the ROUNDED m (0 when spherical).
__global__ __launch_bounds__(256) void km_update_kernel(const double* __restrict__ sums, int D, int cosine,
                                                         double* __restrict__ mu, float* __restrict__ m, float* __restrict__ b)
{
    __shared__ double sh[256];
    const int t = threadIdx.x, k = (int)blockIdx.x;
    const double n = sums[(int64_t)k * (D + 1) + D];
    double* const mk = mu + (int64_t)k * D;
    if (n > 0.0) {
        double sq = 0.0;
        for (int d = t; d < D; d += 256) {
            const double v = sums[(int64_t)k * (D + 1) + d] / n;
            sq += v * v;
            if (!cosine) mk[d] = v;
        }
        if (cosine) {
            const double nrm = sqrt(km_block_sum(sq, sh));
            if (nrm > 0.0)                                    // (a mean of zero length has no direction: mu stays)
                for (int d = t; d < D; d += 256) mk[d] = sums[(int64_t)k * (D + 1) + d] / n / nrm;
        }
    }
    double hs = 0.0;
    for (int d = t; d < D; d += 256) {
        const float r = (float)mk[d];
        m[(int64_t)k * D + d] = r;
        hs += (double)r * (double)r;
    }
    hs = km_block_sum(hs, sh);
    if (t == 0) b[k] = cosine ? 0.0f : (float)(-0.5 * hs);
}

static KmGrid km_grid(int64_t T, int64_t K, int64_t D, int n_ranges)
{
    KmGrid g;
    g.ct = KM_B;                                              // centroids per workgroup: what fits the LDS accumulators
    while (g.ct > 16 && g.ct * D > KM_ACC_FLOATS) g.ct >>= 1;
    g.tiles = (int)((K + g.ct - 1) / g.ct);
    g.fblocks = (int)((T + KM_B - 1) / KM_B);
    int r = n_ranges;
    if (r <= 0) r = (2048 + g.tiles - 1) / g.tiles;           // auto: eight workgroups per CU's worth of (tile, range) pairs
    if (r > KM_MAX_RANGES) r = KM_MAX_RANGES;
    if (r > g.fblocks) r = g.fblocks;
    g.blocks_per_range = (g.fblocks + r - 1) / r;
    g.n_ranges = (g.fblocks + g.blocks_per_range - 1) / g.blocks_per_range;
    return g;
}

static int km_check_sizes(int64_t T, int64_t K, int64_t D, int n_ranges, const char* what)
{
    ABN_REQUIRE(T >= 1 && T < (1LL << 31) - KM_B, "%s: T = %lld out of range", what, (long long)T);
    ABN_REQUIRE(K >= 1 && D >= 1, "%s: K = %lld, D = %lld out of range", what, (long long)K, (long long)D);
    ABN_REQUIRE(n_ranges >= 0 && n_ranges <= KM_MAX_RANGES, "%s: n_ranges = %d, supported 0 (by the grid) .. %d", what,
                n_ranges, KM_MAX_RANGES);
    if (D > KM_MAX_D || K > KM_MAX_K) {
        set_error("%s: D = %lld, K = %lld, supported D <= %d (abn_kmeans_max_d), K <= %d (abn_kmeans_max_k)", what,
                  (long long)D, (long long)K, KM_MAX_D, KM_MAX_K);
        return ABN_E_UNSUPPORTED;
    }
    return ABN_OK;
}

// Workspace: [n_ranges][K][D] fp32 sums, [n_ranges][K] int32 counts, [n_ranges][tiles][4] float64 inertia partials.
struct KmWs { int64_t s_off, n_off, e_off, bytes; };
static KmWs km_ws(const KmGrid& g, int64_t K, int64_t D)
{
    KmWs w;
    w.s_off = 0;
    w.n_off = align_up((int64_t)g.n_ranges * K * D * (int64_t)sizeof(float), 16);
    w.e_off = align_up(w.n_off + (int64_t)g.n_ranges * K * (int64_t)sizeof(int), 16);
    w.bytes = w.e_off + (int64_t)g.n_ranges * g.tiles * 4 * (int64_t)sizeof(double);
    return w;
}

// ---- penalised segmentation (abn_kmeans_viterbi) ---------------------------------------------------------------------
// Persistent workgroups, utterance u = blockIdx.x, + gridDim.x, ...  Per block of 128 frames the workgroup sweeps the
// centroid tiles with km_score_tile (the assign pass's bits) into its own slab [128][ks] -- in LDS behind the operand
// tiles where K <= 128 (the one shape whose 128 frames x K floats fit beside them), otherwise in the workspace --, then takes
// one sequential step per frame: centroid k = 256 q + thread, W in registers, the max and its lowest index by a wave
// reduction and one LDS exchange, one ballot word of stay bits per 64 centroids, and the previous good frame's j* as an
// int32 (-1: the first good frame, -2: a BAD frame).  Wave 0 then walks the stay bits backwards 64 frames at a time.
// The slab, the stay bits and prevj are written and read by this workgroup alone, on one CU, with a workgroup barrier
// between: plain stores and plain loads are ordered there (the stale-line hazard is another CU's stores); the
// per-workgroup regions are 256-byte aligned so that no cache line is shared between two workgroups.
constexpr int KM_VIT_LDS_KS = KM_B + 8;    // K <= 128: the slab lives in LDS behind the operand tiles; rows 136 floats apart, so
                                           // that the two half-waves of a deposit (4 rows apart) fall on different banks
constexpr size_t KM_VIT_LDS_BYTES = KM_TILE_BYTES + sizeof(float) * KM_B * KM_VIT_LDS_KS;     // 140 KiB of the CU's 160

struct KmVitP {
    const float* x; const float* shift; const float* m; const float* b;
    const int64_t* off; const int* len;
    int T, K, D, n_utt, tiles_k;
    float pen;                              // penalty / 2, in score units
    int* ids; double* objective; int* n_switch;
    char* ws; int64_t per_wg;               // bytes of a workgroup's region
    int ks, kw, cap;                        // slab row stride (floats), stay words per frame, frames the region holds
};

static_assert(KM_B == UC_B, "utt_chain.h's geometry is this kernel's");
constexpr ChainLimits KM_VIT_LIMITS = {KM_MAX_D, "abn_kmeans_max_d", KM_MAX_K, "abn_kmeans_viterbi_max_k", "abn_kmeans_viterbi_max_len"};
constexpr int KM_VIT_TAIL = 8;             // bytes behind a region's prevj (part of what abn_kmeans_viterbi_ws_bytes has always returned)

// The (score, index) key, its wave reduction and the traceback: vit_wave.h (shared with hmm.hip's abn_hmm_viterbi).
template <int NQ, bool LDSS>
__global__ __launch_bounds__(256) void km_viterbi_kernel(KmVitP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const As = smem;
    float* const Bs = smem + 2 * KmTile::floats;
    __shared__ int bad_s[KM_B];
    __shared__ unsigned long long red_k[2][4];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    char* const base = p.ws + (int64_t)blockIdx.x * p.per_wg;
    float* const slab = LDSS ? smem + 4 * KmTile::floats : reinterpret_cast<float*>(base);
    const int ks = LDSS ? KM_VIT_LDS_KS : p.ks;
    unsigned long long* const stay = reinterpret_cast<unsigned long long*>(base + (int64_t)sizeof(float) * KM_B * p.ks);
    int* const prevj = reinterpret_cast<int*>(stay + (int64_t)p.cap * p.kw);
    const float pen = p.pen;

    KmP kp;
    kp.x = p.x; kp.shift = p.shift; kp.m = p.m; kp.b = p.b;
    kp.T = p.T; kp.K = p.K; kp.D = p.D;
    kp.ids = nullptr; kp.prev = nullptr; kp.best = nullptr; kp.changed = nullptr;
    kp.tiles_k = p.tiles_k;

    for (int u = (int)blockIdx.x; u < p.n_utt; u += (int)gridDim.x) {
        const int64_t o = p.off[u];
        const int L = p.len[u];
        if (o < 0 || L < 0 || o + L > p.T || L > p.cap) {            // (uniform) nothing of this utterance is touched
            if (t == 0) {
                if (p.objective) p.objective[u] = NAN;
                if (p.n_switch) p.n_switch[u] = -1;
            }
            continue;
        }
        float W[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) W[q] = 0.0f;
        bool started = false;
        int jprev = -1, par = 0;
        double obj = 0.0;

        for (int f0 = 0; f0 < L; f0 += KM_B) {
            const int m0 = (int)o + f0;
            const int nf = min(KM_B, L - f0);
            if (t < KM_B) {
                bool bad = false;
                if (t < nf)
                    for (int d = 0; d < p.D; ++d) {
                        const float xc = p.x[(int64_t)(m0 + t) * p.D + d] - p.shift[d];
                        bad |= !__builtin_isfinite(xc * xc);
                    }
                bad_s[t] = bad;
            }
            for (int ct = 0; ct < p.tiles_k; ++ct) {
                const int n0 = ct * KM_B;
                f32x16 acc[2][2];
                km_score_tile(kp, m0, n0, As, Bs, acc);
                const int col_l = lane & 31, rsub = 4 * (lane >> 5);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            slab[(int64_t)(wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub) * ks + n0 + wn0 + 32 * j + col_l] =
                                acc[i][j][r];
            }
            __syncthreads();                                          // the slab and bad_s are this workgroup's own

            float sn[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) sn[q] = 256 * q + t < p.K ? slab[256 * q + t] : 0.0f;
            for (int f = 0; f < nf; ++f) {
                const int g = f0 + f;
                float s[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) s[q] = sn[q];
                if (f + 1 < nf) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) sn[q] = 256 * q + t < p.K ? slab[(int64_t)(f + 1) * ks + 256 * q + t] : 0.0f;
                }
                if (bad_s[f]) {                                       // (uniform) the state passes through
                    if (t == 0) prevj[g] = -2;
                    continue;
                }
                unsigned long long key = 0;                           // (below the key of -inf)
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int k = 256 * q + t;
                    const bool st = started && W[q] > -pen;
                    const unsigned long long word = __ballot(st);
                    if (lane == 0) stay[(int64_t)g * p.kw + 4 * q + wave] = word;
                    float uq = started ? s[q] + (st ? W[q] : -pen) : s[q];
                    if (k >= p.K) uq = -INFINITY;
                    W[q] = uq;
                    const unsigned long long kq = vit_key(uq, k);
                    key = kq > key ? kq : key;
                }
                key = vit_wave_max(key);
                if (lane == 0) red_k[par][wave] = key;
                __syncthreads();
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const unsigned long long o = red_k[par][w];
                    key = o > key ? o : key;
                }
                par ^= 1;                                             // (the other set is not rewritten before the next barrier)
                const float bv = vit_key_score(key);
                int bi = (int)~(unsigned)key;
                if ((unsigned)bi >= (unsigned)p.K) bi = 0;            // no score compared greater than -inf: still an id
#pragma unroll
                for (int q = 0; q < NQ; ++q) W[q] -= bv;
                obj += (double)bv;
                if (t == 0) prevj[g] = jprev;
                jprev = bi;
                started = true;
            }
            __syncthreads();                                          // before the next block's scores replace these
        }

        if (wave == 0) {                                              // traceback: jprev is the last good frame's j*
            const int nsw = vit_traceback(stay, prevj, p.kw, p.ids, o, L, jprev, lane);
            if (lane == 0) {
                if (p.objective) p.objective[u] = obj;
                if (p.n_switch) p.n_switch[u] = nsw;
            }
        }
        __syncthreads();                                              // the traceback's reads before the next utterance's writes
    }
}

struct KmVitKernels {
    template <int NQ, bool LDSS> static constexpr auto kernel() { return km_viterbi_kernel<NQ, LDSS>; }
};

// ---- penalised segmentation with a minimum duration (abnx_kmeans_viterbi_dur) ------------------------------------------
// km_viterbi_kernel's twin for the minimum-duration topology (vit_wave.h: every centroid a left-to-right chain of S
// states over the same score), with the tables lw = 0, ls = 0, lr = -pen: the same persistent workgroups, score slab,
// stay words and prevj, and so the same workspace.  Thread t keeps the chains of its centroids in V[NQ][SC] registers,
// SC the capacity the kernel is instantiated with (the smallest of 1, 2, 4, 8 that holds S).  A frame needs two
// reductions before its one barrier: the keyed max over the exit states (E and the exit j*, which prevj records) and the
// max over all states (N_t).  After the last frame one more keyed max finds the final state, and wave 0 walks back with
// vit_traceback_dur.
struct KmVitDurP { KmVitP v; int S; };

template <int NQ, bool LDSS, int SC>
__global__ __launch_bounds__(256) void km_viterbi_dur_kernel(KmVitDurP pd)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const As = smem;
    float* const Bs = smem + 2 * KmTile::floats;
    __shared__ int bad_s[KM_B];
    __shared__ unsigned long long red_k[2][4];
    __shared__ float red_n[2][4];

    const KmVitP& p = pd.v;
    const int S = pd.S, e0 = SC - S;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    char* const base = p.ws + (int64_t)blockIdx.x * p.per_wg;
    float* const slab = LDSS ? smem + 4 * KmTile::floats : reinterpret_cast<float*>(base);
    const int ks = LDSS ? KM_VIT_LDS_KS : p.ks;
    unsigned long long* const stay = reinterpret_cast<unsigned long long*>(base + (int64_t)sizeof(float) * KM_B * p.ks);
    int* const prevj = reinterpret_cast<int*>(stay + (int64_t)p.cap * p.kw);
    const float lr = -p.pen;
    constexpr int PARK = vit_dur_parked<NQ, SC>(LDSS);
    float* const park = smem + 4 * KmTile::floats;                    // behind the operand tiles (where the LDS slab would be)

    KmP kp;
    kp.x = p.x; kp.shift = p.shift; kp.m = p.m; kp.b = p.b;
    kp.T = p.T; kp.K = p.K; kp.D = p.D;
    kp.ids = nullptr; kp.prev = nullptr; kp.best = nullptr; kp.changed = nullptr;
    kp.tiles_k = p.tiles_k;

    for (int u = (int)blockIdx.x; u < p.n_utt; u += (int)gridDim.x) {
        const int64_t o = p.off[u];
        const int L = p.len[u];
        if (o < 0 || L < 0 || o + L > p.T || L > p.cap) {            // (uniform) nothing of this utterance is touched
            if (t == 0) {
                if (p.objective) p.objective[u] = NAN;
                if (p.n_switch) p.n_switch[u] = -1;
            }
            continue;
        }
        float V[NQ][SC];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int j = 0; j < SC; ++j) V[q][j] = -INFINITY;
        bool started = false;
        float E = 0.0f;
        int jprev = -1, par = 0;
        double obj = 0.0;

        for (int f0 = 0; f0 < L; f0 += KM_B) {
            const int m0 = (int)o + f0;
            const int nf = min(KM_B, L - f0);
            vit_dur_park<PARK>(V, park, t);
            if (t < KM_B) {
                bool bad = false;
                if (t < nf)
                    for (int d = 0; d < p.D; ++d) {
                        const float xc = p.x[(int64_t)(m0 + t) * p.D + d] - p.shift[d];
                        bad |= !__builtin_isfinite(xc * xc);
                    }
                bad_s[t] = bad;
            }
            for (int ct = 0; ct < p.tiles_k; ++ct) {
                const int n0 = ct * KM_B;
                f32x16 acc[2][2];
                km_score_tile(kp, m0, n0, As, Bs, acc);
                const int col_l = lane & 31, rsub = 4 * (lane >> 5);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            slab[(int64_t)(wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub) * ks + n0 + wn0 + 32 * j + col_l] =
                                acc[i][j][r];
            }
            __syncthreads();                                          // the slab and bad_s are this workgroup's own
            vit_dur_unpark<PARK>(V, park, t);

            // tb is t behind an empty asm: the NQ addresses of these loads are then no loop invariants, which the compiler
            // would keep for the whole kernel (it did, and spilled them to scratch).
            int tb = t;
            asm volatile("" : "+v"(tb));
            float sn[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) sn[q] = 256 * q + tb < p.K ? slab[256 * q + tb] : -INFINITY;
            for (int f = 0; f < nf; ++f) {
                const int g = f0 + f;
                float s[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) s[q] = sn[q];
                if (f + 1 < nf) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) sn[q] = 256 * q + t < p.K ? slab[(int64_t)(f + 1) * ks + 256 * q + t] : -INFINITY;
                }
                if (bad_s[f]) {                                       // (uniform) the state passes through
                    if (t == 0) prevj[g] = -2;
                    continue;
                }
                const float ent = started ? E + lr : 0.0f;            // (uniform: the tables are the same for every centroid)
                unsigned long long key = 0;                           // (below the key of -inf)
                float nmax = -INFINITY;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {                        // (k >= K: s = -inf, so every state stays -inf)
                    const int k = 256 * q + t;
                    bool st;
                    const float m = vit_dur_step<SC>(V[q], s[q], ent, 0.0f, e0, &st);
                    const unsigned long long word = __ballot(st);
                    if (lane == 0) stay[(int64_t)g * p.kw + 4 * q + wave] = word;
                    nmax = fmaxf(nmax, m);
                    const unsigned long long kq = vit_key(V[q][SC - 1], k);
                    key = kq > key ? kq : key;
                }
                key = vit_wave_max(key);
                if (SC > 1) nmax = vit_wave_fmax(nmax);
                if (lane == 0) {
                    red_k[par][wave] = key;
                    if (SC > 1) red_n[par][wave] = nmax;
                }
                __syncthreads();
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const unsigned long long ok = red_k[par][w];
                    key = ok > key ? ok : key;
                    if (SC > 1) nmax = fmaxf(nmax, red_n[par][w]);
                }
                par ^= 1;                                             // (the other set is not rewritten before the next barrier)
                const float xv = vit_key_score(key);
                const float nv = SC > 1 ? nmax : xv;                  // (one state per centroid: the exit max is the max)
                int bi = (int)~(unsigned)key;
                if ((unsigned)bi >= (unsigned)p.K) bi = 0;            // no score compared greater than -inf: still an id
#pragma unroll
                for (int q = 0; q < NQ; ++q)
#pragma unroll
                    for (int j = 0; j < SC; ++j) V[q][j] -= nv;
                E = xv - nv;
                obj += (double)nv;
                if (t == 0) prevj[g] = jprev;
                jprev = bi;
                started = true;
            }
            __syncthreads();                                          // before the next block's scores replace these
        }

        int fcode = -1;                                               // the final state: the lowest k, then the largest slot, at 0
#pragma unroll
        for (int q = NQ - 1; q >= 0; --q) fcode = vit_dur_final_code<SC>(V[q], q, fcode);
        unsigned long long fkey = vit_wave_max(vit_dur_final_key<SC>(fcode, t));
        if (lane == 0) red_k[par][wave] = fkey;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned long long ok = red_k[par][w];
            fkey = ok > fkey ? ok : fkey;
        }

        if (wave == 0) {                                              // traceback from the final state
            int cur = -1, forced = 0;
            if (started && fkey) {
                cur = vit_dur_final_k(fkey);
                const int i = vit_dur_final_slot(fkey) - e0;
                forced = i == S - 1 ? 0 : i + 1;
            }
            const int nsw = vit_traceback_dur(stay, prevj, p.kw, p.ids, o, L, S, cur, forced, lane);
            if (lane == 0) {
                if (p.objective) p.objective[u] = obj;
                if (p.n_switch) p.n_switch[u] = nsw;
            }
        }
        __syncthreads();                                              // the traceback's reads before the next utterance's writes
    }
}

template <int SC>
struct KmVitDurKernels {
    template <int NQ, bool LDSS> static constexpr auto kernel() { return km_viterbi_dur_kernel<NQ, LDSS, SC>; }
};

}  // namespace abn

using namespace abn;

extern "C" int64_t abn_kmeans_viterbi_max_len(void) { return UC_MAX_LEN; }
extern "C" int64_t abn_kmeans_viterbi_max_k(void) { return KM_MAX_K; }

extern "C" int64_t abn_kmeans_viterbi_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D)
{
    return chain_ws_bytes("abn_kmeans_viterbi_ws_bytes", n_utt, max_len, K, D, KM_VIT_LIMITS, vit_frame_bytes(K), KM_VIT_TAIL);
}

// Both segmentation entries: the checks in their order -- min_duration (null: the entry has none) behind penalty_score --,
// the caller's workspace split into abn_kmeans_viterbi_ws_bytes' regions, and the launch.  A min_duration of 1 launches
// the <1> instantiation of km_viterbi_dur_kernel, not km_viterbi_kernel: only abn_kmeans_viterbi launches that one.
static int km_vit_run(const char* what, const int32_t* min_duration, const float* x, int64_t T, int64_t D, const int64_t* off,
                      const int32_t* len, int64_t n_utt, const float* shift, const float* m, const float* b, int64_t K,
                      float penalty_score, int32_t* ids, double* objective, int32_t* n_switch, void* ws, int64_t ws_bytes,
                      void* stream)
{
    ABN_REQUIRE(T >= 1 && T < (1LL << 31) - KM_B, "%s: T = %lld out of range", what, (long long)T);
    int rc = chain_check_sizes(what, n_utt, K, D, KM_VIT_LIMITS);
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(x && off && len && shift && m && b && ids, "%s: null pointer", what);
    ABN_REQUIRE(penalty_score >= 0.0f && __builtin_isfinite(penalty_score), "%s: penalty_score = %g, a finite value >= 0 is needed",
                what, (double)penalty_score);
    const int S = min_duration ? *min_duration : 1;
    ABN_REQUIRE(S >= 1 && S <= VIT_DUR_MAX, "%s: min_duration = %d, 1 .. %d (abnx_viterbi_dur_max)", what, S, VIT_DUR_MAX);
    const ChainWs w = chain_ws(n_utt, 0, K, vit_frame_bytes(K), KM_VIT_TAIL);
    ChainRegion a;
    rc = chain_region(what, "abn_kmeans_viterbi_ws_bytes", ws, ws_bytes, w, &a);
    if (rc != ABN_OK) return rc;
    KmVitDurP p;
    p.v.x = x; p.v.shift = shift; p.v.m = m; p.v.b = b; p.v.off = off; p.v.len = len;
    p.v.T = (int)T; p.v.K = (int)K; p.v.D = (int)D; p.v.n_utt = (int)n_utt;
    p.v.tiles_k = (int)((K + KM_B - 1) / KM_B);
    p.v.pen = penalty_score;
    p.v.ids = ids; p.v.objective = objective; p.v.n_switch = n_switch;
    p.v.ws = a.ws; p.v.per_wg = a.per_wg;
    p.v.ks = a.ks; p.v.kw = a.kw; p.v.cap = a.cap;
    p.S = S;
    if (!min_duration) return vit_launch<KmVitKernels>(what, p.v, K, w, KM_TILE_BYTES, KM_VIT_LDS_BYTES, stream);
    return vit_dur_launch<KmVitDurKernels>(what, p, S, K, w, KM_TILE_BYTES + VIT_DUR_PARK_BYTES, KM_VIT_LDS_BYTES, stream);
}

extern "C" int abn_kmeans_viterbi(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                                  const float* shift, const float* m, const float* b, int64_t K, float penalty_score,
                                  int32_t* ids, double* objective, int32_t* n_switch, void* ws, int64_t ws_bytes, void* stream)
{
    return km_vit_run("abn_kmeans_viterbi", nullptr, x, T, D, off, len, n_utt, shift, m, b, K, penalty_score, ids, objective,
                      n_switch, ws, ws_bytes, stream);
}

extern "C" int32_t abnx_viterbi_dur_max(void) { return VIT_DUR_MAX; }

// abn_kmeans_viterbi with a minimum duration (include/abnet3_hip_next.h); the workspace is abn_kmeans_viterbi_ws_bytes'.
extern "C" int abnx_kmeans_viterbi_dur(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len,
                                       int64_t n_utt, const float* shift, const float* m, const float* b, int64_t K,
                                       float penalty_score, int32_t* ids, double* objective, int32_t* n_switch, void* ws,
                                       int64_t ws_bytes, void* stream, int32_t min_duration)
{
    return km_vit_run("abnx_kmeans_viterbi_dur", &min_duration, x, T, D, off, len, n_utt, shift, m, b, K, penalty_score, ids,
                      objective, n_switch, ws, ws_bytes, stream);
}

extern "C" int64_t abn_kmeans_max_d(void) { return KM_MAX_D; }
extern "C" int64_t abn_kmeans_max_k(void) { return KM_MAX_K; }

extern "C" int64_t abn_kmeans_ws_bytes(int64_t T, int64_t K, int64_t D, int n_ranges)
{
    if (km_check_sizes(T, K, D, n_ranges, "abn_kmeans_ws_bytes") != ABN_OK) return -1;
    return km_ws(km_grid(T, K, D, n_ranges), K, D).bytes;
}

extern "C" int abn_kmeans_assign(const float* x, int64_t T, int64_t D, const float* shift, const float* m, const float* b,
                                 int64_t K, const int32_t* prev_ids, int32_t* ids, float* best, int32_t* changed, void* stream)
{
    const int rc = km_check_sizes(T, K, D, 0, "abn_kmeans_assign");
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(x && shift && m && b && ids, "abn_kmeans_assign: null pointer");
    ABN_REQUIRE(!prev_ids || changed, "abn_kmeans_assign: prev_ids without a counter");
    static bool attr_set[16] = {};
    if (first_use_on_device(attr_set))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(km_assign_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)KM_TILE_BYTES);
    KmP p;
    p.x = x; p.shift = shift; p.m = m; p.b = b;
    p.T = (int)T; p.K = (int)K; p.D = (int)D;
    p.ids = ids; p.prev = prev_ids; p.best = best; p.changed = changed;
    p.tiles_k = (int)((K + KM_B - 1) / KM_B);
    hipLaunchKernelGGL(km_assign_kernel, dim3((unsigned)((T + KM_B - 1) / KM_B)), dim3(256), KM_TILE_BYTES,
                       static_cast<hipStream_t>(stream), p);
    ABN_CHECK_LAUNCH("abn_kmeans_assign");
    return ABN_OK;
}

extern "C" int abn_kmeans_accumulate(const float* x, int64_t T, int64_t D, const float* shift, const float* m, int64_t K,
                                     const int32_t* ids, int n_ranges, void* ws, int64_t ws_bytes, void* stream)
{
    const int rc = km_check_sizes(T, K, D, n_ranges, "abn_kmeans_accumulate");
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(x && shift && m && ids, "abn_kmeans_accumulate: null pointer");
    const KmGrid g = km_grid(T, K, D, n_ranges);
    const KmWs w = km_ws(g, K, D);
    if (!ws || ws_bytes < w.bytes) {
        set_error("abn_kmeans_accumulate: workspace of %lld bytes, %lld needed (abn_kmeans_ws_bytes)", (long long)ws_bytes,
                  (long long)w.bytes);
        return ABN_E_WORKSPACE;
    }
    ABN_REQUIRE(aligned16(ws), "abn_kmeans_accumulate: the workspace must be 16-byte aligned");
    KmAccP p;
    p.x = x; p.shift = shift; p.m = m; p.ids = ids;
    p.T = (int)T; p.K = (int)K; p.D = (int)D;
    char* const base = static_cast<char*>(ws);
    p.S = reinterpret_cast<float*>(base + w.s_off);
    p.N = reinterpret_cast<int*>(base + w.n_off);
    p.E = reinterpret_cast<double*>(base + w.e_off);
    p.g = g;
    const dim3 grid((unsigned)(g.tiles * g.n_ranges));
    const size_t lds = sizeof(float) * (size_t)g.ct * (size_t)D;          // <= 32 KiB
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (D <= 64) hipLaunchKernelGGL((km_accum_kernel<1, 4>), grid, dim3(256), lds, st, p);
    else if (D <= 128) hipLaunchKernelGGL((km_accum_kernel<2, 4>), grid, dim3(256), lds, st, p);
    else if (D <= 256) hipLaunchKernelGGL((km_accum_kernel<4, 2>), grid, dim3(256), lds, st, p);
    else hipLaunchKernelGGL((km_accum_kernel<8, 2>), grid, dim3(256), lds, st, p);
    ABN_CHECK_LAUNCH("abn_kmeans_accumulate");
    return ABN_OK;
}

extern "C" int abn_kmeans_update(const void* ws, int64_t ws_bytes, const int32_t* ids, int64_t T, int64_t K, int64_t D,
                                 int n_ranges, int cosine, double* sums, double* mu, float* m, float* b, double* stats,
                                 void* stream)
{
    const int rc = km_check_sizes(T, K, D, n_ranges, "abn_kmeans_update");
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(ids && sums && stats, "abn_kmeans_update: null pointer");
    ABN_REQUIRE((mu && m && b) || (!mu && !m && !b), "abn_kmeans_update: mu, m and b go together (all null: statistics only)");
    const KmGrid g = km_grid(T, K, D, n_ranges);
    const KmWs w = km_ws(g, K, D);
    if (!ws || ws_bytes < w.bytes) {
        set_error("abn_kmeans_update: workspace of %lld bytes, %lld needed (abn_kmeans_ws_bytes)", (long long)ws_bytes,
                  (long long)w.bytes);
        return ABN_E_WORKSPACE;
    }
    const char* const base = static_cast<const char*>(ws);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(km_reduce_kernel, dim3((unsigned)K + 1), dim3(256), 0, st, reinterpret_cast<const float*>(base + w.s_off),
                       reinterpret_cast<const int*>(base + w.n_off), reinterpret_cast<const double*>(base + w.e_off), ids, (int)T,
                       (int)K, (int)D, g.n_ranges, g.n_ranges * g.tiles * 4, sums, stats);
    ABN_CHECK_LAUNCH("abn_kmeans_update (reduce)");
    if (!mu) return ABN_OK;
    hipLaunchKernelGGL(km_update_kernel, dim3((unsigned)K), dim3(256), 0, st, sums, (int)D, cosine ? 1 : 0, mu, m, b);
    ABN_CHECK_LAUNCH("abn_kmeans_update");
    return ABN_OK;
}
