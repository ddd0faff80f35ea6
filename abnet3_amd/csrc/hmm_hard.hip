// hmm_hard.hip -- the hard (Viterbi-training) statistics of the full-transition HMM: abnv_hmm_hard_stats
// (include/abnet3_hip_next.h, fifth section; abnet3_amd/hmm.py states the definition, tests/hmm_hard_np.py restates it).
// From decoded unit ids: the transition counts of the minimum-duration chain abnw_hmm_dense_viterbi_dur decodes, the
// per-unit sums [S1 | S2 | N] of the good frames, and the good frames per utterance.  Two memsets and three launches:
//   hh_trans_kernel   one wavefront per utterance, 64 frames at a time: the previous good frame of a lane comes from the
//                     ballot mask of the good lanes, the check of the S previous good ids follows that mask (at most 8
//                     steps), the last 8 good ids travel from chunk to chunk in the low lanes of one register.  The counts
//                     go into an int32 [K + 1][K] table in LDS with LDS atomics and are flushed once per workgroup with
//                     64-bit integer atomics (integers: any order gives the same counts).  It also writes every good frame's
//                     id into the workspace's copy `gid` (cleared to -1 before), so that rows outside every utterance and
//                     ids outside 0 .. K - 1 are nothing to the pass below.
//   hh_emit_kernel    abn_kmeans_accumulate's structure: workgroup (unit tile, frame range), every unit of the tile owned
//                     by one wave, which adds its frames' xc and xc^2 in frame order into LDS accumulators of its own and
//                     writes the range's fp32 partials -- every (range, unit) by exactly one wave, so nothing is cleared.
//   hh_reduce_kernel  the partials in range order in float64, the counts of frames in integers.
// No floating-point atomics, no scratch memory, plain vector stores only.
#include "hmm_dense.h"
#include "vit_wave.h"

namespace abn {

constexpr int HH_B = 128;                   // frames per block of the emission pass's ranges
constexpr int HH_MAX_RANGES = 256;
constexpr int HH_MAX_CT = 16;               // most units of an emission workgroup (4 per wave)
constexpr int HH_CARRY = VIT_DUR_MAX;       // good ids carried from chunk to chunk
constexpr int HH_TRANS_GRID = 256;
static_assert(HH_CARRY == 8, "the carry lives in lanes 0 .. 7 and is indexed with & 7");
constexpr size_t hh_trans_lds(int64_t K) { return sizeof(int) * (size_t)(K + 1) * (size_t)K; }
// 64.5 KiB at K = 128, of the CU's 160 KiB
static_assert(hh_trans_lds(HD_MAX_K) <= 96 * 1024, "the count table fits the LDS");

struct HhTransP {
    const int* ids; const int64_t* off; const int* len;
    int T, K, S, n_utt;
    int* gid;                     // [T]: the good frames' ids, -1 everywhere else
    unsigned long long* counts;   // [K + 1][K]
    int* n_good;                  // [n_utt]
};

__global__ __launch_bounds__(256) void hh_trans_kernel(HhTransP p)
{
    extern __shared__ __attribute__((aligned(16))) int hh_tab[];      // [K + 1][K]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = p.K, S = p.S, cells = (K + 1) * K;
    for (int i = threadIdx.x; i < cells; i += 256) hh_tab[i] = 0;
    __syncthreads();

    const unsigned long long lt_mask = (1ull << lane) - 1ull;         // the lanes below this one
    for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < p.n_utt; u += (int64_t)gridDim.x * 4) {
        const int64_t o = p.off[u];
        const int n = p.len[u];
        if (o < 0 || n < 0 || o + n > p.T || n > UC_MAX_LEN) {        // refused: nothing added
            if (lane == 0) p.n_good[u] = -1;
            continue;
        }
        int carry = -1;                                               // lane i < 8: the (i + 1)-th last good id so far, -1: none
        int good_n = 0;
        for (int base = 0; base < n; base += 64) {
            const bool in = base + lane < n;
            const int id = in ? p.ids[o + base + lane] : -1;
            const bool good = in && id >= 0 && id < K;
            const unsigned long long mask = __ballot(good);
            if (good) p.gid[o + base + lane] = id;
            // the S previous good ids, nearest first: down the mask, then into the carry (every lane takes every shuffle)
            unsigned long long below = mask & lt_mask;
            int ci = 0, prev1 = -1;
            bool all_same = true;
            for (int s = 1; s <= S; ++s) {
                const bool here = below != 0ull;
                const int j = here ? 63 - __builtin_clzll(below) : 0;
                const int a = __shfl(id, j);
                const int b = __shfl(carry, ci & (HH_CARRY - 1));
                const int pid = here ? a : b;
                if (here) below ^= 1ull << j;
                else ++ci;
                if (s == 1) prev1 = pid;
                all_same = all_same && pid == id;
            }
            if (good) {
                if (prev1 < 0) atomicAdd(&hh_tab[K * K + id], 1);                     // the utterance's first good frame
                else if (prev1 != id) atomicAdd(&hh_tab[prev1 * K + id], 1);          // a switch
                else if (all_same) atomicAdd(&hh_tab[id * K + id], 1);                // a stay in the chain's last state
            }
            // the new carry: lane i takes the (i + 1)-th highest good lane of this chunk, then the old carry
            const int cnt = __popcll(mask);
            unsigned long long m = mask;
            int src = 0;
#pragma unroll
            for (int t = 0; t < HH_CARRY; ++t) {
                if (m) {
                    const int j = 63 - __builtin_clzll(m);
                    if (lane == t) src = j;
                    m ^= 1ull << j;
                }
            }
            const int fresh = __shfl(id, src);
            const int old = __shfl(carry, (lane - cnt) & (HH_CARRY - 1));
            carry = lane < cnt ? fresh : old;                          // (lanes 8 .. 63 are never read)
            good_n += cnt;
        }
        if (lane == 0) p.n_good[u] = good_n;
    }

    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += 256) {
        const int c = hh_tab[i];
        if (c) atomicAdd(&p.counts[i], (unsigned long long)c);         // integer: any order gives the same count
    }
}

// ---- the emission part ----------------------------------------------------------------------------------------------
struct HhGrid { int ct, tiles, fblocks, n_ranges, blocks_per_range; };

struct HhEmitP {
    const float* x; const float* shift; const int* gid;
    int T, K, D;
    float* S;                   // [n_ranges][K][2 D]
    int* N;                     // [n_ranges][K]
    HhGrid g;
};

// NP: column passes of a lane (columns lane, lane + 64: NP 64 >= D); U: rows whose loads are in flight together.
template <int NP, int U>
__global__ __launch_bounds__(256) void hh_emit_kernel(HhEmitP p)
{
    __shared__ float acc_s[HH_MAX_CT * 2 * GM_MAX_D];
    __shared__ int cnt_s[HH_MAX_CT];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ct = (int)blockIdx.x % p.g.tiles, rg = (int)blockIdx.x / p.g.tiles;
    const int cw = p.g.ct >> 2;                               // units of a wave
    const int lc0 = wave * cw, c0 = ct * p.g.ct + lc0;        // first of them: in the tile, in the table
    const int D = p.D, D2 = 2 * p.D;
    float* const acc = acc_s + lc0 * D2;                      // [cw][S1 | S2]: this wave's alone, so no barrier in the loop
    int* const cnt = cnt_s + lc0;

    for (int u = lane; u < cw * D2; u += 64) acc[u] = 0.0f;
    if (lane < cw) cnt[lane] = 0;
    __syncthreads();

    float sh[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) sh[q] = p.shift[lane + 64 * q < D ? lane + 64 * q : 0];

    const int64_t f0 = (int64_t)rg * p.g.blocks_per_range * HH_B;
    const int64_t fe = f0 + (int64_t)p.g.blocks_per_range * HH_B;
    const int64_t f1 = fe < p.T ? fe : p.T;
    int idn = f0 + lane < f1 ? p.gid[f0 + lane] : -1;
    for (int64_t base = f0; base < f1; base += 64) {
        const int id = idn;
        idn = base + 64 + lane < f1 ? p.gid[base + 64 + lane] : -1;      // the next 64 ids travel behind this block's rows
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
            float xv[U][NP];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const int d = lane + 64 * q < D ? lane + 64 * q : 0;
                    xv[u][q] = p.x[fr[u] * D + d];
                }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!on[u]) continue;
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const int d = lane + 64 * q;
                    if (d < D) {
                        float xc = xv[u][q] - sh[q];
                        float sq = __fmul_rn(xc, xc);         // rounded once, never contracted into the sum
                        if (!__builtin_isfinite(sq)) { xc = 0.0f; sq = 0.0f; }      // abn_hmm_accumulate's rule
                        acc[lc[u] * D2 + d] += xc;
                        acc[lc[u] * D2 + D + d] += sq;
                    }
                }
                if (lane == 0) cnt[lc[u]] += 1;
            }
        }
    }

    // this wave's part of the range's partials: every (range, unit < K) is written by exactly one wave
    __syncthreads();
    for (int u = lane; u < cw * D2; u += 64) {
        const int k = c0 + u / D2;
        if (k < p.K) p.S[((int64_t)rg * p.K + k) * D2 + u % D2] = acc[u];
    }
    if (lane < cw && c0 + lane < p.K) p.N[(int64_t)rg * p.K + c0 + lane] = cnt[lane];
}

// Block k: sums[k] = [S1 | S2 | N], the partials in range order in float64 (the counts in integers).
__global__ __launch_bounds__(256) void hh_reduce_kernel(const float* __restrict__ S, const int* __restrict__ N, int K, int D,
                                                         int n_ranges, double* __restrict__ sums)
{
    const int t = threadIdx.x, k = (int)blockIdx.x, D2 = 2 * D;
    for (int d = t; d < D2; d += 256) {
        double a = 0.0;
        for (int r = 0; r < n_ranges; ++r) a += (double)S[((int64_t)r * K + k) * D2 + d];
        sums[(int64_t)k * (D2 + 1) + d] = a;
    }
    if (t == 0) {
        long long n = 0;
        for (int r = 0; r < n_ranges; ++r) n += N[(int64_t)r * K + k];
        sums[(int64_t)k * (D2 + 1) + D2] = (double)n;
    }
}

static HhGrid hh_grid(int64_t T, int64_t K, int n_ranges)
{
    HhGrid g;
    g.ct = (int)align_up((K + 7) / 8, 4);                     // about eight unit tiles: the ranges are at most 256
    if (g.ct > HH_MAX_CT) g.ct = HH_MAX_CT;
    g.tiles = (int)((K + g.ct - 1) / g.ct);
    g.fblocks = (int)((T + HH_B - 1) / HH_B);
    int r = n_ranges;
    if (r <= 0) r = (2048 + g.tiles - 1) / g.tiles;           // auto: eight workgroups per CU's worth of (tile, range) pairs
    if (r > HH_MAX_RANGES) r = HH_MAX_RANGES;
    if (r > g.fblocks) r = g.fblocks;
    g.blocks_per_range = (g.fblocks + r - 1) / r;
    g.n_ranges = (g.fblocks + g.blocks_per_range - 1) / g.blocks_per_range;
    return g;
}

// Workspace: gid [T] int32, [n_ranges][K][2 D] fp32 partial sums, [n_ranges][K] int32 partial counts.
struct HhWs { int64_t gid_off, s_off, n_off, bytes; };
static HhWs hh_ws(const HhGrid& g, int64_t T, int64_t K, int64_t D)
{
    HhWs w;
    w.gid_off = 0;
    w.s_off = align_up(T * (int64_t)sizeof(int), 16);
    w.n_off = align_up(w.s_off + (int64_t)g.n_ranges * K * 2 * D * (int64_t)sizeof(float), 16);
    w.bytes = align_up(w.n_off + (int64_t)g.n_ranges * K * (int64_t)sizeof(int), 16);
    return w;
}

static int hh_check_sizes(const char* what, int64_t T, int64_t n_utt, int64_t K, int64_t D)
{
    ABN_REQUIRE(T >= 1 && T < (1LL << 31) - HH_B, "%s: T = %lld out of range", what, (long long)T);
    return chain_check_sizes(what, n_utt, K, D, HD_LIMITS);
}

static int hh_check_ranges(const char* what, int n_ranges)
{
    ABN_REQUIRE(n_ranges >= 0 && n_ranges <= HH_MAX_RANGES, "%s: n_ranges = %d, supported 0 (by the grid) .. %d", what, n_ranges,
                HH_MAX_RANGES);
    return ABN_OK;
}

}  // namespace abn

using namespace abn;

extern "C" int64_t abnv_hmm_hard_stats_ws_bytes(int64_t T, int64_t n_utt, int64_t K, int64_t D, int n_ranges)
{
    const char* what = "abnv_hmm_hard_stats_ws_bytes";
    if (hh_check_sizes(what, T, n_utt, K, D) != ABN_OK || hh_check_ranges(what, n_ranges) != ABN_OK) return -1;
    return hh_ws(hh_grid(T, K, n_ranges), T, K, D).bytes;
}

extern "C" int abnv_hmm_hard_stats(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                                   const float* shift, const int32_t* ids, int64_t K, int32_t min_duration, int n_ranges,
                                   int64_t* counts, double* sums, int32_t* n_good, void* ws, int64_t ws_bytes, void* stream)
{
    const char* what = "abnv_hmm_hard_stats";
    int rc = hh_check_sizes(what, T, n_utt, K, D);
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(x && off && len && shift && ids && counts && sums && n_good, "%s: null pointer", what);
    ABN_REQUIRE(min_duration >= 1 && min_duration <= VIT_DUR_MAX, "%s: min_duration = %d, 1 .. %d (abnx_viterbi_dur_max)", what,
                (int)min_duration, VIT_DUR_MAX);
    rc = hh_check_ranges(what, n_ranges);
    if (rc != ABN_OK) return rc;
    const HhGrid g = hh_grid(T, K, n_ranges);
    const HhWs w = hh_ws(g, T, K, D);
    if (!ws || ws_bytes < w.bytes) {
        set_error("%s: workspace of %lld bytes, %lld needed (abnv_hmm_hard_stats_ws_bytes)", what, (long long)ws_bytes,
                  (long long)w.bytes);
        return ABN_E_WORKSPACE;
    }
    ABN_REQUIRE(aligned16(ws), "%s: the workspace must be 16-byte aligned", what);

    static bool attr_set[16] = {};
    if (first_use_on_device(attr_set))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(hh_trans_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)hh_trans_lds(HD_MAX_K));
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* const base = static_cast<char*>(ws);
    int* const gid = reinterpret_cast<int*>(base + w.gid_off);
    if (hipMemsetAsync(counts, 0, (size_t)(K + 1) * (size_t)K * sizeof(int64_t), st) != hipSuccess ||
        hipMemsetAsync(gid, 0xFF, (size_t)T * sizeof(int), st) != hipSuccess) {
        set_error("%s: memset failed", what);
        return ABN_E_LAUNCH;
    }

    HhTransP tp;
    tp.ids = ids; tp.off = off; tp.len = len;
    tp.T = (int)T; tp.K = (int)K; tp.S = (int)min_duration; tp.n_utt = (int)n_utt;
    tp.gid = gid; tp.counts = reinterpret_cast<unsigned long long*>(counts); tp.n_good = n_good;
    const int64_t want = (n_utt + 3) / 4;
    const dim3 tgrid((unsigned)(want < HH_TRANS_GRID ? want : HH_TRANS_GRID));
    hipLaunchKernelGGL(hh_trans_kernel, tgrid, dim3(256), hh_trans_lds(K), st, tp);
    ABN_CHECK_LAUNCH("abnv_hmm_hard_stats (transitions)");

    HhEmitP ep;
    ep.x = x; ep.shift = shift; ep.gid = gid;
    ep.T = (int)T; ep.K = (int)K; ep.D = (int)D;
    ep.S = reinterpret_cast<float*>(base + w.s_off);
    ep.N = reinterpret_cast<int*>(base + w.n_off);
    ep.g = g;
    const dim3 egrid((unsigned)(g.tiles * g.n_ranges));
    if (D <= 64) hipLaunchKernelGGL((hh_emit_kernel<1, 4>), egrid, dim3(256), 0, st, ep);
    else hipLaunchKernelGGL((hh_emit_kernel<2, 4>), egrid, dim3(256), 0, st, ep);
    ABN_CHECK_LAUNCH("abnv_hmm_hard_stats (emissions)");

    hipLaunchKernelGGL(hh_reduce_kernel, dim3((unsigned)K), dim3(256), 0, st, ep.S, ep.N, (int)K, (int)D, g.n_ranges, sums);
    ABN_CHECK_LAUNCH("abnv_hmm_hard_stats (sum)");
    return ABN_OK;
}
