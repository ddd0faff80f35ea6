// samediff.hip -- same-different word discrimination over segment vectors (abnet3_amd/samediff.py states the task):
// the similarity of every token pair i < j, consumed behind the tile that forms it (abn_sd_collect, abn_sd_count).
//
// The n x n similarity matrix S = X X^T is formed exactly as knn.hip forms Q C^T -- 128 x 128 tiles at multiples of
// 128 on the matrix cores in exact fp32 (v_mfma_f32_32x32x2_f32, k ascending, the loaders and register-staged double
// buffering of gemm_f32.h) -- so sim(i, j) is the same bits here, in abn_knn_topk, and in both modes of this kernel.
// Only the tiles on or above the diagonal exist: a workgroup owns one block of 128 rows and a run of column tiles
// (grid: x = run, y = row block; runs that start past the last column tile leave at once).  Behind each tile the
// accumulators go through LDS (the operand buffers are free by then) and wave w walks rows 32 w .. 32 w + 31 with its
// lanes along the columns: what belongs to the row (its type's end, its speaker) is wave-uniform, what belongs to
// the column is loaded once per tile and lane.
//   * collect: a same-type pair's similarity is stored at pos_sim[pos_off[i] + (j - i - 1)], coalesced along j.
//     Types are contiguous, so the row block's types end at cend[its last row]: the first column tile at or past
//     that ends the run.
//   * count: the pair's bucket b = #{r : thr[r] > sim} is found in two levels -- first against thr[n_thr - 1] and
//     thr[0] (the two end buckets, counted in registers and reduced per workgroup to one atomic each), then by a
//     binary search over a table of at most 1024 splitters in LDS (splitter s = the smallest threshold of block s of
//     `step` consecutive thresholds), then by a binary search inside that one block in global memory
//     (ceil(log2(step)) loads; none when n_thr <= 1024).  Inner buckets are one 64-bit integer atomic each -- except
//     the last SD_HOT of them (the buckets between the smallest positives, where the bulk of the negatives lands when
//     the two populations meet and where integer atomics of all workgroups would queue on a few cache lines): those
//     are counted in LDS for the workgroup's whole run and added once at its end.
// Integer counters only: the result is the same whatever the grid.
#include "common.h"
#include "gemm_f32.h"

#include <math.h>

namespace abn {

constexpr int SD_B = 128;                 // row block = column tile (2 x 2 waves of 2 x 2 MFMA blocks)
constexpr int SD_SST = SD_B + 1;          // staging row stride: a wave reads one row, consecutive dwords
constexpr int SD_MAX_D = 4096;
constexpr int64_t SD_MAX_N = ABN_SD_MAX_N;
constexpr int64_t SD_MAX_THR = ABN_SD_MAX_THR;
constexpr int SD_SPLITTERS = 1024;
constexpr int SD_HOT = 752;               // buckets n_thr - SD_HOT .. n_thr - 1 are counted in LDS (what two workgroups per CU leave free)
using SdTile = TileShape<SD_B, true>;
constexpr int SD_TILE_FLOATS = 4 * SdTile::floats;                       // two stages of each operand
static_assert(SD_TILE_FLOATS >= SD_B * SD_SST, "the similarity tile is staged in the operand buffers");
// operand stages | splitters | the rows' type ends | the rows' speakers | three workgroup counters (+ pad) | hot buckets
constexpr size_t SD_LDS_BYTES = sizeof(float) * (SD_TILE_FLOATS + SD_SPLITTERS) + 4 * (2 * SD_B + 4 + SD_HOT);
// Two workgroups per CU, also if a workgroup's LDS is granted in granules of 1280 bytes (160 KiB / 128; an assumption, no
// document at hand states the granule): 81 872 B round up to 81 920 B, and two of those are the CU's 163 840 B exactly.
// There is no slack: one more word here and the assertion fails instead of the occupancy halving unnoticed.
static_assert(2 * ((SD_LDS_BYTES + 1279) / 1280 * 1280) <= 160 * 1024, "two workgroups per CU");

struct SdP {
    const float* X;
    int n, d;
    const int32_t* cbeg; const int32_t* cend; const int32_t* spk;
    int condition;
    const float* thr; int n_thr, step, n_split;
    unsigned long long* hist; unsigned long long* n_bad;
    const int64_t* pos_off; float* pos_sim;
    int tiles, run;
};

template <bool COUNT>
__global__ __launch_bounds__(256) void sd_tile_kernel(SdP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const As = smem;
    float* const Bs = smem + 2 * SdTile::floats;
    float* const stage = smem;
    float* const split = smem + SD_TILE_FLOATS;                                  // [SD_SPLITTERS]
    int32_t* const row_end = reinterpret_cast<int32_t*>(split + SD_SPLITTERS);   // [128]
    int32_t* const row_spk = row_end + SD_B;                                     // [128]
    uint32_t* const wg_cnt = reinterpret_cast<uint32_t*>(row_spk + SD_B);        // lo, hi, bad
    uint32_t* const hot = wg_cnt + 4;                                            // [SD_HOT]
    const int hot0 = max(p.n_thr - SD_HOT, 0);                                   // first bucket counted in LDS

    const int rblk = (int)blockIdx.y;
    const int m0 = rblk * SD_B;
    const int t0 = rblk + (int)blockIdx.x * p.run;
    if (t0 >= p.tiles) return;
    int t1 = min(p.tiles, t0 + p.run);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    const int ke = p.d, nkt = (p.d + BK - 1) / BK;
    constexpr int PT = SdTile::per_thread;

    if (t < SD_B) {
        const int i = min(m0 + t, p.n - 1);
        row_end[t] = p.cend[i];
        if (COUNT) row_spk[t] = p.spk ? p.spk[i] : 0;
    }
    if (COUNT) {
        for (int s = t; s < p.n_split; s += 256)
            split[s] = p.thr[min((int64_t)(s + 1) * p.step, (int64_t)p.n_thr) - 1];
        if (t < 4) wg_cnt[t] = 0;
        for (int s = t; s < SD_HOT; s += 256) hot[s] = 0;
    }
    __syncthreads();
    if (!COUNT) {                                // column tiles at or past the end of the block's last type hold no pair
        const int last_end = row_end[SD_B - 1];
        t1 = min(t1, (last_end + SD_B - 1) / SD_B);
        if (t0 >= t1) return;
    }
    const float thr_max = (COUNT && p.n_thr > 0) ? p.thr[0] : 0.0f;
    const float thr_min = (COUNT && p.n_thr > 0) ? p.thr[p.n_thr - 1] : 0.0f;
    uint32_t c_lo = 0, c_hi = 0, c_bad = 0;

    f32x4 ra[PT], rb[PT];
    uint32_t voa[PT], vob[PT];
    tile_offsets<SD_B, true>(voa, p.d);
    tile_offsets<SD_B, true>(vob, p.d);
    const bool a_in = m0 + SD_B <= p.n;
    const float* const a_org = p.X + (int64_t)m0 * p.d;

    auto issue = [&](int n0, int k0) {
        const bool k_in = k0 + BK <= ke, b_in = n0 + SD_B <= p.n;
        if (a_in && k_in) tile_issue_fast<SD_B, true>(ra, a_org + k0, voa);
        else tile_issue<SD_B, true, true, false>(ra, p.X, p.d, p.n, m0, k0, ke);
        if (b_in && k_in) tile_issue_fast<SD_B, true>(rb, p.X + (int64_t)n0 * p.d + k0, vob);
        else tile_issue<SD_B, true, true, false>(rb, p.X, p.d, p.n, n0, k0, ke);
    };
    auto commit = [&](int n0, int k0, float* as, float* bs) {
        const bool k_in = k0 + BK <= ke, b_in = n0 + SD_B <= p.n;
        if (a_in && k_in) tile_commit<SD_B, true, true>(ra, as, p.n, m0, k0, ke, -1);
        else tile_commit<SD_B, true, false>(ra, as, p.n, m0, k0, ke, -1);
        if (b_in && k_in) tile_commit<SD_B, true, true>(rb, bs, p.n, n0, k0, ke, -1);
        else tile_commit<SD_B, true, false>(rb, bs, p.n, n0, k0, ke, -1);
    };

    issue(t0 * SD_B, 0);
    for (int ct = t0; ct < t1; ++ct) {
        const int n0 = ct * SD_B;
        const bool b_in = n0 + SD_B <= p.n;
        const float* const b_org = p.X + (int64_t)n0 * p.d;
        commit(n0, 0, As, Bs);
        __syncthreads();

        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

        for (int kt = 0; kt < nkt; ++kt) {
            const int cur = kt & 1;
            const bool more = kt + 1 < nkt;
            const int knext = (kt + 1) * BK;
            const float* as = As + cur * SdTile::floats;
            const float* bs = Bs + cur * SdTile::floats;
            // an interior next k-tile's loads are spread behind the first two k-groups' MFMAs (gemm_f32.h)
            const bool fast = more && a_in && b_in && (knext + BK <= ke);
            if (more && !fast) issue(n0, knext);
#pragma unroll
            for (int g = 0; g < BK / 8; ++g) {
                f32x4 fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) fa[i] = frag_read<SD_B, true>(as, wm0 + 32 * i, g, lane);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[j] = frag_read<SD_B, true>(bs, wn0 + 32 * j, g, lane);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
                if (g < 2 && fast) {
#pragma unroll
                    for (int u = g * PT; u < (g + 1) * PT; ++u) {
                        if (u < PT) ra[u] = *reinterpret_cast<const f32x4*>(a_org + knext + voa[u]);
                        else rb[u - PT] = *reinterpret_cast<const f32x4*>(b_org + knext + vob[u - PT]);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (more) commit(n0, knext, As + (cur ^ 1) * SdTile::floats, Bs + (cur ^ 1) * SdTile::floats);
            __syncthreads();
        }

        // the next column tile's first loads fly while this one is consumed
        if (ct + 1 < t1) issue(n0 + SD_B, 0);

        // Accumulator register r of lane l holds row (r&3) + 8 (r>>2) + 4 (l>>5), column l&31 of its 32 x 32 block.
        {
            const int col_l = lane & 31, rsub = 4 * (lane >> 5);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        stage[(wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub) * SD_SST + wn0 + 32 * j + col_l] = acc[i][j][r];
        }
        __syncthreads();

        // wave w: rows 32 w .. 32 w + 31; lane l: columns l and l + 64
        {
            const int j0 = n0 + lane, j1 = n0 + lane + 64;
            int sj0 = 0, sj1 = 0;
            if (COUNT && p.spk && p.condition != ABN_SD_ALL) {
                sj0 = p.spk[min(j0, p.n - 1)];
                sj1 = p.spk[min(j1, p.n - 1)];
            }
            const int r_end = min(32 * wave + 32, p.n - m0);
            for (int r = 32 * wave; r < r_end; ++r) {
                const int i = m0 + r;
                const int ce = row_end[r];
                const float* const row = stage + r * SD_SST;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int j = h ? j1 : j0;
                    if (j <= i || j >= p.n) continue;             // the diagonal tile's lower half; the zero fill
                    const float v = row[lane + 64 * h];
                    const bool same = j < ce;
                    if (!COUNT) {
                        if (same) p.pos_sim[p.pos_off[i] + (j - i - 1)] = v;
                        continue;
                    }
                    if (same && p.condition != ABN_SD_ALL) {
                        const bool same_spk = row_spk[r] == (h ? sj1 : sj0);
                        if (same_spk == (p.condition == ABN_SD_SWDP)) continue;      // left out of the pool
                    }
                    if (!(fabsf(v) <= 3.4028234663852886e38f)) { ++c_bad; continue; }   // NaN, +-inf
                    if (p.n_thr == 0 || !(thr_max > v)) { ++c_lo; continue; }          // bucket 0
                    if (thr_min > v) { ++c_hi; continue; }                            // bucket n_thr
                    // the first block whose smallest threshold is not above v: all blocks before it lie above v
                    int lo = 0, hi = p.n_split - 1;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (split[mid] > v) lo = mid + 1; else hi = mid;
                    }
                    // the first threshold of that block that is not above v; the block's last one is not
                    int64_t a = (int64_t)lo * p.step, b = min((int64_t)(lo + 1) * p.step, (int64_t)p.n_thr) - 1;
                    while (a < b) {
                        const int64_t mid = (a + b) >> 1;
                        if (p.thr[mid] > v) a = mid + 1; else b = mid;
                    }
                    if (a >= hot0) atomicAdd(&hot[(int)a - hot0], 1u);
                    else atomicAdd(p.hist + a, 1ULL);
                }
            }
        }
        __syncthreads();
    }

    if (COUNT) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            c_lo += __shfl_xor(c_lo, o, 64);
            c_hi += __shfl_xor(c_hi, o, 64);
            c_bad += __shfl_xor(c_bad, o, 64);
        }
        if (lane == 0) {
            if (c_lo) atomicAdd(&wg_cnt[0], c_lo);
            if (c_hi) atomicAdd(&wg_cnt[1], c_hi);
            if (c_bad) atomicAdd(&wg_cnt[2], c_bad);
        }
        __syncthreads();
        if (t == 0) {
            if (wg_cnt[0]) atomicAdd(p.hist, (unsigned long long)wg_cnt[0]);
            if (wg_cnt[1]) atomicAdd(p.hist + p.n_thr, (unsigned long long)wg_cnt[1]);
            if (wg_cnt[2]) atomicAdd(p.n_bad, (unsigned long long)wg_cnt[2]);
        }
        for (int s = t; s < p.n_thr - hot0; s += 256)
            if (hot[s]) atomicAdd(p.hist + hot0 + s, (unsigned long long)hot[s]);
    }
}

static int sd_check_sizes(int64_t n, int d, const char* what)
{
    ABN_REQUIRE(n >= 1, "%s: n = %lld out of range", what, (long long)n);
    if (n > SD_MAX_N) {
        set_error("%s: n = %lld, supported 1 .. %lld", what, (long long)n, (long long)SD_MAX_N);
        return ABN_E_UNSUPPORTED;
    }
    if (d < 4 || d > SD_MAX_D || (d & 3)) {
        set_error("%s: d = %d, supported multiples of 4 in 4 .. %d", what, d, SD_MAX_D);
        return ABN_E_UNSUPPORTED;
    }
    return ABN_OK;
}

// Column tiles per workgroup: ABN_SD_TILES, or 8 .. 64 so that about 2048 workgroups hold work (the longer the run, the
// more of the hot buckets' counts a workgroup adds up in LDS before it touches memory).  Shared by the launch and
// abn_sd_grid_runs.
static int sd_run(int tiles)
{
    int run = switches().sd_tiles;
    if (run <= 0) {
        const int64_t auto_run = (int64_t)tiles * (tiles + 1) / 2 / 2048;
        run = (int)(auto_run < 8 ? 8 : auto_run > 64 ? 64 : auto_run);
    }
    return run;
}

template <bool COUNT>
static int sd_launch(SdP& p, const char* what, hipStream_t st)
{
    p.tiles = (p.n + SD_B - 1) / SD_B;
    p.run = sd_run(p.tiles);
    const int runs = (p.tiles + p.run - 1) / p.run;
    static bool attr_set[16] = {};
    if (first_use_on_device(attr_set))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(sd_tile_kernel<COUNT>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)SD_LDS_BYTES);
    hipLaunchKernelGGL(sd_tile_kernel<COUNT>, dim3((unsigned)runs, (unsigned)p.tiles), dim3(256), SD_LDS_BYTES, st, p);
    ABN_CHECK_LAUNCH(what);
    return ABN_OK;
}

}  // namespace abn

using namespace abn;

extern "C" int64_t abn_sd_grid_runs(int64_t n)
{
    if (n < 1 || n > SD_MAX_N) return -1;
    const int tiles = (int)((n + SD_B - 1) / SD_B);
    return (tiles + sd_run(tiles) - 1) / sd_run(tiles);
}

extern "C" int abn_sd_collect(const float* X, int64_t n, int d, const int32_t* cbeg, const int32_t* cend,
                              const int64_t* pos_off, float* pos_sim, void* stream)
{
    const int rc = sd_check_sizes(n, d, "abn_sd_collect");
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(X && cbeg && cend && pos_off && pos_sim, "abn_sd_collect: null pointer");
    ABN_REQUIRE(aligned16(X), "abn_sd_collect: X must be 16-byte aligned");
    if (n < 2) return ABN_OK;
    SdP p = {};
    p.X = X; p.n = (int)n; p.d = d; p.cbeg = cbeg; p.cend = cend;
    p.pos_off = pos_off; p.pos_sim = pos_sim;
    return sd_launch<false>(p, "abn_sd_collect", static_cast<hipStream_t>(stream));
}

extern "C" int abn_sd_count(const float* X, int64_t n, int d, const int32_t* cbeg, const int32_t* cend,
                            const int32_t* spk, int condition, const float* thr, int64_t n_thr, uint64_t* hist,
                            uint64_t* n_bad, void* stream)
{
    const int rc = sd_check_sizes(n, d, "abn_sd_count");
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(n_thr >= 0, "abn_sd_count: n_thr = %lld out of range", (long long)n_thr);
    if (n_thr > SD_MAX_THR) {
        set_error("abn_sd_count: n_thr = %lld, supported 0 .. %lld", (long long)n_thr, (long long)SD_MAX_THR);
        return ABN_E_UNSUPPORTED;
    }
    ABN_REQUIRE(X && cbeg && cend && hist && n_bad && (thr || n_thr == 0), "abn_sd_count: null pointer");
    ABN_REQUIRE(condition == ABN_SD_ALL || condition == ABN_SD_SWDP || condition == ABN_SD_SWSP,
                "abn_sd_count: condition = %d is none of ABN_SD_ALL, ABN_SD_SWDP, ABN_SD_SWSP", condition);
    ABN_REQUIRE(spk || condition == ABN_SD_ALL, "abn_sd_count: the speaker conditions need spk");
    ABN_REQUIRE(aligned16(X), "abn_sd_count: X must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(hist, 0, (size_t)(n_thr + 1) * 8, st) != hipSuccess || hipMemsetAsync(n_bad, 0, 8, st) != hipSuccess) {
        set_error("abn_sd_count: clearing the counters failed: %s", hipGetErrorString(hipGetLastError()));
        return ABN_E_LAUNCH;
    }
    if (n < 2) return ABN_OK;
    SdP p = {};
    p.X = X; p.n = (int)n; p.d = d; p.cbeg = cbeg; p.cend = cend; p.spk = spk; p.condition = condition;
    p.thr = thr; p.n_thr = (int)n_thr;
    p.step = (int)((n_thr + SD_SPLITTERS - 1) / SD_SPLITTERS);
    if (p.step < 1) p.step = 1;
    p.n_split = (int)((n_thr + p.step - 1) / p.step);
    p.hist = reinterpret_cast<unsigned long long*>(hist);
    p.n_bad = reinterpret_cast<unsigned long long*>(n_bad);
    return sd_launch<true>(p, "abn_sd_count", st);
}
