// edit_hist.hip -- the (distance, length) histogram of all within-cluster token pairs, without a pair table
// (abnet3_amd/tde.py: cluster_histogram, TermEvaluator.evaluate_full).  The contract is include/abnet3_hip_next.h's
// (prefix abns_); tests/tde_full_np.py restates the counts with explicit loops.
//
// Enumeration.  The host half of the entry reads cl_first (a HOST array) and keeps the clusters of two tokens or more:
// pfx[k] = the pairs of the kept clusters before the k-th, ctok[k] its first token, csize[k] its size -- one record per
// CLUSTER, nothing per pair.  Pair number p lies in the cluster k with pfx[k] <= p < pfx[k + 1], and its rank q = p - pfx[k]
// is unranked row-major over i < j: row i starts at i (2 s - i - 1) / 2, so i = floor((2 s - 1 - sqrt((2 s - 1)^2 - 8 q)) / 2),
// taken in float64 and corrected by integer steps.  Consecutive p share i and walk j: with the tokens of a cluster sorted
// by length (the Python wrapper does that) the 64 lanes of a wavefront meet one token against 64 of neighbouring length.
//
// One wavefront per workgroup, 64 consecutive pairs per step, and per workgroup ONE contiguous range of steps: the cluster
// of a step's first pair is found by one binary search at the start and moves forward by a scan afterwards; a lane whose
// pair lies beyond that cluster's end searches the at most `lane` clusters that follow (every kept cluster has a pair).
//
// The distance is edit_core.h's edit_pair, exactly as edit.hip runs it: the shorter side lane-interleaved in LDS along
// the bits, the same three instantiations picked from M.  The overlap test and the both-empty test come first.
//
// Counting.  Every workgroup counts in LDS (32-bit): the whole [2][M + 1][M + 1] table up to M = 64, the buckets with
// d, L <= 32 beyond (the 256-symbol instantiation's pattern fills 64 KiB; phone transcriptions are short).  Before the
// lanes add, the bucket of the lowest counting lane is peeled off with a ballot and added once with its population --
// the single hot bucket of a cluster whose tokens are all of one type costs one LDS atomic per step, not 64 on one
// address.  The LDS table is flushed with 64-bit global atomics every HIST_FLUSH_STEPS steps (a counter grows by at most
// 64 a step: 2^18 between flushes) and at the end; buckets outside it go straight to global 64-bit atomics.  Integers
// only: the counts depend neither on the grid nor on any order.
#include "common.h"
#include "edit_core.h"
#include "../../include/abnet3_hip_next.h"

#include <stdlib.h>
#include <vector>

using namespace abn;

namespace {

constexpr int LANES = 64;
constexpr int HIST_FLUSH_STEPS = 4096;
constexpr int HIST_HOT = 32;                  // beyond M = 64: the LDS table holds d, L <= HIST_HOT
constexpr int HIST_GRID_BLOCKS = 4096;
constexpr int HIST_GRID_BLOCKS_MAX = 65536;

struct HistArgs {
    const int32_t* sym;
    int64_t rows;
    const int64_t* tok_off;
    const int32_t* tok_n;
    const int32_t* tok_file;
    const double* tok_on;
    const double* tok_end;
    const int32_t* tok_group;                 // null: one group
    const int64_t* pfx;                       // [K + 1]
    const int64_t* ctok;                      // [K]
    const int32_t* csize;                     // [K]
    int64_t K, P, steps, per;
    int32_t M, HB;
    unsigned long long* hist;
    unsigned long long* counts;
};

__global__ __launch_bounds__(256) void edit_hist_check_kernel(const int64_t* __restrict__ tok_off, const int32_t* __restrict__ tok_n,
                                                              int64_t n_tokens, int64_t rows, int32_t M, int32_t* __restrict__ bad)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tokens) return;
    const int64_t o = tok_off[t];
    const int32_t n = tok_n[t];
    if (n < 0 || n > M || o < 0 || o > rows - n) *bad = 1;
}

__device__ __forceinline__ int64_t row_start(int64_t i, int64_t s) { return i * (2 * s - i - 1) / 2; }

__device__ __forceinline__ void hist_flush(uint32_t* lh, int lane, int hb1, int32_t M, unsigned long long* hist)
{
    __syncthreads();
    const int plane = hb1 * hb1;
    for (int k = lane; k < 2 * plane; k += LANES) {
        const uint32_t v = lh[k];
        if (v) {
            lh[k] = 0;
            const int g = k / plane, r = k - g * plane, d = r / hb1, L = r - d * hb1;
            atomicAdd(&hist[((int64_t)g * (M + 1) + d) * (M + 1) + L], (unsigned long long)v);
        }
    }
    __syncthreads();
}

template <typename Word, int W>
__global__ __launch_bounds__(LANES) void edit_hist_kernel(HistArgs a)
{
    constexpr int CAP = (int)sizeof(Word) * 8 * W;
    extern __shared__ __align__(16) unsigned char hist_lds[];
    int32_t* pat = reinterpret_cast<int32_t*>(hist_lds);
    uint32_t* lh = reinterpret_cast<uint32_t*>(hist_lds + (size_t)CAP * LANES * 4);
    const int lane = threadIdx.x;
    const int hb1 = a.HB + 1, M1 = a.M + 1;
    for (int k = lane; k < 2 * hb1 * hb1; k += LANES) lh[k] = 0;
    __syncthreads();

    int64_t step = (int64_t)blockIdx.x * a.per;
    const int64_t step_end = step + a.per < a.steps ? step + a.per : a.steps;
    if (step >= step_end) return;
    int64_t c0 = 0;
    {
        const int64_t p0 = step * LANES;
        int64_t lo = 0, hi = a.K - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (a.pfx[mid] <= p0) lo = mid;
            else hi = mid - 1;
        }
        c0 = lo;
    }
    unsigned long long n_pairs = 0, n_skipped = 0;
    int since = 0;
    for (; step < step_end; ++step) {
        const int64_t p0 = step * LANES;
        while (p0 >= a.pfx[c0 + 1]) ++c0;                   // pfx[K] = P > p0
        const int64_t p = p0 + lane;
        int key = -1;                                       // the pair's LDS bucket
        if (p < a.P) {
            int64_t c = c0;
            if (p >= a.pfx[c0 + 1]) {
                int64_t lo = c0 + 1, hi = c0 + lane < a.K - 1 ? c0 + lane : a.K - 1;
                while (lo < hi) {
                    const int64_t mid = (lo + hi + 1) >> 1;
                    if (a.pfx[mid] <= p) lo = mid;
                    else hi = mid - 1;
                }
                c = lo;
            }
            const int64_t q = p - a.pfx[c], s = a.csize[c];
            const double t = 2.0 * (double)s - 1.0;
            int64_t i = (int64_t)((t - sqrt(fmax(t * t - 8.0 * (double)q, 0.0))) * 0.5);
            i = i < 0 ? 0 : (i > s - 2 ? s - 2 : i);
            while (row_start(i, s) > q) --i;
            while (row_start(i + 1, s) <= q) ++i;
            const int64_t ta = a.ctok[c] + i, tb = ta + 1 + (q - row_start(i, s));
            const bool overlap = a.tok_file[ta] == a.tok_file[tb] &&
                                 fmin(a.tok_end[ta], a.tok_end[tb]) > fmax(a.tok_on[ta], a.tok_on[tb]);
            if (!overlap) {
                ++n_pairs;
                const int32_t l1 = a.tok_n[ta], l2 = a.tok_n[tb];
                if (l1 == 0 && l2 == 0) {
                    ++n_skipped;
                } else {
                    const bool swap = l2 < l1;              // side 2 is the shorter one
                    const int32_t m = swap ? l2 : l1, n = swap ? l1 : l2;
                    const int64_t o1 = a.tok_off[ta], o2 = a.tok_off[tb];
                    int32_t d = n;
                    if (m > 0) {
                        const int32_t* sh = a.sym + (swap ? o2 : o1);
                        const int32_t* tx = a.sym + (swap ? o1 : o2);
                        for (int j = 0; j < m; ++j) pat[j * LANES + lane] = sh[j];
                        d = edit_pair<Word, W, LANES>(pat + lane, m, tx, n);
                    }
                    const int g = a.tok_group ? (a.tok_group[ta] != a.tok_group[tb] ? 1 : 0) : 0;
                    if (d <= a.HB && n <= a.HB) key = (g * hb1 + d) * hb1 + n;
                    else atomicAdd(&a.hist[((int64_t)g * M1 + d) * M1 + n], 1ull);
                }
            }
        }
        const unsigned long long counting = __ballot(key >= 0);
        if (counting) {
            const int first = __builtin_ctzll(counting);
            const int k0 = __shfl(key, first);
            const unsigned long long same = __ballot(key == k0);
            if (lane == first) atomicAdd(&lh[k0], (uint32_t)__popcll(same));
            else if (key >= 0 && key != k0) atomicAdd(&lh[key], 1u);
        }
        if (++since == HIST_FLUSH_STEPS) {
            hist_flush(lh, lane, hb1, a.M, a.hist);
            since = 0;
        }
    }
    hist_flush(lh, lane, hb1, a.M, a.hist);
    for (int off = LANES / 2; off > 0; off >>= 1) {
        n_pairs += __shfl_down(n_pairs, off);
        n_skipped += __shfl_down(n_skipped, off);
    }
    if (lane == 0) {
        if (n_pairs) atomicAdd(&a.counts[0], n_pairs);
        if (n_skipped) atomicAdd(&a.counts[1], n_skipped);
    }
}

// the workspace: [16 bytes: the check kernel's flag][pfx (K + 1) int64][ctok K int64][csize K int32], K <= n_clusters
int64_t hist_ws_bytes(int64_t n_clusters) { return align_up(16 + (n_clusters + 1) * 8 + n_clusters * 8 + n_clusters * 4, 256); }

int hist_lds_bytes(int cap, int hb) { return cap * LANES * 4 + 2 * (hb + 1) * (hb + 1) * 4; }

int hist_grid_blocks()
{
    const char* e = getenv("ABN_EDIT_HIST_BLOCKS");        // read at every call
    if (e && *e) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 1 && v <= HIST_GRID_BLOCKS_MAX) return (int)v;
    }
    return HIST_GRID_BLOCKS;
}

template <typename Word, int W>
void hist_launch(const HistArgs& a, unsigned grid, int lds, hipStream_t st)
{
    if (lds > 64 * 1024) {
        static bool attr_set[16] = {};
        if (first_use_on_device(attr_set))
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(edit_hist_kernel<Word, W>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    }
    hipLaunchKernelGGL((edit_hist_kernel<Word, W>), dim3(grid), dim3(LANES), (size_t)lds, st, a);
}

}  // namespace

extern "C" int64_t abns_edit_hist_max_len(void) { return ABN_EDIT_MAX_SHORT; }

extern "C" int64_t abns_edit_cluster_hist_ws_bytes(int64_t n_tokens, int64_t n_clusters, int64_t n_pairs)
{
    if (n_tokens < 0 || n_clusters < 0 || n_pairs < 0 || n_tokens > INT32_MAX || n_clusters > INT32_MAX) {
        set_error("abns_edit_cluster_hist_ws_bytes: sizes out of range (%lld tokens, %lld clusters, %lld pairs)", (long long)n_tokens,
                  (long long)n_clusters, (long long)n_pairs);
        return -1;
    }
    return hist_ws_bytes(n_clusters);                       // one record per cluster: nothing grows with the pairs
}

extern "C" int abns_edit_cluster_hist(const int32_t* sym, int64_t rows, const int64_t* tok_off, const int32_t* tok_n,
                                      const int32_t* tok_file, const double* tok_on, const double* tok_end, const int32_t* tok_group,
                                      int64_t n_tokens, const int64_t* cl_first, int64_t n_clusters, int64_t M, int64_t* hist,
                                      int64_t* counts, void* ws, int64_t ws_bytes, void* stream)
{
    ABN_REQUIRE(M >= 1 && M <= ABN_EDIT_MAX_SHORT, "edit_cluster_hist: M must lie in 1 .. %d, not %lld", ABN_EDIT_MAX_SHORT, (long long)M);
    ABN_REQUIRE(rows >= 0 && n_tokens >= 0 && n_clusters >= 0 && ws_bytes >= 0, "edit_cluster_hist: negative size");
    ABN_REQUIRE(n_tokens <= INT32_MAX && n_clusters <= INT32_MAX, "edit_cluster_hist: more than 2^31 - 1 tokens or clusters");
    ABN_REQUIRE((sym || rows == 0) && cl_first && hist && counts && ws, "edit_cluster_hist: null pointer");
    ABN_REQUIRE(n_tokens == 0 || (tok_off && tok_n && tok_file && tok_on && tok_end), "edit_cluster_hist: null pointer");
    ABN_REQUIRE(aligned16(ws), "edit_cluster_hist: the workspace must be 16-byte aligned");
    ABN_REQUIRE(cl_first[0] == 0 && cl_first[n_clusters] == n_tokens, "edit_cluster_hist: cl_first must run from 0 to n_tokens");
    int64_t K = 0;
    for (int64_t c = 0; c < n_clusters; ++c) {
        ABN_REQUIRE(cl_first[c + 1] >= cl_first[c], "edit_cluster_hist: cl_first decreases at cluster %lld", (long long)c);
        K += cl_first[c + 1] - cl_first[c] >= 2;
    }
    if (ws_bytes < hist_ws_bytes(n_clusters)) {
        set_error("edit_cluster_hist: the workspace holds %lld bytes, %lld are needed", (long long)ws_bytes, (long long)hist_ws_bytes(n_clusters));
        return ABN_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t table_bytes = (size_t)2 * (size_t)(M + 1) * (size_t)(M + 1) * sizeof(int64_t);

    // the host half: the clusters that hold a pair, as one block of the workspace's layout
    const size_t head = 16 + (size_t)(K + 1) * 8 + (size_t)K * 8 + (size_t)K * 4;
    std::vector<int64_t> block((head + 7) / 8, 0);
    int64_t* pfx = block.data() + 2;
    int64_t* ctok = pfx + K + 1;
    int32_t* csize = reinterpret_cast<int32_t*>(ctok + K);
    int64_t P = 0, k = 0;
    for (int64_t c = 0; c < n_clusters; ++c) {
        const int64_t s = cl_first[c + 1] - cl_first[c];
        if (s < 2) continue;
        pfx[k] = P, ctok[k] = cl_first[c], csize[k] = (int32_t)s;
        P += s * (s - 1) / 2;
        ++k;
    }
    pfx[K] = P;

    unsigned char* base = static_cast<unsigned char*>(ws);
    int32_t bad = 0;
    if (n_tokens > 0) {
        // the tokens are checked on the device before anything is written; the host waits for the flag (and so for the copy
        // of `block`, which lives on this stack)
        if (hipMemcpyAsync(base, block.data(), head, hipMemcpyHostToDevice, st) != hipSuccess) {
            set_error("edit_cluster_hist: the copy of the cluster records failed");
            return ABN_E_LAUNCH;
        }
        hipLaunchKernelGGL(edit_hist_check_kernel, dim3((unsigned)((n_tokens + 255) / 256)), dim3(256), 0, st, tok_off, tok_n, n_tokens, rows,
                           (int32_t)M, reinterpret_cast<int32_t*>(base));
        ABN_CHECK_LAUNCH("edit_cluster_hist (check)");
        if (hipMemcpyAsync(&bad, base, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            set_error("edit_cluster_hist: reading the check's flag failed");
            return ABN_E_LAUNCH;
        }
        ABN_REQUIRE(!bad, "edit_cluster_hist: a token leaves the symbol table or is longer than M = %lld", (long long)M);
    }
    if (hipMemsetAsync(hist, 0, table_bytes, st) != hipSuccess || hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st) != hipSuccess) {
        set_error("edit_cluster_hist: memset failed");
        return ABN_E_LAUNCH;
    }
    if (P == 0) return ABN_OK;

    HistArgs a;
    a.sym = sym, a.rows = rows, a.tok_off = tok_off, a.tok_n = tok_n, a.tok_file = tok_file, a.tok_on = tok_on, a.tok_end = tok_end;
    a.tok_group = tok_group;
    a.pfx = reinterpret_cast<const int64_t*>(base + 16);
    a.ctok = a.pfx + K + 1;
    a.csize = reinterpret_cast<const int32_t*>(a.ctok + K);
    a.K = K, a.P = P, a.steps = (P + LANES - 1) / LANES;
    const int64_t want = hist_grid_blocks();
    a.per = (a.steps + want - 1) / want;
    const unsigned grid = (unsigned)((a.steps + a.per - 1) / a.per);
    a.M = (int32_t)M, a.HB = (int32_t)(M <= 64 ? M : HIST_HOT);
    a.hist = reinterpret_cast<unsigned long long*>(hist), a.counts = reinterpret_cast<unsigned long long*>(counts);
    if (M <= 32) hist_launch<uint32_t, 1>(a, grid, hist_lds_bytes(32, a.HB), st);
    else if (M <= 64) hist_launch<uint64_t, 1>(a, grid, hist_lds_bytes(64, a.HB), st);
    else hist_launch<uint64_t, 4>(a, grid, hist_lds_bytes(256, a.HB), st);
    ABN_CHECK_LAUNCH("edit_cluster_hist");
    return ABN_OK;
}
