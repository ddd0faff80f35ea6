// edit.hip -- batched Levenshtein distance over short int32 sequences (abnet3_amd/tde.py: the normalised edit distance
// of discovered term pairs).  The contract is include/abnet3_hip.h's; tests/tde_np.py restates the distance as the plain
// two-row DP.
//
// One LANE per pair (the sequences are phone transcriptions of 3 .. 60 symbols: nothing to spread over a wavefront), a
// grid-stride loop over the device pair table, workgroups of one wavefront.  The recurrence is edit_core.h's bit-vector
// one; the lane puts the SHORTER side along the bits and walks the longer one.  A lane first copies its short side into
// LDS lane-interleaved (pat[j * 64 + lane]: the 64 lanes of a read hit 64 different banks), because the compare loop
// reads every short-side symbol once per EDIT_TEXT_BLOCK long-side symbols; no lane reads another lane's slots, so there
// is no barrier.  The long side is read straight from global memory, once per symbol and in order: 32 consecutive
// symbols of a lane share a 128-byte line, which stays in L1 / L2 between the lane's visits.
//
// Three instantiations, picked on the host from the caller's max_short: 32-bit words up to 32 symbols (8 KiB of LDS per
// wavefront), one 64-bit word up to 64 (16 KiB), four up to 256 (64 KiB).  The words are template-sized arrays under
// full unrolling: registers, no scratch.
#include "common.h"
#include "edit_core.h"

using namespace abn;

namespace {

constexpr int LANES = ABN_EDIT_BLOCK_PAIRS;
static_assert(LANES == 64, "one wavefront per workgroup: a lane's LDS slots are its own, no barrier");

template <typename Word, int W>
__global__ __launch_bounds__(LANES) void edit_distance_kernel(const int32_t* __restrict__ sym1, int64_t rows1,
                                                              const int32_t* __restrict__ sym2, int64_t rows2,
                                                              const int64_t* __restrict__ off1, const int32_t* __restrict__ n1,
                                                              const int64_t* __restrict__ off2, const int32_t* __restrict__ n2,
                                                              int64_t npairs, int32_t max_short, int32_t* __restrict__ dist)
{
    constexpr int CAP = (int)sizeof(Word) * 8 * W;
    __shared__ int32_t pat[CAP * LANES];
    const int lane = threadIdx.x;
    for (int64_t p = (int64_t)blockIdx.x * LANES + lane; p < npairs; p += (int64_t)gridDim.x * LANES) {
        const int64_t o1 = off1[p], o2 = off2[p];
        const int32_t l1 = n1[p], l2 = n2[p];
        const bool swap = l2 < l1;                          // side 2 is the shorter one
        const int32_t m = swap ? l2 : l1, n = swap ? l1 : l2;
        // (l >= 0 first: rows - l cannot overflow)
        if (l1 < 0 || l2 < 0 || o1 < 0 || o2 < 0 || o1 > rows1 - l1 || o2 > rows2 - l2 || m > max_short || m > CAP) {
            dist[p] = -1;
            continue;
        }
        if (m == 0) {
            dist[p] = n;
            continue;
        }
        const int32_t* s = swap ? sym2 + o2 : sym1 + o1;
        const int32_t* t = swap ? sym1 + o1 : sym2 + o2;
        for (int j = 0; j < m; ++j) pat[j * LANES + lane] = s[j];
        dist[p] = edit_pair<Word, W, LANES>(pat + lane, m, t, n);
    }
}

}  // namespace

extern "C" int64_t abn_edit_max_short(void) { return ABN_EDIT_MAX_SHORT; }

extern "C" int abn_edit_distance_batched(const int32_t* sym1, int64_t rows1, const int32_t* sym2, int64_t rows2,
                                         const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                                         int64_t npairs, int64_t max_short, int32_t* dist, void* stream)
{
    ABN_REQUIRE(max_short >= 1 && max_short <= ABN_EDIT_MAX_SHORT, "edit_distance: max_short must lie in 1 .. %d, not %lld",
                ABN_EDIT_MAX_SHORT, (long long)max_short);
    ABN_REQUIRE(npairs >= 0 && rows1 >= 0 && rows2 >= 0, "edit_distance: negative size");
    if (npairs == 0) return ABN_OK;
    ABN_REQUIRE((sym1 || rows1 == 0) && (sym2 || rows2 == 0) && off1 && n1 && off2 && n2 && dist, "edit_distance: null pointer");
    const int64_t blocks = (npairs + LANES - 1) / LANES;
    const dim3 grid((unsigned)(blocks < ABN_EDIT_GRID_BLOCKS ? blocks : ABN_EDIT_GRID_BLOCKS)), block(LANES);
    hipStream_t st = (hipStream_t)stream;
    const int32_t ms = (int32_t)max_short;
    if (max_short <= 32)
        hipLaunchKernelGGL((edit_distance_kernel<uint32_t, 1>), grid, block, 0, st, sym1, rows1, sym2, rows2, off1, n1, off2, n2, npairs, ms, dist);
    else if (max_short <= 64)
        hipLaunchKernelGGL((edit_distance_kernel<uint64_t, 1>), grid, block, 0, st, sym1, rows1, sym2, rows2, off1, n1, off2, n2, npairs, ms, dist);
    else
        hipLaunchKernelGGL((edit_distance_kernel<uint64_t, 4>), grid, block, 0, st, sym1, rows1, sym2, rows2, off1, n1, off2, n2, npairs, ms, dist);
    ABN_CHECK_LAUNCH("edit_distance");
    return ABN_OK;
}
