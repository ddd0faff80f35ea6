// tcl.hip -- abn_tcl_pairs: every temporal-coherence pair of a pass in one launch, one lane per draw.
//
// The reference (abnet3/dataloader.py:324-352) draws, per iteration, a file and a frame t of it with Python's
// `random`, and appends (t, t + delta) for every delta of TCL_DISTANCE_SAME (+1) and TCL_DISTANCES_DIFF (-1) to host
// lists.  Here iteration g of a pass is a pure function of (seed, g, epoch): one Philox4x32-10 call gives 128 bits,
// the upper 64 pick the file, the lower 64 the frame, each by a multiply-high map (philox.h) -- no rejection, no
// retry, no float.  The pairs go straight into the index arrays a BatchPlan reads its batches from: global rows of
// the corpus table and the labels, either packed (iteration i at n_deltas * i) or wherever dst[i] says (the mix: the
// drawn pairs sit behind each batch's word pairs).  tests/tcl_np.py restates it bit for bit.
// The kernel is latency-bound on two dependent reads (dst / the file's row and length) from tables that sit in L2:
// a handful of registers, no LDS, full occupancy; 256-thread blocks, and a grid-stride loop so that the iteration
// count is a 64-bit number whatever the grid is.
#include "common.h"
#include "philox.h"

namespace abn {

constexpr uint32_t TCL_STREAM_TAG = 0x54434C31u;        // 'TCL1': the fourth counter word (the sampler's are 0 .. 3)
constexpr int TCL_BLOCK = 256;
constexpr int64_t TCL_MAX_GRID = 1 << 16;

struct TclP {
    const int64_t* row0; const int64_t* len; const int64_t* dst;
    int64_t* idx1; int64_t* idx2; void* labels;
    int64_t n_iter, first_iter, out_len;
    uint64_t n_files;
    uint32_t k0, k1, epoch;
    int32_t n_deltas, n_same, max_diff;
    int32_t deltas[16];
};

template <typename Label>
__global__ __launch_bounds__(TCL_BLOCK) void tcl_pairs_kernel(TclP p)
{
    Label* __restrict__ labels = static_cast<Label*>(p.labels);
    const int64_t stride = (int64_t)gridDim.x * TCL_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * TCL_BLOCK + threadIdx.x; i < p.n_iter; i += stride) {
        const uint64_t g = (uint64_t)(p.first_iter + i);
        const U4 r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), p.epoch, TCL_STREAM_TAG, p.k0, p.k1);
        const uint64_t rf = ((uint64_t)r.y << 32) | r.x, rt = ((uint64_t)r.w << 32) | r.z;
        const int64_t base = p.dst ? p.dst[i] : (int64_t)p.n_deltas * i;
        const uint64_t f = map64(rf, p.n_files);
        const int64_t row0 = p.row0[f], len = p.len[f];
        const int64_t a = row0 + (int64_t)map64(rt, (uint64_t)(len - p.max_diff));
        if (base < 0 || base > p.out_len - p.n_deltas) continue;        // (a dst entry outside the arrays: nothing is written)
        for (int j = 0; j < p.n_deltas; ++j) {
            p.idx1[base + j] = a;
            p.idx2[base + j] = a + p.deltas[j];
            labels[base + j] = j < p.n_same ? (Label)1 : (Label)-1;
        }
    }
}

}  // namespace abn

using namespace abn;

extern "C" int abn_tcl_pairs(const int64_t* file_row0, const int64_t* file_len, const int64_t* file_len_host,
                             int64_t n_files, const int32_t* deltas, int n_deltas, int n_same, int64_t n_iter,
                             int64_t first_iter, uint64_t seed, uint32_t epoch, const int64_t* dst, int64_t* idx1,
                             int64_t* idx2, void* labels, int labels_f64, int64_t out_len, void* stream)
{
    ABN_REQUIRE(n_files >= 1 && n_files < (1LL << 31), "abn_tcl_pairs: n_files = %lld, 1 .. 2^31 - 1", (long long)n_files);
    ABN_REQUIRE(n_deltas >= 1 && n_deltas <= 16, "abn_tcl_pairs: n_deltas = %d, 1 .. 16", n_deltas);
    ABN_REQUIRE(n_same >= 0 && n_same <= n_deltas, "abn_tcl_pairs: n_same = %d of %d deltas", n_same, n_deltas);
    ABN_REQUIRE(file_row0 && file_len && file_len_host && deltas, "abn_tcl_pairs: null file table / deltas");
    ABN_REQUIRE(n_iter >= 0 && first_iter >= 0 && n_iter <= INT64_MAX - first_iter && out_len >= 0 &&
                n_iter <= INT64_MAX / 16,
                "abn_tcl_pairs: n_iter = %lld, first_iter = %lld, out_len = %lld out of range", (long long)n_iter,
                (long long)first_iter, (long long)out_len);
    TclP p;
    p.max_diff = 0;
    for (int j = 0; j < 16; ++j) p.deltas[j] = 0;
    for (int j = 0; j < n_deltas; ++j) {
        ABN_REQUIRE(deltas[j] >= 0 && deltas[j] < (1 << 30), "abn_tcl_pairs: deltas[%d] = %d, not negative", j, deltas[j]);
        p.deltas[j] = deltas[j];
        if (deltas[j] > p.max_diff) p.max_diff = deltas[j];
    }
    for (int64_t f = 0; f < n_files; ++f)
        ABN_REQUIRE(file_len_host[f] > p.max_diff, "abn_tcl_pairs: file %lld has %lld frames, more than the largest delta (%d) needed",
                    (long long)f, (long long)file_len_host[f], p.max_diff);
    if (n_iter == 0) return ABN_OK;
    ABN_REQUIRE(idx1 && idx2 && labels, "abn_tcl_pairs: null output pointer");
    ABN_REQUIRE(dst || (int64_t)n_deltas * n_iter <= out_len, "abn_tcl_pairs: %lld iterations of %d pairs do not fit %lld elements",
                (long long)n_iter, n_deltas, (long long)out_len);
    ABN_REQUIRE(out_len >= n_deltas, "abn_tcl_pairs: out_len = %lld holds no iteration", (long long)out_len);
    p.row0 = file_row0; p.len = file_len; p.dst = dst;
    p.idx1 = idx1; p.idx2 = idx2; p.labels = labels;
    p.n_iter = n_iter; p.first_iter = first_iter; p.out_len = out_len;
    p.n_files = (uint64_t)n_files;
    p.k0 = (uint32_t)seed; p.k1 = (uint32_t)(seed >> 32); p.epoch = epoch;
    p.n_deltas = n_deltas; p.n_same = n_same;
    int64_t grid = (n_iter + TCL_BLOCK - 1) / TCL_BLOCK;
    if (grid > TCL_MAX_GRID) grid = TCL_MAX_GRID;
    if (labels_f64)
        hipLaunchKernelGGL(tcl_pairs_kernel<double>, dim3((unsigned)grid), dim3(TCL_BLOCK), 0, static_cast<hipStream_t>(stream), p);
    else
        hipLaunchKernelGGL(tcl_pairs_kernel<int64_t>, dim3((unsigned)grid), dim3(TCL_BLOCK), 0, static_cast<hipStream_t>(stream), p);
    ABN_CHECK_LAUNCH("abn_tcl_pairs");
    return ABN_OK;
}
