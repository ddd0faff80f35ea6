// abx.hip -- the kernels of the ABX evaluation (abnet3_amd/abx.py): DTW distances of token pairs without
// paths, and the triplet scores of ABX cells.
//
// 1. abn_dtw_cost_batched, abn_dtw_cost_kl_batched: for pair p, total_cost and path_len of the DTW alignment that
//    abn_dtw_batched computes, bit for bit, with no back-pointers and no traceback: the COST mode of dtw_wave.h's
//    dtw_wave_kernel (the kernel body, its cells and what the mode does are described there), over the angular
//    distance or, _kl, the symmetrised Kullback-Leibler divergence over the tables of abn_kl_tables.  The length is
//    carried forward along the predecessor the recurrence picks (the one abn_dtw_batched's back-pointer encodes), so
//    path_len = 1 + the predecessor's length and the virtual cell (-1, -1) has length 0.  Token 2 is capped at
//    ABN_DTW_COST_MAX_N2 columns; token 1 is unbounded.
//
// 2. kl_tables_kernel (abn_kl_tables): P, L and the per-row BAD flag of a feature table, one wavefront per row.
//
// 3. abx_score_kernel (abn_abx_score): a ROW is one X of one ABX cell with its two lists of distances, d(A, X)
//    over A and d(B, X) over B (contiguous ranges of the distance array).  One wavefront per row: each lane holds
//    one d(B, X), the wavefront walks the d(A, X) and counts 2 per A closer than B and 1 per tie, as integers; the
//    row's sum and its A x B triplet count go to the cell with int64 atomics (order-free: bit-identical results).
#include "dtw_wave.h"

namespace abn {
namespace {

// one wavefront per row: P = max(x, floor), L = float(log(double(P))), bad_row = a non-finite or negative x in the row
__global__ __launch_bounds__(256) void kl_tables_kernel(const float* __restrict__ x, int64_t rows, int D, float floor_,
                                                        float* __restrict__ P, float* __restrict__ L,
                                                        uint8_t* __restrict__ bad_row)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < rows; r += waves) {
        bool bad = false;
        for (int k = lane; k < D; k += 64) {
            const float v = x[r * D + k];
            bad |= !(v >= 0.0f) || v == __builtin_inff();
            const float pv = v > floor_ ? v : floor_;           // (NaN: the floor; the row is BAD anyway)
            P[r * D + k] = pv;
            L[r * D + k] = (float)log((double)pv);
        }
        const bool any = __any(bad);
        if (lane == 0) bad_row[r] = any ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void abx_score_kernel(const double* __restrict__ dist, int64_t ndist,
                                                        const int64_t* __restrict__ a_off, const int32_t* __restrict__ a_len,
                                                        const int64_t* __restrict__ b_off, const int32_t* __restrict__ b_len,
                                                        const int32_t* __restrict__ row_cell, int64_t nrows, int64_t ncells,
                                                        unsigned long long* __restrict__ score2,
                                                        unsigned long long* __restrict__ count, int32_t* __restrict__ refused)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < nrows; r += waves) {
        const int64_t ao = a_off[r], bo = b_off[r];
        const int na = a_len[r], nb = b_len[r], cell = row_cell[r];
        if (na < 0 || nb < 0 || ao < 0 || bo < 0 || ao + na > ndist || bo + nb > ndist || cell < 0 || cell >= ncells) {
            if (lane == 0 && refused) atomicAdd(refused, 1);
            continue;
        }
        unsigned long long s2 = 0;
        for (int b0 = 0; b0 < nb; b0 += 64) {
            if (b0 + lane < nb) {
                const double db = dist[bo + b0 + lane];
                unsigned int part = 0;                           // <= 2 * 4096 per chunk of A: no overflow
                for (int a = 0; a < na; ++a) {
                    const double da = dist[ao + a];
                    part += (da < db ? 2u : 0u) + (da == db ? 1u : 0u);
                    if ((a & 4095) == 4095) { s2 += part; part = 0; }
                }
                s2 += part;
            }
        }
        for (int o = 32; o > 0; o >>= 1) s2 += __shfl_down(s2, o);
        if (lane == 0) {
            atomicAdd(&score2[cell], s2);
            atomicAdd(&count[cell], (unsigned long long)na * (unsigned long long)nb);
        }
    }
}

}  // namespace
}  // namespace abn

using namespace abn;

extern "C" int64_t abn_dtw_cost_max_n2(void) { return ABN_DTW_COST_MAX_N2; }

extern "C" int abn_dtw_cost_batched(const float* feats1, int64_t rows1, const float* feats2, int64_t rows2,
                                    const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                                    int64_t npairs, int64_t D, double* total_cost, int32_t* path_len, void* stream)
{
    return launch_dtw_wave("dtw_cost", feats1, rows1, feats2, rows2, off1, n1, off2, n2, npairs, D,
                           dtw_out<MODE_COST>{total_cost, path_len, 0}, cell_extra<CELL_COSINE>(), stream);
}

extern "C" int abn_dtw_cost_parallel_batched(const float* feats1, int64_t rows1, const float* feats2, int64_t rows2,
                                             const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                                             int64_t npairs, int64_t D, double* total_cost, int32_t* path_len, void* stream)
{
    return launch_dtw_wave("dtw_cost_parallel", feats1, rows1, feats2, rows2, off1, n1, off2, n2, npairs, D,
                           dtw_out<MODE_COST>{total_cost, path_len, 1}, cell_extra<CELL_COSINE>(), stream);
}

extern "C" int abn_kl_tables(const float* x, int64_t rows, int64_t D, float floor, float* P, float* L, uint8_t* bad_row,
                             void* stream)
{
    ABN_REQUIRE(rows >= 0 && D >= 1 && D < (1 << 20), "kl_tables: bad rows/D");
    ABN_REQUIRE(floor > 0.0f && floor < __builtin_inff(), "kl_tables: the floor must be a positive finite number");
    if (rows == 0) return ABN_OK;
    ABN_REQUIRE(x && P && L && bad_row, "kl_tables: null pointer");
    ABN_REQUIRE(rows * D < (1LL << 62), "kl_tables: feature array too large");
    const int64_t blocks = (rows + 3) / 4;
    hipLaunchKernelGGL(kl_tables_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream,
                       x, rows, (int)D, floor, P, L, bad_row);
    ABN_CHECK_LAUNCH("kl_tables");
    return ABN_OK;
}

extern "C" int abn_dtw_cost_kl_batched(const float* P1, const float* L1, int64_t rows1, const float* P2, const float* L2,
                                       int64_t rows2, const int64_t* off1, const int32_t* n1, const int64_t* off2,
                                       const int32_t* n2, int64_t npairs, int64_t D, const uint8_t* bad1,
                                       const uint8_t* bad2, double* total_cost, int32_t* path_len, void* stream)
{
    return launch_dtw_wave("dtw_cost_kl", P1, rows1, P2, rows2, off1, n1, off2, n2, npairs, D,
                           dtw_out<MODE_COST>{total_cost, path_len, 0}, cell_extra<CELL_KL>{L1, L2, bad1, bad2}, stream);
}

extern "C" int abn_abx_score(const double* dist, int64_t ndist, const int64_t* a_off, const int32_t* a_len,
                             const int64_t* b_off, const int32_t* b_len, const int32_t* row_cell, int64_t nrows,
                             int64_t ncells, int64_t* score2, int64_t* count, int32_t* refused, void* stream)
{
    ABN_REQUIRE(ndist >= 0 && nrows >= 0 && ncells >= 0 && ncells < (1LL << 31), "abx_score: bad sizes");
    ABN_REQUIRE(ncells == 0 || (score2 && count), "abx_score: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (refused && hipMemsetAsync(refused, 0, 4, st) != hipSuccess) { set_error("abx_score: memset failed"); return ABN_E_LAUNCH; }
    if (ncells == 0) return ABN_OK;
    if (hipMemsetAsync(score2, 0, (size_t)ncells * 8, st) != hipSuccess ||
        hipMemsetAsync(count, 0, (size_t)ncells * 8, st) != hipSuccess) {
        set_error("abx_score: memset failed");
        return ABN_E_LAUNCH;
    }
    if (nrows == 0) return ABN_OK;
    ABN_REQUIRE(dist && a_off && a_len && b_off && b_len && row_cell, "abx_score: null pointer");
    const int64_t blocks = (nrows + 3) / 4;
    hipLaunchKernelGGL(abx_score_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, dist, ndist,
                       a_off, a_len, b_off, b_len, row_cell, nrows, ncells, (unsigned long long*)score2,
                       (unsigned long long*)count, refused);
    ABN_CHECK_LAUNCH("abx_score");
    return ABN_OK;
}
