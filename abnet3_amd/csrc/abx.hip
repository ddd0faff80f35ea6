// abx.hip -- the kernels of the ABX evaluation (abnet3_amd/abx.py): DTW distances of token pairs without
// paths, and the triplet scores of ABX cells.
//
// 1. dtw_cost_kernel (abn_dtw_cost_batched): for pair p, total_cost and path_len of the DTW alignment that
//    abn_dtw_batched computes, bit for bit, with no back-pointers and no traceback.  The cell is dist_ref.h's
//    angular distance (one fmaf chain over k, numpy's norm order, the compiler's correctly rounded division,
//    glibc's acosf, / float32(pi); the file is compiled with -ffp-contract=off), the recurrence
//    cost = d + min(diag, up, left) in float64 with the first minimum in the order diag, up, left.  The length is
//    carried forward along the predecessor that recurrence picks (the one abn_dtw_batched's back-pointer encodes),
//    so path_len = 1 + the predecessor's length and the virtual cell (-1, -1) has length 0.
//
//    One wavefront per pair (a grid-stride loop over the device-resident pair table).  Token 1 is cut into BANDS
//    of 64 rows, one row per lane; a band into ROUNDS of 64 anti-diagonals.  A round first computes the cells of
//    its 64 diagonals CELL-PARALLEL -- every lane takes 2 x 2 tiles of the rectangle of rows x columns that holds
//    them (four fmaf chains sharing their loads), so a 15 x 15 pair keeps all 64 lanes busy instead of 15 -- and
//    drops them into a diagonal-major ring in LDS
//    (ring[(i + j) & 63][i]).  Then the lanes sweep the 64 diagonals: lane i holds row i's costs, the row above
//    arrives over a DPP wave shift, the diagonal neighbour is the previous step's upper value.  The band's last row
//    (cost and length per column) is handed to the next band through LDS, which caps token 2 at
//    ABN_DTW_COST_MAX_N2 columns; token 1 is unbounded.  Token-2 norms are computed once per pair (LDS), token-1
//    norms once per band.  Frames are read from L1 / L2: no workspace, one launch.
//
//    The cell is a template parameter.  CELL_KL (abn_dtw_cost_kl_batched) is the symmetrised Kullback-Leibler
//    divergence of two posteriorgram frames over the tables of abn_kl_tables (P = max(x, floor), L = log P):
//    acc = acc + ((P_p[k] - P_q[k]) * (L_p[k] - L_q[k])) in ascending k, every operation rounded to float32 on its
//    own (no fma: -ffp-contract=off), d = 0.5f * acc.  Every term is >= 0, so d >= 0 and d == 0 for identical
//    frames.  Bands, rounds, the ring, the sweep and the boundary row are the cosine cell's; norms and their LDS do
//    not exist, a pair with a BAD row (non-finite or negative input) is dropped before any cell is computed.
//    (The 2 x 2 tiles, the wave shift and the LDS hand-off live in dtw_tiles.h: search.hip's kernel uses them too.)
//
// 2. kl_tables_kernel (abn_kl_tables): P, L and the per-row BAD flag of a feature table, one wavefront per row.
//
// 3. abx_score_kernel (abn_abx_score): a ROW is one X of one ABX cell with its two lists of distances, d(A, X)
//    over A and d(B, X) over B (contiguous ranges of the distance array).  One wavefront per row: each lane holds
//    one d(B, X), the wavefront walks the d(A, X) and counts 2 per A closer than B and 1 per tie, as integers; the
//    row's sum and its A x B triplet count go to the cell with int64 atomics (order-free: bit-identical results).
#include "common.h"
#include "dist_ref.h"
#include "dtw_tiles.h"

namespace abn {
namespace {

constexpr int CB = 64;                          // rows of a band = lanes
constexpr int RD = 64;                          // anti-diagonals of a round (the LDS ring's rows; 32 measured the same)
constexpr int MAXN2 = ABN_DTW_COST_MAX_N2;      // token-2 frames a pair may have (the LDS boundary row)

// what the KL cell reads beside the two P tables (feats1 / feats2 of the kernel); the cosine cell has nothing here
template <bool KL>
struct cell_extra {};
template <>
struct cell_extra<true> {
    const float* L1;
    const float* L2;
    const uint8_t* bad1;
    const uint8_t* bad2;
};
constexpr bool CELL_COSINE = false, CELL_KL = true;

template <bool VEC, bool KL>
__global__ __launch_bounds__(64) void dtw_cost_kernel(const float* __restrict__ feats1, int64_t rows1,
                                                      const float* __restrict__ feats2, int64_t rows2,
                                                      const int64_t* __restrict__ off1, const int32_t* __restrict__ n1,
                                                      const int64_t* __restrict__ off2, const int32_t* __restrict__ n2,
                                                      int64_t npairs, int D, double* __restrict__ total_cost,
                                                      int32_t* __restrict__ path_len, cell_extra<KL> ex)
{
    __shared__ float ring[RD][CB];              // [diagonal % RD][row of the band]
    __shared__ double bnd_c[MAXN2];             // the band's last row: costs ...
    __shared__ int32_t bnd_l[MAXN2];            // ... and path lengths, per column
    __shared__ float ny_s[MAXN2];
    __shared__ float nx_s[CB];
    const int lane = threadIdx.x;
    const double INF = __builtin_inf();

    for (int64_t p = blockIdx.x; p < npairs; p += gridDim.x) {
        const int64_t o1 = off1[p], o2 = off2[p];
        const int N = n1[p], M = n2[p];
        if (N < 0 || M < 0 || M > MAXN2 || o1 < 0 || o2 < 0 || o1 + N > rows1 || o2 + M > rows2) {
            if (lane == 0) { path_len[p] = -1; total_cost[p] = 0.0; }          // refused: nothing is read
            continue;
        }
        if (N == 0 || M == 0) {
            if (lane == 0) { path_len[p] = 0; total_cost[p] = 0.0; }
            continue;
        }
        const float* X = feats1 + o1 * D;
        const float* Y = feats2 + o2 * D;
        bool bad = false;
        const float* LX = nullptr;
        const float* LY = nullptr;
        if constexpr (KL) {                                     // a BAD row in either token: the pair is dropped
            for (int i = lane; i < N; i += CB) bad |= ex.bad1[o1 + i] != 0;
            for (int j = lane; j < M; j += CB) bad |= ex.bad2[o2 + j] != 0;
            if (__any(bad)) {
                if (lane == 0) { path_len[p] = 0; total_cost[p] = 0.0; }
                continue;
            }
            LX = ex.L1 + o1 * D;
            LY = ex.L2 + o2 * D;
        } else {
            for (int j = lane; j < M; j += CB) ny_s[j] = row_norm_numpy(Y + (int64_t)j * D, D);
        }
        double fin_c = 0.0;
        int fin_l = 0;
        for (int i0 = 0; i0 < N; i0 += CB) {
            const int nr = min(CB, N - i0);
            const bool feed = i0 + CB < N;                      // the last row goes to the band below
            if constexpr (!KL) {
                if (lane < nr) nx_s[lane] = row_norm_numpy(X + (int64_t)(i0 + lane) * D, D);
                wave_lds_sync();
            }
            // sweep state of row i0 + lane: p1 = its cost at the previous column, up_prev = the row above one
            // column back (= the diagonal neighbour of the next step); the virtual cell (-1, -1) costs 0
            double p1 = INF, up_prev = (i0 == 0 && lane == 0) ? 0.0 : INF;
            int l1 = 0, lup_prev = 0;
            const int ndiag = nr + M - 1;
            for (int s0 = 0; s0 < ndiag; s0 += RD) {
                // ---- produce: the cells (i, j) of band rows with s0 <= i + j < s0 + RD
                const int jlo = max(0, s0 - (nr - 1)), jhi = min(M, s0 + RD);
                // 2 x 2 tiles of cells, one per lane at a time (an odd last row / column repeats its neighbour: the
                // repeated cell is computed twice and stored twice, the same value)
                const int tr = (nr + 1) >> 1, ntile = tr * ((jhi - jlo + 1) >> 1);
                for (int t = lane; t < ntile; t += CB) {
                    const int tj = t / tr, ia = 2 * (t - tj * tr), ja = jlo + 2 * tj;
                    const int ib = min(ia + 1, nr - 1), jb = min(ja + 1, jhi - 1);
                    float dot[4];
                    const int64_t xa = (int64_t)(i0 + ia) * D, xb = (int64_t)(i0 + ib) * D;
                    const int64_t ya = (int64_t)ja * D, yb = (int64_t)jb * D;
                    if constexpr (KL) kl_tile<VEC>(X + xa, X + xb, LX + xa, LX + xb, Y + ya, Y + yb, LY + ya, LY + yb, D, dot);
                    else dot_tile<VEC>(X + xa, X + xb, Y + ya, Y + yb, D, dot);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int il = c < 2 ? ia : ib, j = (c & 1) ? jb : ja, s = il + j;
                        if (s < s0 || s >= s0 + RD) continue;
                        if constexpr (KL) {
                            ring[s & (RD - 1)][il] = 0.5f * dot[c];
                        } else {
                            const float nx = nx_s[il], ny = ny_s[j];
                            const float d = (norm_is_plain(nx) && norm_is_plain(ny)) ? angular_distance_ref<true>(dot[c], nx, ny)
                                                                                     : angular_distance_ref<false>(dot[c], nx, ny);
                            bad |= !(d >= 0.0f);                // utils.py:59: the pair is dropped
                            ring[s & (RD - 1)][il] = d;
                        }
                    }
                }
                wave_lds_sync();
                // ---- sweep: diagonals s0 .. s0 + RD - 1; lane i is at column s - i
                // (the step's LDS operands are read one step ahead: they do not depend on the chain)
                const int ns = min(RD, ndiag - s0);
                float dnext = ring[s0 & (RD - 1)][lane];
                double tnext = INF;
                int tlnext = 0;
                if (lane == 0 && i0 > 0 && s0 < M) { tnext = bnd_c[s0]; tlnext = bnd_l[s0]; }
                for (int e = 0; e < ns; ++e) {
                    const int s = s0 + e, j = s - lane;
                    const float dist = dnext;
                    double up = shr1_f64(p1);
                    int lup = shr1_i32(l1);
                    if (lane == 0) { up = tnext; lup = tlnext; }
                    dnext = ring[(s + 1) & (RD - 1)][lane];
                    if (lane == 0 && i0 > 0 && s + 1 < M) { tnext = bnd_c[s + 1]; tlnext = bnd_l[s + 1]; }
                    const double dg = up_prev, left = p1;
                    const int ldg = lup_prev;
                    up_prev = up;
                    lup_prev = lup;
                    if (lane < nr && (unsigned)j < (unsigned)M) {
                        const bool take_up = up < dg;               // first minimum in the order diag, up, left
                        const double b1 = take_up ? up : dg;
                        const bool take_left = left < b1;
                        const double best = take_left ? left : b1;
                        const int lbest = take_left ? l1 : (take_up ? lup : ldg);
                        p1 = (double)dist + best;
                        l1 = lbest + 1;
                        if (feed && lane == CB - 1) { bnd_c[j] = p1; bnd_l[j] = l1; }
                    }
                }
                wave_lds_sync();                                // the next round's cells overwrite the ring
            }
            if (i0 + nr == N) {                                 // lane nr - 1 holds cell (N - 1, M - 1)
                fin_c = __shfl(p1, nr - 1);
                fin_l = __shfl(l1, nr - 1);
            }
        }
        const bool dropped = __any(bad);
        if (lane == 0) {
            total_cost[p] = dropped ? 0.0 : fin_c;
            path_len[p] = dropped ? 0 : fin_l;
        }
        wave_lds_sync();                                        // ny_s / nx_s / the boundary row: the next pair's
    }
}

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

extern "C" int64_t abn_dtw_cost_max_n2(void) { return MAXN2; }

extern "C" int abn_dtw_cost_batched(const float* feats1, int64_t rows1, const float* feats2, int64_t rows2,
                                    const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                                    int64_t npairs, int64_t D, double* total_cost, int32_t* path_len, void* stream)
{
    ABN_REQUIRE(npairs >= 0 && D >= 1 && D < (1 << 20) && rows1 >= 0 && rows2 >= 0, "dtw_cost: bad npairs/D/rows");
    if (npairs == 0) return ABN_OK;
    ABN_REQUIRE(feats1 && feats2 && off1 && n1 && off2 && n2 && total_cost && path_len, "dtw_cost: null pointer");
    ABN_REQUIRE(rows1 * D < (1LL << 62) && rows2 * D < (1LL << 62), "dtw_cost: feature array too large");
    const int64_t grid = npairs < 256 * 32 ? npairs : 256 * 32;
    const bool vec = D % 4 == 0 && aligned16(feats1) && aligned16(feats2);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((dtw_cost_kernel<true, CELL_COSINE>), dim3((unsigned)grid), dim3(64), 0, st, feats1, rows1, feats2, rows2,
                                off1, n1, off2, n2, npairs, (int)D, total_cost, path_len, cell_extra<CELL_COSINE>());
    else hipLaunchKernelGGL((dtw_cost_kernel<false, CELL_COSINE>), dim3((unsigned)grid), dim3(64), 0, st, feats1, rows1, feats2, rows2,
                            off1, n1, off2, n2, npairs, (int)D, total_cost, path_len, cell_extra<CELL_COSINE>());
    ABN_CHECK_LAUNCH("dtw_cost");
    return ABN_OK;
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
    ABN_REQUIRE(npairs >= 0 && D >= 1 && D < (1 << 20) && rows1 >= 0 && rows2 >= 0, "dtw_cost_kl: bad npairs/D/rows");
    if (npairs == 0) return ABN_OK;
    ABN_REQUIRE(P1 && L1 && P2 && L2 && bad1 && bad2 && off1 && n1 && off2 && n2 && total_cost && path_len,
                "dtw_cost_kl: null pointer");
    ABN_REQUIRE(rows1 * D < (1LL << 62) && rows2 * D < (1LL << 62), "dtw_cost_kl: feature array too large");
    const int64_t grid = npairs < 256 * 32 ? npairs : 256 * 32;
    const bool vec = D % 4 == 0 && aligned16(P1) && aligned16(L1) && aligned16(P2) && aligned16(L2);
    hipStream_t st = (hipStream_t)stream;
    const cell_extra<CELL_KL> ex = {L1, L2, bad1, bad2};
    if (vec) hipLaunchKernelGGL((dtw_cost_kernel<true, CELL_KL>), dim3((unsigned)grid), dim3(64), 0, st, P1, rows1, P2, rows2,
                                off1, n1, off2, n2, npairs, (int)D, total_cost, path_len, ex);
    else hipLaunchKernelGGL((dtw_cost_kernel<false, CELL_KL>), dim3((unsigned)grid), dim3(64), 0, st, P1, rows1, P2, rows2,
                            off1, n1, off2, n2, npairs, (int)D, total_cost, path_len, ex);
    ABN_CHECK_LAUNCH("dtw_cost_kl");
    return ABN_OK;
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
