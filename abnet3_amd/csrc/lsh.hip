// lsh.hip -- the prefilter of spoken-term discovery (abnet3_amd/prefilter.py): random-hyperplane signatures of every
// frame, and for every kernel pair of TermDiscoverer the longest diagonal run of near-equal signatures in its "dot
// plot".  The contract is include/abnet3_hip.h's; tests/prefilter_np.py restates both in numpy.  All-integer apart from
// the dot products of the signatures: no atomics, no workspace, the same bits on every call.
//
// lsh_signatures_kernel: a workgroup of 256 threads takes 32 table rows and walks D in chunks of 32 columns: the chunk
// of the rows and of all planes is staged in LDS (rows padded to 36 floats: read four columns at a time, conflict-free),
// thread (tx, ty) keeps the dot products of rows 4 ty .. 4 ty + 3 with planes tx, tx + 32, ... in
// registers -- tx is the plane's bit inside its word, so one __ballot is two finished words (the two ty of a wavefront).
// The table is read from memory once; the planes (at most 4 MiB, usually 25 KiB) come from L2 once per workgroup.  The
// thread sees every element of its rows on the way and settles `live` itself.
//
// lsh_diag_hits_kernel: one workgroup of four wavefronts per pair, a grid-stride loop over pairs.  Side 2's signatures
// (word-major, so that a wavefront's read of one word is consecutive addresses) and live bytes are staged in LDS.  A
// wavefront takes blocks of 64 consecutive diagonals k = i - j, one per lane, and steps through the rows i of side 1
// that cross the block: 64 rows are loaded one per lane and handed round by index, lane l compares with column
// j = i - k.  The dilation is an OR over 2 dilate + 1 neighbouring bits of the step's __ballot, which is why blocks
// overlap by 2 dilate lanes: the outer `dilate` lanes on either side only supply hits.  The window count is the
// population count of a 64-bit history register.  A lane keeps its best (run, diagonal, row) under "strictly greater"
// -- its diagonals and rows only grow --, the wavefront and then the workgroup reduce in the tie order.
#include <math.h>

#include "common.h"

using namespace abn;

namespace {

constexpr int SIG_ROWS = 32, SIG_DC = 32, SIG_THREADS = 256, SIG_RT = 4;
constexpr int SIG_LD = SIG_DC + 4;      // floats per staged row: 16-byte rows, and 16 lanes' float4 reads of one column cover all banks once
static_assert(SIG_THREADS / 32 * SIG_RT == SIG_ROWS, "thread (tx, ty) owns rows 4 ty .. 4 ty + 3");

template <int NQ>
__global__ __launch_bounds__(SIG_THREADS) void lsh_signatures_kernel(const float* __restrict__ table, int64_t rows, int D,
                                                                     const float* __restrict__ planes,
                                                                     uint32_t* __restrict__ sig, uint8_t* __restrict__ live)
{
    __shared__ __align__(16) float xs[SIG_ROWS][SIG_LD];
    __shared__ __align__(16) float ps[NQ * 32][SIG_LD];
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * SIG_ROWS;
    float acc[SIG_RT][NQ];
    bool bad[SIG_RT], nonzero[SIG_RT];
#pragma unroll
    for (int rr = 0; rr < SIG_RT; ++rr) {
        bad[rr] = nonzero[rr] = false;
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[rr][q] = 0.0f;
    }
    for (int d0 = 0; d0 < D; d0 += SIG_DC) {
        // (columns past D and rows past the table are staged as zeros and never read from memory)
        for (int idx = t; idx < SIG_ROWS * SIG_DC; idx += SIG_THREADS) {
            const int r = idx / SIG_DC, d = idx % SIG_DC;
            xs[r][d] = (r0 + r < rows && d0 + d < D) ? table[(r0 + r) * D + d0 + d] : 0.0f;
        }
        for (int idx = t; idx < NQ * 32 * SIG_DC; idx += SIG_THREADS) {
            const int b = idx / SIG_DC, d = idx % SIG_DC;
            ps[b][d] = d0 + d < D ? planes[(int64_t)b * D + d0 + d] : 0.0f;
        }
        __syncthreads();
#pragma unroll 2
        for (int d = 0; d < SIG_DC; d += 4) {                       // four columns per LDS read, added in ascending order
            float4 x[SIG_RT];
#pragma unroll
            for (int rr = 0; rr < SIG_RT; ++rr) {
                x[rr] = *reinterpret_cast<const float4*>(&xs[ty * SIG_RT + rr][d]);
                // NaN, +inf, -inf
                bad[rr] |= !(fabsf(x[rr].x) < INFINITY) || !(fabsf(x[rr].y) < INFINITY) || !(fabsf(x[rr].z) < INFINITY) ||
                           !(fabsf(x[rr].w) < INFINITY);
                nonzero[rr] |= x[rr].x != 0.0f || x[rr].y != 0.0f || x[rr].z != 0.0f || x[rr].w != 0.0f;
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const float4 pl = *reinterpret_cast<const float4*>(&ps[q * 32 + tx][d]);
#pragma unroll
                for (int rr = 0; rr < SIG_RT; ++rr)
                    acc[rr][q] = fmaf(x[rr].w, pl.w, fmaf(x[rr].z, pl.z, fmaf(x[rr].y, pl.y, fmaf(x[rr].x, pl.x, acc[rr][q]))));
            }
        }
        __syncthreads();
    }
    // a wavefront holds ty = 2 w (lanes 0 .. 31) and 2 w + 1 (lanes 32 .. 63): the ballot's halves are their words
#pragma unroll
    for (int rr = 0; rr < SIG_RT; ++rr) {
        const int64_t row = r0 + ty * SIG_RT + rr;
        const bool alive = !bad[rr] && nonzero[rr];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const unsigned long long m = __ballot(alive && acc[rr][q] > 0.0f);
            const uint32_t word = (ty & 1) ? (uint32_t)(m >> 32) : (uint32_t)m;
            if (tx == 0 && row < rows) sig[row * NQ + q] = word;
        }
        if (tx == 0 && row < rows) live[row] = alive ? 1 : 0;
    }
}

constexpr int DH_WAVES = 4, DH_THREADS = 64 * DH_WAVES, DH_CAP = ABN_DTW_LOCAL_MAX_N2;

// (run, diagonal, row) a beats b: the larger run, then the smaller diagonal, then the smaller row
__device__ __forceinline__ bool dh_better(int ar, int ad, int ai, int br, int bd, int bi)
{
    return ar > br || (ar == br && (ad < bd || (ad == bd && ai < bi)));
}

template <int W>
__global__ __launch_bounds__(DH_THREADS) void lsh_diag_hits_kernel(
    const uint32_t* __restrict__ sig1, const uint8_t* __restrict__ live1, int64_t rows1, const uint32_t* __restrict__ sig2,
    const uint8_t* __restrict__ live2, int64_t rows2, const int64_t* __restrict__ off1, const int32_t* __restrict__ n1,
    const int64_t* __restrict__ off2, const int32_t* __restrict__ n2, int64_t npairs, int max_hamming, int span, int dilate,
    int64_t exclude, int32_t* __restrict__ best, int32_t* __restrict__ diag, int32_t* __restrict__ end1)
{
    __shared__ uint32_t s2[W][DH_CAP];
    __shared__ uint8_t l2s[DH_CAP];
    __shared__ int32_t red[DH_WAVES][3];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned long long smask = span >= 64 ? ~0ull : ((1ull << span) - 1);
    const unsigned long long dmask = (1ull << (2 * dilate + 1)) - 1;
    const int U = 64 - 2 * dilate;                                  // the diagonals a block reports
    const bool useful = lane >= dilate && lane < 64 - dilate;
    const int dshift = lane >= dilate ? lane - dilate : 0;
    for (int64_t p = blockIdx.x; p < npairs; p += gridDim.x) {
        const int64_t o1 = off1[p], o2 = off2[p];
        const int32_t l1 = n1[p], l2 = n2[p];
        // (l >= 0 first: rows - l cannot overflow) -- the same for every thread of the workgroup
        if (l1 < 0 || l2 < 0 || o1 < 0 || o2 < 0 || o1 > rows1 - l1 || o2 > rows2 - l2 || l2 > DH_CAP) {
            if (threadIdx.x == 0) best[p] = -1, diag[p] = 0, end1[p] = -1;
            continue;
        }
        if (l1 == 0 || l2 == 0) {
            if (threadIdx.x == 0) best[p] = 0, diag[p] = 0, end1[p] = -1;
            continue;
        }
        for (int j = threadIdx.x; j < l2; j += DH_THREADS) {
            l2s[j] = live2[o2 + j];
#pragma unroll
            for (int w = 0; w < W; ++w) s2[w][j] = sig2[(o2 + j) * W + w];
        }
        __syncthreads();
        int bb = 0, bd = 0, bi = -1;
        const int64_t kmin = -(int64_t)(l2 - 1), nd = (int64_t)l1 + l2 - 1;
        const int64_t nb = (nd + U - 1) / U;
        for (int64_t b = wave; b < nb; b += DH_WAVES) {
            const int64_t kbase = kmin + b * U - dilate;            // lane 0's diagonal
            const int64_t k = kbase + lane;
            const int64_t gap = o1 - o2 + k;                        // (off1 + i) - (off2 + j) anywhere on diagonal k
            const bool allowed = exclude == 0 || gap >= exclude || -gap >= exclude;
            const int64_t ilo = kbase > 0 ? kbase : 0;
            const int64_t top = kbase + 63 + l2 - 1;
            const int64_t ihi = top < l1 - 1 ? top : l1 - 1;
            unsigned long long hist = 0;
            for (int64_t ic = ilo; ic <= ihi; ic += 64) {
                const int64_t row = ic + lane;
                const bool have = row <= ihi;
                const bool lv = have && live1[o1 + row] != 0;
                uint32_t mine[W];
#pragma unroll
                for (int w = 0; w < W; ++w) mine[w] = lv ? sig1[(o1 + row) * W + w] : 0u;
                const unsigned long long l1m = __ballot(lv);
                const int nr = ihi - ic + 1 < 64 ? (int)(ihi - ic + 1) : 64;
                for (int r = 0; r < nr; ++r) {
                    const int64_t jj = ic + r - k;
                    const bool inr = jj >= 0 && jj < l2;
                    bool hit = false;
                    if ((l1m >> r) & 1) {                           // the same for every lane
                        const int j = inr ? (int)jj : 0;
                        int ham = 0;
#pragma unroll
                        for (int w = 0; w < W; ++w) ham += __popc(__shfl(mine[w], r) ^ s2[w][j]);
                        hit = inr && allowed && l2s[j] != 0 && ham <= max_hamming;
                    }
                    const unsigned long long m = __ballot(hit);
                    const bool h = inr && ((m >> dshift) & dmask) != 0;
                    hist = (hist << 1) | (h ? 1ull : 0ull);
                    const int run = __popcll(hist & smask);
                    if (useful && inr && run > bb) bb = run, bd = (int)k, bi = (int)(ic + r);
                }
            }
        }
        for (int s = 32; s; s >>= 1) {
            const int ob = __shfl_xor(bb, s), od = __shfl_xor(bd, s), oi = __shfl_xor(bi, s);
            if (dh_better(ob, od, oi, bb, bd, bi)) bb = ob, bd = od, bi = oi;
        }
        if (lane == 0) red[wave][0] = bb, red[wave][1] = bd, red[wave][2] = bi;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < DH_WAVES; ++w)
                if (dh_better(red[w][0], red[w][1], red[w][2], bb, bd, bi)) bb = red[w][0], bd = red[w][1], bi = red[w][2];
            best[p] = bb, diag[p] = bb > 0 ? bd : 0, end1[p] = bb > 0 ? bi : -1;
        }
        // (the next pair's staging is behind this barrier for every wavefront; its `red` writes behind the next one)
    }
}

}  // namespace

extern "C" int abn_lsh_signatures(const float* table, int64_t rows, int64_t D, const float* planes, int64_t bits,
                                  uint32_t* sig, uint8_t* live, void* stream)
{
    ABN_REQUIRE(bits >= 32 && bits <= ABN_LSH_MAX_BITS && bits % 32 == 0, "lsh_signatures: bits must be a multiple of 32 in 32 .. %d, not %lld",
                ABN_LSH_MAX_BITS, (long long)bits);
    ABN_REQUIRE(D >= 1 && D <= ABN_LSH_MAX_D, "lsh_signatures: D must lie in 1 .. %d, not %lld", ABN_LSH_MAX_D, (long long)D);
    ABN_REQUIRE(rows >= 0 && rows < (1LL << 35), "lsh_signatures: rows must lie in 0 .. 2^35 - 1");
    if (rows == 0) return ABN_OK;
    ABN_REQUIRE(table && planes && sig && live, "lsh_signatures: null pointer");
    const dim3 grid((unsigned)((rows + SIG_ROWS - 1) / SIG_ROWS)), block(SIG_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define ABN_LSH_SIG(NQ) \
    case NQ: hipLaunchKernelGGL((lsh_signatures_kernel<NQ>), grid, block, 0, st, table, rows, (int)D, planes, sig, live); break
    switch (bits / 32) {
        ABN_LSH_SIG(1); ABN_LSH_SIG(2); ABN_LSH_SIG(3); ABN_LSH_SIG(4);
        ABN_LSH_SIG(5); ABN_LSH_SIG(6); ABN_LSH_SIG(7); ABN_LSH_SIG(8);
    }
#undef ABN_LSH_SIG
    ABN_CHECK_LAUNCH("lsh_signatures");
    return ABN_OK;
}

extern "C" int abn_lsh_diag_hits_batched(const uint32_t* sig1, const uint8_t* live1, int64_t rows1, const uint32_t* sig2,
                                         const uint8_t* live2, int64_t rows2, const int64_t* off1, const int32_t* n1,
                                         const int64_t* off2, const int32_t* n2, int64_t npairs, int64_t words,
                                         int64_t max_hamming, int64_t span, int64_t dilate, int64_t exclude, int32_t* best,
                                         int32_t* diag, int32_t* end1, void* stream)
{
    ABN_REQUIRE(words >= 1 && words <= ABN_LSH_MAX_BITS / 32, "lsh_diag_hits: words must lie in 1 .. %d, not %lld",
                ABN_LSH_MAX_BITS / 32, (long long)words);
    ABN_REQUIRE(max_hamming >= 0 && max_hamming <= 32 * words, "lsh_diag_hits: max_hamming must lie in 0 .. %lld (the bits), not %lld",
                (long long)(32 * words), (long long)max_hamming);
    ABN_REQUIRE(span >= 1 && span <= ABN_LSH_MAX_SPAN, "lsh_diag_hits: span must lie in 1 .. %d, not %lld", ABN_LSH_MAX_SPAN,
                (long long)span);
    ABN_REQUIRE(dilate >= 0 && dilate <= ABN_LSH_MAX_DILATE, "lsh_diag_hits: dilate must lie in 0 .. %d, not %lld",
                ABN_LSH_MAX_DILATE, (long long)dilate);
    ABN_REQUIRE(exclude >= 0, "lsh_diag_hits: exclude must be >= 0");
    ABN_REQUIRE(exclude == 0 || (sig1 == sig2 && live1 == live2 && rows1 == rows2),
                "lsh_diag_hits: exclude > 0 needs both sides to be one table");
    ABN_REQUIRE(npairs >= 0 && rows1 >= 0 && rows2 >= 0 && rows1 < (1LL << 58) && rows2 < (1LL << 58), "lsh_diag_hits: bad npairs/rows");
    if (npairs == 0) return ABN_OK;
    ABN_REQUIRE((sig1 || rows1 == 0) && (live1 || rows1 == 0) && (sig2 || rows2 == 0) && (live2 || rows2 == 0) && off1 && n1 &&
                    off2 && n2 && best && diag && end1,
                "lsh_diag_hits: null pointer");
    const dim3 grid((unsigned)(npairs < ABN_LSH_GRID_BLOCKS ? npairs : ABN_LSH_GRID_BLOCKS)), block(DH_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define ABN_LSH_DH(W)                                                                                                        \
    case W:                                                                                                                  \
        hipLaunchKernelGGL((lsh_diag_hits_kernel<W>), grid, block, 0, st, sig1, live1, rows1, sig2, live2, rows2, off1, n1,  \
                           off2, n2, npairs, (int)max_hamming, (int)span, (int)dilate, exclude, best, diag, end1);           \
        break
    switch (words) {
        ABN_LSH_DH(1); ABN_LSH_DH(2); ABN_LSH_DH(3); ABN_LSH_DH(4);
        ABN_LSH_DH(5); ABN_LSH_DH(6); ABN_LSH_DH(7); ABN_LSH_DH(8);
    }
#undef ABN_LSH_DH
    ABN_CHECK_LAUNCH("lsh_diag_hits");
    return ABN_OK;
}
