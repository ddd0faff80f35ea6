// knn.hip -- k nearest neighbours of fixed-size segment vectors by cosine similarity (abn_knn_topk), and the
// gather + normalise kernel that builds those vectors from a feature table (abn_segment_vectors).
//
// The search is one large GEMM, S = Q C^T (rows of both L2-normalised by the caller), whose nq x nc result is
// never written anywhere: a workgroup owns a block of 128 queries and a range of 128-wide candidate tiles, forms
// each 128 x 128 similarity tile on the matrix cores in exact fp32 (v_mfma_f32_32x32x2_f32, the tiles, loaders and
// register-staged double buffering of gemm_f32.h, both operands K-contiguous), and folds it into the queries'
// running top-k lists, which stay in LDS for the workgroup's whole life:
//   * the tile's accumulators go through LDS (the k loop's tile buffers are free by then), one row per query;
//   * thread r < 128 owns query row r and its list.  It keeps the list's k-th similarity (tau) in a register and
//     walks its row: one compare, `v > tau`, rejects almost everything once the list has warmed up.  A workgroup
//     meets its candidates in ascending j, so an element that ties with the k-th place never displaces it and a
//     strict compare is the whole order (sim descending, j ascending);
//   * a survivor is checked for the bounds of C and for the overlap exclusion (three ints of c_meta, read only
//     here), then inserted by shifting the tail of the sorted list: O(k) LDS moves, rare.
// The candidate range is split over `split` workgroups per query block so that a small nq still fills the chip and
// so that a large one keeps its query blocks in L2 (8 query blocks x 4 ranges per XCD instead of 32 query blocks);
// each writes a partial list and knn_merge_kernel selects the k best of a query's split * k entries under the same
// total order.  The order is total (j is unique), the top k of a set under a total order do not depend on how the
// set was partitioned, and sim(i, j) is one MFMA accumulation chain over k = 0, 2, 4, ... whatever tile or range j
// falls in (tiles start at multiples of 128 for every split): the output is bit-identical for any split factor.
#include "common.h"
#include "gemm_f32.h"

#include <math.h>

namespace abn {

constexpr int KN_B = 128;                 // query block = candidate tile = 128 (2 x 2 waves of 2 x 2 MFMA blocks)
constexpr int KN_SST = KN_B + 1;          // staging row stride: thread r reads row r, 129 dwords apart = conflict-free
constexpr int KN_MAX_K = 32;
constexpr int KN_MAX_D = 4096;
constexpr int KN_MAX_SPLIT = 64;
using KnTile = TileShape<KN_B, true>;
constexpr size_t KN_TILE_BYTES = sizeof(float) * 4 * KnTile::floats;          // two stages of each operand
static_assert(KN_TILE_BYTES >= sizeof(float) * KN_B * KN_SST, "the similarity tile is staged in the operand buffers");
static inline size_t knn_lds_bytes(int k) { return KN_TILE_BYTES + (size_t)k * KN_B * 8; }

struct KnnP {
    const float* Q; const float* C;
    int nq, nc, d, k;
    const int32_t* qm; const int32_t* cm;        // [n][3] file, begin, end -- both or neither
    int split, tiles_per_split, tiles_c, qblocks;
    int32_t* idx; float* sim;                    // [nq][split][k]
};

__global__ __launch_bounds__(256) void knn_tile_topk_kernel(KnnP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const As = smem;
    float* const Bs = smem + 2 * KnTile::floats;
    float* const stage = smem;
    float* const lsim = smem + 4 * KnTile::floats;                        // [k][128]
    int32_t* const lidx = reinterpret_cast<int32_t*>(lsim + p.k * KN_B);  // [k][128]

    // Workgroups b, b + 8, ... share an XCD: give each XCD a contiguous run of (query block, range) pairs, the
    // ranges of a query block next to each other.
    const int total = p.qblocks * p.split;
    int w = (int)blockIdx.x;
    if ((total & 7) == 0) w = (w & 7) * (total >> 3) + (w >> 3);
    const int qblk = w / p.split, s = w % p.split;
    const int m0 = qblk * KN_B;
    const int t0 = s * p.tiles_per_split, t1 = min(p.tiles_c, t0 + p.tiles_per_split);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    const int ke = p.d, nkt = (p.d + BK - 1) / BK;
    constexpr int PT = KnTile::per_thread;

    // the list of query row t (threads 0 .. 127)
    const int qi = m0 + t;
    const bool owner = t < KN_B && qi < p.nq;
    const bool excl = p.qm != nullptr;
    int cnt = 0, qf = 0, qb = 0, qe = 0;
    float tau = -INFINITY;
    if (owner && excl) { qf = p.qm[3 * (int64_t)qi]; qb = p.qm[3 * (int64_t)qi + 1]; qe = p.qm[3 * (int64_t)qi + 2]; }

    f32x4 ra[PT], rb[PT];
    uint32_t voa[PT], vob[PT];
    tile_offsets<KN_B, true>(voa, p.d);
    tile_offsets<KN_B, true>(vob, p.d);
    const bool a_in = m0 + KN_B <= p.nq;
    const float* const a_org = p.Q + (int64_t)m0 * p.d;

    auto issue = [&](int n0, int k0) {
        const bool k_in = k0 + BK <= ke, b_in = n0 + KN_B <= p.nc;
        if (a_in && k_in) tile_issue_fast<KN_B, true>(ra, a_org + k0, voa);
        else tile_issue<KN_B, true, true, false>(ra, p.Q, p.d, p.nq, m0, k0, ke);
        if (b_in && k_in) tile_issue_fast<KN_B, true>(rb, p.C + (int64_t)n0 * p.d + k0, vob);
        else tile_issue<KN_B, true, true, false>(rb, p.C, p.d, p.nc, n0, k0, ke);
    };
    auto commit = [&](int n0, int k0, float* as, float* bs) {
        const bool k_in = k0 + BK <= ke, b_in = n0 + KN_B <= p.nc;
        if (a_in && k_in) tile_commit<KN_B, true, true>(ra, as, p.nq, m0, k0, ke, -1);
        else tile_commit<KN_B, true, false>(ra, as, p.nq, m0, k0, ke, -1);
        if (b_in && k_in) tile_commit<KN_B, true, true>(rb, bs, p.nc, n0, k0, ke, -1);
        else tile_commit<KN_B, true, false>(rb, bs, p.nc, n0, k0, ke, -1);
    };

    if (t0 < t1) issue(t0 * KN_B, 0);
    for (int ct = t0; ct < t1; ++ct) {
        const int n0 = ct * KN_B;
        const bool b_in = n0 + KN_B <= p.nc;
        const float* const b_org = p.C + (int64_t)n0 * p.d;
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
            const float* as = As + cur * KnTile::floats;
            const float* bs = Bs + cur * KnTile::floats;
            // an interior next k-tile's loads are spread behind the first two k-groups' MFMAs (gemm_f32.h)
            const bool fast = more && a_in && b_in && (knext + BK <= ke);
            if (more && !fast) issue(n0, knext);
#pragma unroll
            for (int g = 0; g < BK / 8; ++g) {
                f32x4 fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) fa[i] = frag_read<KN_B, true>(as, wm0 + 32 * i, g, lane);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[j] = frag_read<KN_B, true>(bs, wn0 + 32 * j, g, lane);
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
            if (more) commit(n0, knext, As + (cur ^ 1) * KnTile::floats, Bs + (cur ^ 1) * KnTile::floats);
            __syncthreads();
        }

        // the next candidate tile's first loads fly while this one is folded
        if (ct + 1 < t1) issue(n0 + KN_B, 0);

        // Accumulator register r of lane l holds row (r&3) + 8 (r>>2) + 4 (l>>5), column l&31 of its 32 x 32 block.
        {
            const int col_l = lane & 31, rsub = 4 * (lane >> 5);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        stage[(wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub) * KN_SST + wn0 + 32 * j + col_l] = acc[i][j][r];
        }
        __syncthreads();
        if (owner) {
            const float* const row = stage + t * KN_SST;
            const int k = p.k;
#pragma unroll 4
            for (int c = 0; c < KN_B; ++c) {
                const float v = row[c];
                if (!(v > tau)) continue;
                const int j = n0 + c;
                if (j >= p.nc) continue;                      // the zero fill past C's last row
                if (excl) {
                    const int32_t* m = p.cm + 3 * (int64_t)j;
                    if (m[0] == qf && qb < m[2] && m[1] < qe) continue;
                }
                int pos = cnt < k ? cnt : k - 1;
                while (pos > 0 && lsim[(pos - 1) * KN_B + t] < v) {
                    lsim[pos * KN_B + t] = lsim[(pos - 1) * KN_B + t];
                    lidx[pos * KN_B + t] = lidx[(pos - 1) * KN_B + t];
                    --pos;
                }
                lsim[pos * KN_B + t] = v;
                lidx[pos * KN_B + t] = j;
                if (cnt < k) ++cnt;
                if (cnt == k) tau = lsim[(k - 1) * KN_B + t];
            }
        }
        __syncthreads();
    }

    if (owner) {
        const int64_t o = ((int64_t)qi * p.split + s) * p.k;
        for (int q = 0; q < p.k; ++q) {
            p.idx[o + q] = q < cnt ? lidx[q * KN_B + t] : -1;
            p.sim[o + q] = q < cnt ? lsim[q * KN_B + t] : -INFINITY;
        }
    }
}

// One thread per query: the k best of its split * k partial entries by (sim descending, j ascending), selected one
// at a time as "the best entry that comes after the one just written" -- no per-thread arrays, no scratch.
__global__ __launch_bounds__(256) void knn_merge_kernel(const int32_t* __restrict__ pidx, const float* __restrict__ psim,
                                                         int nq, int n_part, int k, int32_t* __restrict__ idx,
                                                         float* __restrict__ sim)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const int32_t* const pi = pidx + (int64_t)i * n_part;
    const float* const ps = psim + (int64_t)i * n_part;
    float last_s = INFINITY;
    int last_j = -1;
    for (int q = 0; q < k; ++q) {
        float best_s = -INFINITY;
        int best_j = -1;
        for (int e = 0; e < n_part; ++e) {
            const int j = pi[e];
            const float v = ps[e];
            if (j < 0) continue;
            const bool after = v < last_s || (v == last_s && j > last_j);
            const bool better = best_j < 0 || v > best_s || (v == best_s && j < best_j);
            if (after && better) { best_s = v; best_j = j; }
        }
        idx[(int64_t)i * k + q] = best_j;
        sim[(int64_t)i * k + q] = best_s;
        if (best_j < 0) {                       // nothing left: the tail is -1 / -inf
            for (int r = q + 1; r < k; ++r) { idx[(int64_t)i * k + r] = -1; sim[(int64_t)i * k + r] = -INFINITY; }
            return;
        }
        last_s = best_s;
        last_j = best_j;
    }
}

// One wavefront per segment: frame j of the vector is table row row0 + ((2j + 1) L) / (2K); the sum of squares is
// accumulated in float64 (exact products, so the norm does not depend on the lanes' order beyond 1e-16), the scale
// (float)(1 / sqrt(ss)) is applied in fp32.
__global__ __launch_bounds__(256) void segment_vectors_kernel(const float* __restrict__ table, int D,
                                                               const int64_t* __restrict__ seg_row0,
                                                               const int32_t* __restrict__ seg_len, int64_t nseg, int K,
                                                               float* __restrict__ out, uint8_t* __restrict__ keep)
{
    const int64_t sgm = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sgm >= nseg) return;
    const int lane = threadIdx.x & 63;
    const int64_t row0 = seg_row0[sgm];
    const int L = seg_len[sgm], n = K * D;
    double ss = 0.0;
    for (int e = lane; e < n; e += 64) {
        const int j = e / D, c = e - j * D;
        const float v = table[(row0 + ((2 * j + 1) * L) / (2 * K)) * D + c];
        ss += (double)v * (double)v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float inv = ss > 0.0 ? (float)(1.0 / sqrt(ss)) : 0.0f;
    float* const dst = out + sgm * n;
    for (int e = lane; e < n; e += 64) {
        const int j = e / D, c = e - j * D;
        dst[e] = table[(row0 + ((2 * j + 1) * L) / (2 * K)) * D + c] * inv;
    }
    if (lane == 0) keep[sgm] = ss > 0.0 ? 1 : 0;
}

// The split factor and what follows from it; shared by the sizing query and the launch.
struct KnnGrid { int qblocks, tiles_c, split, tiles_per_split; };
static KnnGrid knn_grid(int64_t nq, int64_t nc)
{
    KnnGrid g;
    g.qblocks = (int)((nq + KN_B - 1) / KN_B);
    g.tiles_c = (int)((nc + KN_B - 1) / KN_B);
    int s = switches().knn_split;
    if (s <= 0) {                                            // auto: two workgroups per CU at least, four ranges at least
        s = (512 + g.qblocks - 1) / g.qblocks;
        if (s < 4) s = 4;
    }
    if (s > KN_MAX_SPLIT) s = KN_MAX_SPLIT;
    if (s > g.tiles_c) s = g.tiles_c;
    g.tiles_per_split = (g.tiles_c + s - 1) / s;
    g.split = (g.tiles_c + g.tiles_per_split - 1) / g.tiles_per_split;
    return g;
}

static int knn_check_sizes(int64_t nq, int64_t nc, int d, int k, const char* what)
{
    ABN_REQUIRE(nq >= 1 && nc >= 1 && nq < (1 << 30) && nc < (1 << 30), "%s: nq = %lld, nc = %lld out of range", what,
                (long long)nq, (long long)nc);
    if (k < 1 || k > KN_MAX_K) {
        set_error("%s: k = %d, supported 1 .. %d", what, k, KN_MAX_K);
        return ABN_E_UNSUPPORTED;
    }
    if (d < 4 || d > KN_MAX_D || (d & 3)) {
        set_error("%s: d = %d, supported multiples of 4 in 4 .. %d", what, d, KN_MAX_D);
        return ABN_E_UNSUPPORTED;
    }
    return ABN_OK;
}

}  // namespace abn

using namespace abn;

extern "C" int64_t abn_knn_ws_bytes(int64_t nq, int64_t nc, int k)
{
    if (nq < 1 || nc < 1 || nq >= (1 << 30) || nc >= (1 << 30) || k < 1 || k > KN_MAX_K) return -1;
    const KnnGrid g = knn_grid(nq, nc);
    return g.split > 1 ? nq * g.split * k * 8 : 0;
}

extern "C" int abn_knn_topk(const float* Q, int64_t nq, const float* C, int64_t nc, int d, const int32_t* q_meta,
                            const int32_t* c_meta, int k, int32_t* idx, float* sim, void* ws, int64_t ws_bytes,
                            void* stream)
{
    const int rc = knn_check_sizes(nq, nc, d, k, "abn_knn_topk");
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(Q && C && idx && sim, "abn_knn_topk: null pointer");
    ABN_REQUIRE(aligned16(Q) && aligned16(C), "abn_knn_topk: Q and C must be 16-byte aligned");
    const KnnGrid g = knn_grid(nq, nc);
    const int64_t need = g.split > 1 ? nq * g.split * k * 8 : 0;
    if (need > 0 && (!ws || ws_bytes < need)) {
        set_error("abn_knn_topk: workspace of %lld bytes, %lld needed (abn_knn_ws_bytes)", (long long)ws_bytes, (long long)need);
        return ABN_E_WORKSPACE;
    }
    ABN_REQUIRE((int64_t)g.qblocks * g.split < (1LL << 31), "abn_knn_topk: grid too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    static bool attr_set[16] = {};
    if (first_use_on_device(attr_set))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(knn_tile_topk_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)knn_lds_bytes(KN_MAX_K));
    KnnP p;
    p.Q = Q; p.C = C; p.nq = (int)nq; p.nc = (int)nc; p.d = d; p.k = k;
    const bool excl = q_meta && c_meta;
    p.qm = excl ? q_meta : nullptr; p.cm = excl ? c_meta : nullptr;
    p.split = g.split; p.tiles_per_split = g.tiles_per_split; p.tiles_c = g.tiles_c; p.qblocks = g.qblocks;
    if (g.split > 1) {
        p.idx = static_cast<int32_t*>(ws);
        p.sim = reinterpret_cast<float*>(static_cast<char*>(ws) + nq * g.split * k * 4);
    } else {
        p.idx = idx; p.sim = sim;
    }
    hipLaunchKernelGGL(knn_tile_topk_kernel, dim3((unsigned)(g.qblocks * g.split)), dim3(256), knn_lds_bytes(k), st, p);
    ABN_CHECK_LAUNCH("abn_knn_topk");
    if (g.split > 1) {
        hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, p.idx, p.sim, (int)nq,
                           g.split * k, k, idx, sim);
        ABN_CHECK_LAUNCH("abn_knn_topk (merge)");
    }
    return ABN_OK;
}

extern "C" int abn_segment_vectors(const float* table, int64_t D, const int64_t* seg_row0, const int32_t* seg_len,
                                   int64_t nseg, int K, float* out, uint8_t* keep, void* stream)
{
    ABN_REQUIRE(nseg >= 0 && nseg < (1LL << 31), "abn_segment_vectors: nseg = %lld out of range", (long long)nseg);
    if (D < 1 || D > 4096 || K < 1 || K > 1024 || D * K > (1 << 20)) {
        set_error("abn_segment_vectors: D = %lld, K = %d unsupported (1 <= D <= 4096, 1 <= K <= 1024, K D <= 2^20)",
                  (long long)D, K);
        return ABN_E_UNSUPPORTED;
    }
    ABN_REQUIRE(table && seg_row0 && seg_len && out && keep, "abn_segment_vectors: null pointer");
    if (nseg == 0) return ABN_OK;
    hipLaunchKernelGGL(segment_vectors_kernel, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), table, (int)D, seg_row0, seg_len, nseg, K, out, keep);
    ABN_CHECK_LAUNCH("abn_segment_vectors");
    return ABN_OK;
}
