// sampler.hip -- abn_sample_pairs: every pair of one data set (train or dev) in one launch, one lane per pair.
//
// The reference (abnet3/sampler.py:404-473) materialises one dictionary entry per ordered pair of cells and samples
// that table.  Every entry is a product of one factor per cell, so the same distribution is drawn here by exact
// conditional decomposition from O(cells) tables (include/abnet3_hip.h, abn_sampler_tables):
//   first cell a  ~  its marginal = weight(a) x total weight of a's admissible partners (cum_m[q], one search);
//   second cell b ~  weight(b) among a's admissible partners: a search in a running sum from which the excluded
//                    cell (Stype_Dspk, Dtype_Sspk) or the excluded speaker AND type (Dtype_Dspk) are cut out.
// Dtype_Dspk's partners are "not a's speaker, not a's type": in S order a's speaker is one range, the cells of
// a's type are one per speaker.  The search runs over speakers on H(x) = (running sum of the speakers' totals up to
// x) - (what the cells of a's type contribute up to speaker x, a search in the type's range in T order), then inside
// the speaker found with that speaker's cell of a's type cut out.
// All arithmetic is integer: nothing here rounds, and tests/sampler_np.py restates it bit for bit.  Every loop is a
// binary search whose trip count is bounded by the table sizes; there is no rejection and no retry.  The kernel is
// latency-bound on dependent loads from tables that sit in L2: small register footprint, full occupancy, no LDS.
#include "common.h"
#include "philox.h"

namespace abn {

struct SamplerP {
    abn_sampler_tables t;
    int64_t off[5];                 // first output element of each configuration; off[4] = all
    uint32_t k0, k1;                // Philox key = seed
    int32_t* tok1; int32_t* tok2; int64_t* key;
};

// (philox4x32_10 and map128: philox.h, shared with tcl.hip)

// first index in [lo, hi) whose running sum exceeds x (hi if none)
__device__ __forceinline__ int upper_u64(const uint64_t* __restrict__ cum, int lo, int hi, uint64_t x)
{
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > x) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// first index in [lo, hi) of the ascending v with v[index] > x / >= x
__device__ __forceinline__ int upper_i32(const int32_t* __restrict__ v, int lo, int hi, int x)
{
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v[mid] > x) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__device__ __forceinline__ int lower_i32(const int32_t* __restrict__ v, int lo, int hi, int x)
{
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v[mid] >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__device__ __forceinline__ uint64_t before(const uint64_t* __restrict__ cum, int i) { return i > 0 ? cum[i - 1] : 0; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Dtype_Dspk: what the speakers 0 .. x hold outside the type whose cells are T-order [tb, te)
__device__ __forceinline__ uint64_t dd_H(const abn_sampler_tables& t, int x, int tb, int te, uint64_t base_t)
{
    if (x < 0) return 0;
    const int c = upper_i32(t.spk_t, tb, te, x);
    return t.cum_spk[x] - (before(t.cum_u_t, c) - base_t);
}

__global__ __launch_bounds__(1024) void sample_pairs_kernel(SamplerP p)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= p.off[4]) return;
    const int q = (g >= p.off[1]) + (g >= p.off[2]) + (g >= p.off[3]);
    const uint64_t i = (uint64_t)(g - p.off[q]);
    const uint32_t i0 = (uint32_t)i, i1 = (uint32_t)(i >> 32);
    const abn_sampler_tables& t = p.t;
    const int K = t.n_cells;

    const U4 rk = philox4x32_10(i0, i1, (uint32_t)q, 3u, p.k0, p.k1);
    p.key[g] = (int64_t)((((uint64_t)rk.y << 32) | rk.x) >> 1);
    const uint64_t M = t.total[q];
    if (M == 0) {                                            // empty support: the caller asks for none of these
        p.tok1[g] = -1;
        p.tok2[g] = -1;
        return;
    }
    const U4 r0 = philox4x32_10(i0, i1, (uint32_t)q, 0u, p.k0, p.k1);
    const U4 r1 = philox4x32_10(i0, i1, (uint32_t)q, 1u, p.k0, p.k1);
    const U4 r2 = philox4x32_10(i0, i1, (uint32_t)q, 2u, p.k0, p.k1);
    const uint64_t ra = ((uint64_t)r2.y << 32) | r2.x, rb = ((uint64_t)r2.w << 32) | r2.z;

    const int a = clampi(upper_u64(t.cum_m + (int64_t)q * K, 0, K, map128(r0, M)), 0, K - 1);
    int ca, cb;                                              // the two cells in T order
    bool same_cell = false;
    if (q == 0) {
        ca = cb = a;
        same_cell = true;
    } else if (q == 1) {
        const int ty = t.type_t[a], tb = t.type_beg[ty], te = t.type_beg[ty + 1];
        const uint64_t base = before(t.cum_f_t, tb), fa = t.f_t[a];
        uint64_t y = map128(r1, t.cum_f_t[te - 1] - base - fa);
        if (y >= before(t.cum_f_t, a) - base) y += fa;
        ca = a;
        cb = clampi(upper_u64(t.cum_f_t, tb, te, base + y), tb, te - 1);
    } else if (q == 2) {
        const int sp = t.spk_s[a], sb = t.spk_beg[sp], se = t.spk_beg[sp + 1];
        const uint64_t base = before(t.cum_u_s, sb), ua = t.u_s[a];
        uint64_t y = map128(r1, t.cum_u_s[se - 1] - base - ua);
        if (y >= before(t.cum_u_s, a) - base) y += ua;
        const int b = clampi(upper_u64(t.cum_u_s, sb, se, base + y), sb, se - 1);
        const bool swap = t.type_s[b] < t.type_s[a];
        ca = t.s2t[swap ? b : a];
        cb = t.s2t[swap ? a : b];
    } else {
        const int sp = t.spk_s[a], ty = t.type_s[a];
        const int sb = t.spk_beg[sp], se = t.spk_beg[sp + 1], tb = t.type_beg[ty], te = t.type_beg[ty + 1];
        const uint64_t base_t = before(t.cum_u_t, tb), ua = t.u_s[a];
        const uint64_t u_spk = t.cum_u_s[se - 1] - before(t.cum_u_s, sb), u_type = t.cum_u_t[te - 1] - base_t;
        uint64_t y = map128(r1, t.cum_spk[t.n_spk - 1] - u_spk - u_type + ua);
        if (y >= dd_H(t, sp - 1, tb, te, base_t)) y += u_spk - ua;          // a's speaker cut out
        int lo = 0, hi = t.n_spk;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (dd_H(t, mid, tb, te, base_t) > y) hi = mid; else lo = mid + 1;
        }
        const int x = clampi(lo, 0, t.n_spk - 1);
        uint64_t z = y - dd_H(t, x - 1, tb, te, base_t);
        const int xb = t.spk_beg[x], xe = t.spk_beg[x + 1];
        const uint64_t base_x = before(t.cum_u_s, xb);
        const int e = lower_i32(t.type_s, xb, xe, ty);                       // x's cell of a's type cut out
        if (e < xe && t.type_s[e] == ty && z >= before(t.cum_u_s, e) - base_x) z += t.u_s[e];
        const int b = clampi(upper_u64(t.cum_u_s, xb, xe, base_x + z), xb, xe - 1);
        const bool swap = t.type_s[b] < ty;
        ca = t.s2t[swap ? b : a];
        cb = t.s2t[swap ? a : b];
    }
    ca = clampi(ca, 0, K - 1);
    cb = clampi(cb, 0, K - 1);
    const int oa = t.tok_beg[ca], na = t.tok_beg[ca + 1] - oa;
    const int ob = t.tok_beg[cb], nb = t.tok_beg[cb + 1] - ob;
    int ia = (int)__umul64hi(ra, (uint64_t)na), ib;
    if (same_cell) {                                         // two distinct tokens of one cell, ordered, uniform
        ib = nb > 1 ? (int)__umul64hi(rb, (uint64_t)(nb - 1)) : 0;
        if (ib >= ia && nb > 1) ++ib;
    } else {
        ib = (int)__umul64hi(rb, (uint64_t)nb);
    }
    p.tok1[g] = t.toks[clampi(oa + ia, 0, t.n_tok - 1)];
    p.tok2[g] = t.toks[clampi(ob + ib, 0, t.n_tok - 1)];
}

}  // namespace abn

using namespace abn;

extern "C" int abn_sample_pairs(const abn_sampler_tables* tables, const int64_t* n, uint64_t seed, int32_t* tok1,
                                int32_t* tok2, int64_t* key, int block, void* stream)
{
    ABN_REQUIRE(tables && n, "abn_sample_pairs: null tables / counts");
    const abn_sampler_tables& t = *tables;
    ABN_REQUIRE(t.n_cells >= 1 && t.n_cells < (1 << 24) && t.n_spk >= 1 && t.n_spk <= t.n_cells && t.n_type >= 1 &&
                t.n_tok >= t.n_cells,                       // (a type may be empty: a cluster that a split emptied)
                "abn_sample_pairs: n_cells = %d, n_spk = %d, n_type = %d, n_tok = %d out of range", t.n_cells, t.n_spk,
                t.n_type, t.n_tok);
    ABN_REQUIRE(t.spk_t && t.type_t && t.type_beg && t.f_t && t.cum_u_t && t.cum_f_t && t.tok_beg && t.toks && t.spk_s &&
                t.type_s && t.s2t && t.spk_beg && t.u_s && t.cum_u_s && t.cum_spk && t.cum_m,
                "abn_sample_pairs: null table pointer");
    ABN_REQUIRE(block >= 64 && block <= 1024 && block % 64 == 0, "abn_sample_pairs: block = %d, a multiple of 64 in 64 .. 1024", block);
    SamplerP p;
    p.t = t;
    p.off[0] = 0;
    for (int q = 0; q < 4; ++q) {
        ABN_REQUIRE(n[q] >= 0 && n[q] < (1LL << 31), "abn_sample_pairs: n[%d] = %lld out of range", q, (long long)n[q]);
        p.off[q + 1] = p.off[q] + n[q];
    }
    ABN_REQUIRE(p.off[4] < (1LL << 31), "abn_sample_pairs: %lld pairs, fewer than 2^31 supported", (long long)p.off[4]);
    if (p.off[4] == 0) return ABN_OK;
    ABN_REQUIRE(tok1 && tok2 && key, "abn_sample_pairs: null output pointer");
    p.k0 = (uint32_t)seed; p.k1 = (uint32_t)(seed >> 32);
    p.tok1 = tok1; p.tok2 = tok2; p.key = key;
    hipLaunchKernelGGL(sample_pairs_kernel, dim3((unsigned)((p.off[4] + block - 1) / block)), dim3(block), 0,
                       static_cast<hipStream_t>(stream), p);
    ABN_CHECK_LAUNCH("abn_sample_pairs");
    return ABN_OK;
}
