// eskmeans.hip -- embedded segmental k-means (Kamper, Livescu & Goldwater 2017): the two launches of an iteration's
// segmentation, abn_esk_score and abn_esk_segment.  abnet3_amd/eskmeans.py states the definitions, DESIGN.md section
// 3.4f the shapes.
//
// Landmarks: lm [n_lm] int64 rows of table [T][D]; utterance u owns lm[lm_off[u] .. lm_off[u + 1]).  Candidate (g, s),
// 1 <= s <= S, runs from landmark g to g + s of one utterance, covers rows lm[g] .. lm[g + s] - 1 and lives at g S + s - 1.
//   * esk_score_kernel: a workgroup owns 128 consecutive candidates.  It never forms their vectors in memory: per
//     candidate one wave takes the sum of squares of the sampled rows exactly as segment_vectors_kernel (knn.hip) does
//     -- float64, lane e mod 64, then the xor tree -- and keeps (row0, n, 1 / norm) in LDS, with the sampled rows
//     tabulated there too while frames <= 64; the A-operand loader of
//     kmeans_tile.h's score tile then gathers table[row0 + ((2 j + 1) n) / (2 frames)][c] * inv on the way into LDS, with
//     the ones column appended, and the workgroup sweeps the centroid tiles with km_assign_kernel's running (best score,
//     lowest index).  The bits are those of abn_segment_vectors followed by abn_kmeans_assign on the table that is not
//     built.
//   * esk_segment_kernel: one wavefront per utterance.  64 end positions at a time, the lanes turn the candidates'
//     (best, id) into costs in LDS (coalesced loads); lane 0 then takes the 64 dependent steps of the recurrence with
//     the last S values of gamma in registers and leaves the chosen spans in LDS, the lanes store them; lane 0 walks
//     the back-pointers, and the lanes write the outputs.  The chain is a few hundred steps of S additions and
//     comparisons per utterance; the utterances run side by side.
// No floating-point atomics, no workspace; every sum has one order.  Built with -ffp-contract=off (the cost is two
// roundings, as the host restatement takes them).
#include "common.h"
#include "kmeans_tile.h"

#include <limits.h>
#include <math.h>

namespace abn {

constexpr int ESK_MAX_SPAN = 8;
constexpr int ESK_TAB_FRAMES = 64;        // up to here the sampled rows of a workgroup's candidates are tabulated in LDS (<= 32 KiB)

struct EskP {
    const float* table; int T, D;          // D: the feature dimension (KmP::D is the depth frames D)
    const int64_t* lm; const int64_t* lm_off;
    int n_utt; int64_t n_lm;
    int frames, S; int64_t max_frames;
    float* cand_best; int* cand_id;
    int64_t n_cand;
};

// The candidates of a workgroup as the A operand.  row0 / n / inv: LDS, [128]; n = 0 marks a row that contributes zeros.
// tab (frames <= ESK_TAB_FRAMES, else null): the sampled rows [128][frames], so that the division is taken once per
// (candidate, sampled frame) and not once per element and centroid tile.
struct EskCandRows {
    const EskP& e; int depth;
    const int* row0; const int* n; const float* inv; const int* tab;
    __device__ __forceinline__ void issue(float* r, int k0) const
    {
        const int t = threadIdx.x, ka = k0 + (t & 31);
        const int j = ka / e.D, c = ka - j * e.D;
        if (tab) {
            const int jj = ka < depth ? j : 0;
#pragma unroll
            for (int i = 0; i < KM_PT; ++i) {
                const int rl = (t >> 5) + 8 * i;
                r[i] = e.table[(ka < depth && n[rl] > 0) ? (int64_t)tab[rl * e.frames + jj] * e.D + c : 0];
            }
            return;
        }
        const int num = 2 * (ka < depth ? j : 0) + 1, den = 2 * e.frames;    // (j clamped: no product beyond frames n)
#pragma unroll
        for (int i = 0; i < KM_PT; ++i) {
            const int rl = (t >> 5) + 8 * i;
            const int nn = n[rl];
            r[i] = e.table[(ka < depth && nn > 0) ? (int64_t)(row0[rl] + (num * nn) / den) * e.D + c : 0];
        }
    }
    // (as km_x_commit with a zero shift: a non-finite value contributes 0, its candidate is marked by the caller)
    __device__ __forceinline__ void commit(const float* r, float* __restrict__ lds, int k0) const
    {
        const int t = threadIdx.x, ka = k0 + (t & 31);
#pragma unroll
        for (int i = 0; i < KM_PT; ++i) {
            const int rl = (t >> 5) + 8 * i;
            const float xc = r[i] * inv[rl];
            const float v = ka < depth ? (__builtin_isfinite(xc * xc) ? xc : 0.0f) : ka == depth ? 1.0f : 0.0f;
            lds[rl * KmTile::stride + (t & 31)] = n[rl] > 0 ? v : 0.0f;
        }
    }
};

__global__ __launch_bounds__(256) void esk_score_kernel(EskP e, KmP p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int* const tab = e.frames <= ESK_TAB_FRAMES ? reinterpret_cast<int*>(smem + 4 * KmTile::floats) : nullptr;
    __shared__ float red_s[KM_B], inv_s[KM_B];
    __shared__ int red_i[KM_B], row0_s[KM_B], n_s[KM_B];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * KM_B;
    const int depth = p.D;

    // which rows: the candidate's utterance by bisection of lm_off, then every bound that keeps the loads inside
    if (t < KM_B) {
        const int64_t c = c0 + t;
        int row0 = 0, n = 0;
        if (c < e.n_cand) {
            const int64_t g = c / e.S;
            const int s = (int)(c - g * e.S) + 1;
            int lo = 0, hi = e.n_utt;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (e.lm_off[mid] <= g) lo = mid; else hi = mid;
            }
            const int64_t u0 = e.lm_off[lo], u1 = e.lm_off[lo + 1];
            if (g >= u0 && g + s < u1 && u1 <= e.n_lm) {
                const int64_t a = e.lm[g], b = e.lm[g + s];
                const int64_t len = b - a;
                const bool allowed = s == 1 || len <= e.max_frames;
                if (a >= 0 && len >= 1 && b <= e.T && allowed && len <= INT_MAX / (2 * e.frames)) {
                    row0 = (int)a;
                    n = (int)len;
                }
            }
        }
        row0_s[t] = row0;
        n_s[t] = n;
    }
    __syncthreads();
    if (tab)
        for (int u = t; u < KM_B * e.frames; u += 256) {
            const int rl = u / e.frames, j = u - rl * e.frames;
            tab[u] = row0_s[rl] + ((2 * j + 1) * n_s[rl]) / (2 * e.frames);
        }
    __syncthreads();

    // 1 / norm, one wave per candidate, in segment_vectors_kernel's order
    for (int rl = wave; rl < KM_B; rl += 4) {
        const int n = n_s[rl], row0 = row0_s[rl];
        float inv = 0.0f;
        if (n > 0) {                                                  // (wave-uniform)
            double ss = 0.0;
            for (int el = lane; el < depth; el += 64) {
                const int j = el / e.D, c = el - j * e.D;
                const int sr = tab ? tab[rl * e.frames + j] : row0 + ((2 * j + 1) * n) / (2 * e.frames);
                const float v = e.table[(int64_t)sr * e.D + c];
                ss += (double)v * (double)v;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
            inv = ss > 0.0 ? (float)(1.0 / sqrt(ss)) : 0.0f;
            // all zero, a NaN (ss is NaN), an infinity (inv = 0 against an infinite value), or a norm so small that inv
            // overflows: exactly the candidates whose vector abn_kmeans_assign would call BAD or keep = 0 leaves out
            if (!(ss > 0.0) || !__builtin_isfinite(ss) || !__builtin_isfinite(inv)) {
                inv = 0.0f;
                if (lane == 0) n_s[rl] = 0;
            }
        }
        if (lane == 0) inv_s[rl] = inv;
    }
    __syncthreads();

    const EskCandRows rows{e, depth, row0_s, n_s, inv_s, tab};
    const int row = t & (KM_B - 1), half = t >> 7;
    float bs;
    int bi;
    km_sweep_argmax(rows, p, smem, red_s, red_i, bs, bi);
    if (!half && c0 + row < e.n_cand) {
        const bool bad = n_s[row] <= 0;
        e.cand_id[c0 + row] = bad ? -1 : bi;
        e.cand_best[c0 + row] = bad ? NAN : bs;
    }
}

struct EskSegP {
    const float* cand_best; const int* cand_id;
    const int64_t* lm; const int64_t* lm_off;
    int n_utt; int64_t n_lm; int S;
    uint8_t* cut; int* word; int* span; double* objective; int* n_seg;
};

// One wavefront per utterance (see the head of the file).  `span` holds the back-pointers between the forward pass and
// the traceback (span[lo + j] = the span of the best segment ENDING at j), `word` the chosen spans between the traceback
// and the last pass; both are this wave's own rows, written and read on one CU with a barrier between.
__global__ __launch_bounds__(64) void esk_segment_kernel(EskSegP p)
{
    __shared__ float cost_s[64][ESK_MAX_SPAN + 1];
    __shared__ int bp_s[64];
    const int lane = threadIdx.x, u = (int)blockIdx.x, S = p.S;
    const int64_t lo = p.lm_off[u], hi = p.lm_off[u + 1];
    if (lo < 0 || hi > p.n_lm || hi - lo < 2 || hi - lo > INT_MAX) {   // (uniform) not an utterance: nothing is touched
        if (lane == 0) {
            if (p.objective) p.objective[u] = NAN;
            if (p.n_seg) p.n_seg[u] = -1;
        }
        return;
    }
    const int L = (int)(hi - lo) - 1;
    for (int j = lane; j <= L; j += 64) { p.cut[lo + j] = 0; p.word[lo + j] = -1; p.span[lo + j] = -1; }

    float gm[ESK_MAX_SPAN];                                           // lane 0: gamma[j - 1 - i]
#pragma unroll
    for (int i = 0; i < ESK_MAX_SPAN; ++i) gm[i] = INFINITY;
    gm[0] = 0.0f;
    for (int j0 = 1; j0 <= L; j0 += 64) {
        const int j = j0 + lane, cnt = min(64, L - j0 + 1);
        if (j <= L) {
            const int64_t end = p.lm[lo + j];
            for (int s = 1; s <= S; ++s) {
                float c = INFINITY;
                if (j - s >= 0) {
                    const int64_t at = (lo + j - s) * S + s - 1;
                    const int id = p.cand_id[at];
                    const float best = p.cand_best[at];
                    const float n = (float)(end - p.lm[lo + j - s]);
                    if (id >= 0) c = n * (1.0f - 2.0f * best);
                }
                cost_s[lane][s - 1] = c;
            }
        }
        __syncthreads();
        if (lane == 0) {
            for (int i = 0; i < cnt; ++i) {
                float g = INFINITY;
                int bp = 0;
#pragma unroll
                for (int s = 1; s <= ESK_MAX_SPAN; ++s) {
                    if (s <= S) {
                        const float v = gm[s - 1] + cost_s[i][s - 1];
                        if (v < g) { g = v; bp = s; }                 // strict: equal sums go to the smallest s
                    }
                }
#pragma unroll
                for (int q = ESK_MAX_SPAN - 1; q > 0; --q) gm[q] = gm[q - 1];
                gm[0] = g;
                bp_s[i] = bp;
            }
        }
        __syncthreads();
        if (j <= L) p.span[lo + j] = bp_s[lane];
        __syncthreads();
    }

    int nseg = -1;
    if (lane == 0) {
        const float total = gm[0];
        if (total < INFINITY) {                                       // (false for NaN too)
            nseg = 0;
            int j = L;
            p.cut[lo + L] = 1;
            while (j > 0) {
                const int s = p.span[lo + j];
                if (s < 1 || s > j) { nseg = -1; break; }             // (cannot happen on a finite total)
                j -= s;
                p.word[lo + j] = s;
                p.cut[lo + j] = 1;
                ++nseg;
            }
        }
        if (p.objective) p.objective[u] = nseg >= 0 ? (double)total : (double)NAN;
        if (p.n_seg) p.n_seg[u] = nseg;
    }
    nseg = __shfl(nseg, 0, 64);
    __syncthreads();
    for (int j = lane; j <= L; j += 64) {
        const int s = nseg >= 0 ? p.word[lo + j] : -1;
        p.span[lo + j] = s >= 1 ? s : -1;
        p.word[lo + j] = s >= 1 ? p.cand_id[(lo + j) * S + s - 1] : -1;
        if (nseg < 0) p.cut[lo + j] = 0;
    }
}

}  // namespace abn

using namespace abn;

extern "C" int64_t abn_esk_max_span(void) { return ESK_MAX_SPAN; }

extern "C" int abn_esk_score(const float* table, int64_t T, int64_t D, const int64_t* lm, const int64_t* lm_off, int64_t n_utt,
                             int64_t n_lm, int frames, int S, int64_t max_frames, const float* m, const float* b, int64_t K,
                             float* cand_best, int32_t* cand_id, void* stream)
{
    ABN_REQUIRE(T >= 1 && T < (1LL << 31) - KM_B, "abn_esk_score: T = %lld out of range", (long long)T);
    ABN_REQUIRE(D >= 1 && frames >= 1 && K >= 1 && S >= 1, "abn_esk_score: D = %lld, frames = %d, K = %lld, S = %d out of range",
                (long long)D, frames, (long long)K, S);
    ABN_REQUIRE(n_utt >= 1 && n_utt < (1LL << 31) && n_lm >= 2 && max_frames >= 1,
                "abn_esk_score: n_utt = %lld, n_lm = %lld, max_frames = %lld out of range", (long long)n_utt, (long long)n_lm,
                (long long)max_frames);
    if (S > ESK_MAX_SPAN || D > KM_MAX_D || frames > KM_MAX_D || (int64_t)frames * D > KM_MAX_D || K > KM_MAX_K) {
        set_error("abn_esk_score: S = %d, frames x D = %d x %lld, K = %lld, supported S <= %d (abn_esk_max_span), frames D <= %d "
                  "(abn_kmeans_max_d), K <= %d (abn_kmeans_max_k)", S, frames, (long long)D, (long long)K, ESK_MAX_SPAN, KM_MAX_D,
                  KM_MAX_K);
        return ABN_E_UNSUPPORTED;
    }
    ABN_REQUIRE(n_lm <= ((1LL << 31) - KM_B) / S, "abn_esk_score: n_lm = %lld x S = %d candidates out of range", (long long)n_lm, S);
    ABN_REQUIRE(table && lm && lm_off && m && b && cand_best && cand_id, "abn_esk_score: null pointer");
    static bool attr_set[16] = {};
    if (first_use_on_device(attr_set))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(esk_score_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(KM_TILE_BYTES + sizeof(int) * KM_B * ESK_TAB_FRAMES));
    const size_t lds = KM_TILE_BYTES + (frames <= ESK_TAB_FRAMES ? sizeof(int) * KM_B * (size_t)frames : 0);
    EskP e;
    e.table = table; e.T = (int)T; e.D = (int)D;
    e.lm = lm; e.lm_off = lm_off; e.n_utt = (int)n_utt; e.n_lm = n_lm;
    e.frames = frames; e.S = S; e.max_frames = max_frames;
    e.cand_best = cand_best; e.cand_id = cand_id; e.n_cand = n_lm * S;
    KmP p;
    p.x = nullptr; p.shift = nullptr; p.m = m; p.b = b;
    p.T = 0; p.K = (int)K; p.D = frames * (int)D;
    p.ids = nullptr; p.prev = nullptr; p.best = nullptr; p.changed = nullptr;
    p.tiles_k = (int)((K + KM_B - 1) / KM_B);
    hipLaunchKernelGGL(esk_score_kernel, dim3((unsigned)((e.n_cand + KM_B - 1) / KM_B)), dim3(256), lds,
                       static_cast<hipStream_t>(stream), e, p);
    ABN_CHECK_LAUNCH("abn_esk_score");
    return ABN_OK;
}

extern "C" int abn_esk_segment(const float* cand_best, const int32_t* cand_id, const int64_t* lm, const int64_t* lm_off,
                               int64_t n_utt, int64_t n_lm, int S, uint8_t* cut, int32_t* word, int32_t* span, double* objective,
                               int32_t* n_seg, void* stream)
{
    ABN_REQUIRE(n_utt >= 1 && n_utt < (1LL << 31) && n_lm >= 2 && S >= 1, "abn_esk_segment: n_utt = %lld, n_lm = %lld, S = %d out of range",
                (long long)n_utt, (long long)n_lm, S);
    if (S > ESK_MAX_SPAN) {
        set_error("abn_esk_segment: S = %d, supported S <= %d (abn_esk_max_span)", S, ESK_MAX_SPAN);
        return ABN_E_UNSUPPORTED;
    }
    ABN_REQUIRE(n_lm <= ((1LL << 31) - KM_B) / S, "abn_esk_segment: n_lm = %lld x S = %d candidates out of range", (long long)n_lm, S);
    ABN_REQUIRE(cand_best && cand_id && lm && lm_off && cut && word && span, "abn_esk_segment: null pointer");
    EskSegP p;
    p.cand_best = cand_best; p.cand_id = cand_id; p.lm = lm; p.lm_off = lm_off;
    p.n_utt = (int)n_utt; p.n_lm = n_lm; p.S = S;
    p.cut = cut; p.word = word; p.span = span; p.objective = objective; p.n_seg = n_seg;
    hipLaunchKernelGGL(esk_segment_kernel, dim3((unsigned)n_utt), dim3(64), 0, static_cast<hipStream_t>(stream), p);
    ABN_CHECK_LAUNCH("abn_esk_segment");
    return ABN_OK;
}
