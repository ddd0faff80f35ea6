// hmm_dense.h -- the shared layer of the persistent kernels of the HMM with a full transition matrix: device and host for
// hmm_dense_kernel (hmm_dense.hip: abny_hmm_dense_forward_backward), hmm_dense_vit_kernel and hmm_dense_dur_kernel
// (hmm_dense_vit.hip: abnz_hmm_dense_viterbi, abnw_hmm_dense_viterbi_dur), host only for hmm_hsmm_kernel (hmm_hsmm.hip:
// abnu_hmm_hsmm_viterbi).  A phase that these kernels share without a measured cost is written here once, as a
// __forceinline__ function over the caller's own LDS arrays; a kernel's file holds what is its own.  (Their score-only
// GmmP is gmm_tile.h's hmm_score_params; hmm_dense_kernel's sum reductions are fixed_sum.h's, shared with hmm.hip.)
//
// The launch shape they share: one launch for the corpus, persistent workgroups of 256 threads that loop over the
// utterances (u = blockIdx.x, + gridDim.x, ...: a static assignment), an utterance in blocks of 128 frames.  A block starts
// with hd_logn_block: the BAD flags and the 128 x K raw scores logN from the mixture's fp32 MFMA tile (gmm_tile.h, c0 as
// the third table) into the slab at the head of the workgroup's region of the workspace.  A [KC][KC + 1] fp32 matrix
// (hd_load_matrix) lives in LDS for the whole launch behind the score tile's operands, KC the capacity the kernel is
// instantiated with (16, 32, 64, 128: hd_kc_for, hd_for_kc); KC + 1 is odd, so rows and columns are both read
// conflict-free.  A step over it is a KC x KC product over 256 threads: thread t has own = t % KC and the slice sl = t / KC
// of SW = KC^2 / 256 consecutive indices of the other side, and the NS = 256 / KC partial results go through LDS and are
// combined slice 0 first.
//
// hmm_dense_vit_kernel and hmm_dense_dur_kernel (HmmDenseVitP) share more: hd_refused and hd_write_results (what an
// utterance leaves in log_prob / n_switch / n_good), hd_key_index (the lowest index of a frame's maximum, from its 64-bit
// key: vit_wave.h) and hd_write_ids (a block's ids, coalesced, behind the lane that chases the backpointers in LDS).
// What is NOT here, each beside a comment with its measurement (profiles/hmm_dense_shared_layer.md): the per-frame entry
// maximum, the workgroup key reduction and the plane copies between LDS and the region stand in each decoder's own
// text, because through shared functions each kernel measured 1 % slower at one capacity.  For the same reason
// hmm_hsmm_kernel (hmm_hsmm.hip) takes the score block alone and keeps its own flat parameter struct; its entry uses the
// host side.
//
// Host side: hd_launch (the opt-in to the LDS and the launch of one instantiation), hd_for_kc (the capacity list) and
// hd_decode_setup, the decoders' entry prologue.  Workspace geometry and size checks are utt_chain.h's.
#pragma once
#include "common.h"
#include "gemm_f32.h"
#include "gmm_tile.h"
#include "utt_chain.h"
#include "vit_wave.h"

#include <math.h>
#include <type_traits>

namespace abn {

static_assert(GM_B == UC_B, "utt_chain.h's geometry is these kernels'");
constexpr int HD_MAX_K = 128;
constexpr ChainLimits HD_LIMITS = {GM_MAX_D, "abn_gmm_max_d", HD_MAX_K, "abny_hmm_dense_max_k", "abn_hmm_max_len"};
constexpr size_t hd_trans_bytes(int kc) { return sizeof(float) * kc * (kc + 1); }
constexpr size_t hd_lds_bytes(int kc) { return GM_TILE_BYTES + hd_trans_bytes(kc); }
// 72 KiB of operand tiles + 64.5 KiB of transitions + under 8 KiB of static arrays, of the CU's 160 KiB
static_assert(hd_lds_bytes(HD_MAX_K) + 8 * 1024 <= 160 * 1024, "the transition matrix fits beside the operand tiles");

static inline int hd_kc_for(int64_t K) { return K <= 16 ? 16 : K <= 32 ? 32 : K <= 64 ? 64 : 128; }

// What the two kernels of hmm_dense_vit.hip take, and what hd_decode_setup fills for every decoder entry: li and lt are the
// entry's initial and transition tables (abnu_hmm_hsmm_viterbi: li and lx, copied into its own HsmmP).
struct HmmDenseVitP {
    GmmP g;                                 // x, shift, A, B, c = c0, T, K, D, tiles_k: a kernel argument, as in hmm.hip
    const float* li; const float* lt;
    const int64_t* off; const int* len;
    int n_utt;
    int* ids; double* log_prob; int* n_switch; int* n_good;
    char* ws; int64_t per_wg;               // bytes of a workgroup's region
    int ks, cap;                            // slab row stride (floats), frames the region holds
};

// ---- device: the three kernels ---------------------------------------------------------------------------------------------

// The block of frames m0 .. m0 + nf - 1: BAD flags and the score tile logN into the slab (hmm_vit_scores of hmm.hip with
// one tile of components).  Ends behind a barrier.
__device__ __forceinline__ void hd_logn_block(const GmmP& gp, int m0, int nf, float* smem, float* slab, int ks, int* bad_s)
{
    float* const As = smem;
    float* const Bs = smem + 2 * GmTile::floats;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    if (t < GM_B) {
        bool bad = false;
        if (t < nf)
            for (int d = 0; d < gp.D; ++d) {
                const float xc = gp.x[(int64_t)(m0 + t) * gp.D + d] - gp.shift[d];
                bad |= !__builtin_isfinite(xc * xc);
            }
        bad_s[t] = bad;
    }
    {
        f32x16 acc[2][2];                                             // (K <= 128: one tile of components)
        gmm_score_tile(gp, m0, 0, As, Bs, acc);
        const int col_l = lane & 31, rsub = 4 * (lane >> 5);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    slab[(int64_t)(wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + rsub) * ks + wn0 + 32 * j + col_l] = acc[i][j][r];
    }
    __syncthreads();                                                  // the slab and bad_s are this workgroup's own
}

// dst [KC][KC + 1] in LDS from src [K][K]: `fill` outside K x K and, with mask_diagonal, on the diagonal.  No barrier.
template <int KC>
__device__ __forceinline__ void hd_load_matrix(float* dst, const float* src, int K, float fill, bool mask_diagonal)
{
    constexpr int TS = KC + 1;
    for (int i = threadIdx.x; i < KC * TS; i += 256) {
        const int j = i / TS, k = i % TS;
        dst[i] = (j < K && k < K && !(mask_diagonal && j == k)) ? src[j * K + k] : fill;
    }
}

// (uniform) whether utterance (o, L) lies outside the T frames or the region's cap: nothing of it is touched then.
__device__ __forceinline__ bool hd_out_of_range(int64_t o, int L, int T, int cap) { return o < 0 || L < 0 || o + L > T || L > cap; }

// ---- device: hmm_dense_vit_kernel and hmm_dense_dur_kernel -----------------------------------------------------------------

// (uniform) a refused utterance gets NaN / -1 / -1 from thread 0.
__device__ __forceinline__ bool hd_refused(const HmmDenseVitP& p, int u, int64_t o, int L)
{
    if (!hd_out_of_range(o, L, p.g.T, p.cap)) return false;
    if (threadIdx.x == 0) {
        if (p.log_prob) p.log_prob[u] = NAN;
        if (p.n_switch) p.n_switch[u] = -1;
        if (p.n_good) p.n_good[u] = -1;
    }
    return true;
}

// The lowest index of a frame's maximum, from the workgroup's key (vit_wave.h's vit_key).
__device__ __forceinline__ int hd_key_index(unsigned long long key, int K)
{
    const int bi = (int)~(unsigned)key;
    return (unsigned)bi >= (unsigned)K ? 0 : bi;                      // no score compared greater than -inf: still an id
}

// A block's ids, which the chasing lane left in ids_s, coalesced.  Starts with the barrier behind that lane.
__device__ __forceinline__ void hd_write_ids(int* ids, int64_t o, int f0, int nf, const int* ids_s)
{
    __syncthreads();
    if ((int)threadIdx.x < nf) ids[o + f0 + threadIdx.x] = ids_s[threadIdx.x];
}

// The utterance's results from thread 0.  Ends behind a barrier: the traceback's reads before the next utterance's writes.
__device__ __forceinline__ void hd_write_results(const HmmDenseVitP& p, int u, double lp, int nsw, int ngood)
{
    if (threadIdx.x == 0) {
        if (p.log_prob) p.log_prob[u] = lp;
        if (p.n_switch) p.n_switch[u] = nsw;
        if (p.n_good) p.n_good[u] = ngood;
    }
    __syncthreads();
}

// ---- host ------------------------------------------------------------------------------------------------------------------

// A decoder region's bytes per frame: `planes` bytes per unit of the capacity K rounds up to, and one for the BAD flag.
static inline int64_t hd_frame_bytes(int64_t K, int planes, bool bad_byte)
{
    return planes * (K >= 1 && K <= HD_MAX_K ? hd_kc_for(K) : HD_MAX_K) + (bad_byte ? 1 : 0);
}

// f(std::integral_constant<int, KC>) for the capacity kc (hd_kc_for), in the manner of for_each_nq.
template <class F>
static inline void hd_for_kc(int kc, F&& f)
{
    if (kc == 16) f(std::integral_constant<int, 16>{});
    else if (kc == 32) f(std::integral_constant<int, 32>{});
    else if (kc == 64) f(std::integral_constant<int, 64>{});
    else f(std::integral_constant<int, 128>{});
}

// The launch of one instantiation, with its opt-in to hd_lds_bytes(KC) at its first use on a device.
template <auto KERNEL, int KC, class P>
static void hd_launch(const P& p, int grid, hipStream_t st)
{
    static bool attr_set[16] = {};
    if (first_use_on_device(attr_set)) chain_opt_in(reinterpret_cast<const void*>(KERNEL), hd_lds_bytes(KC));
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(256), hd_lds_bytes(KC), st, p);
}

// A decoder entry's prologue: the checks in their order -- own_check() is the entry's own (extra pointers, min_duration, L),
// behind the pointers as in abnx_hmm_viterbi_dur --, the caller's workspace split into regions of frame_bytes a frame, and
// the kernel's arguments.
template <class F>
static int hd_decode_setup(const char* what, const char* ws_fn, F&& own_check, int64_t frame_bytes,
                           const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                           const float* shift, const float* A, const float* B, const float* c0, const float* li, const float* lt, int64_t K,
                           int32_t* ids, double* log_prob, int32_t* n_switch, int32_t* n_good, void* ws, int64_t ws_bytes,
                           HmmDenseVitP* p, int* grid)
{
    ABN_REQUIRE(T >= 1 && T < (1LL << 31) - GM_B, "%s: T = %lld out of range", what, (long long)T);
    int rc = chain_check_sizes(what, n_utt, K, D, HD_LIMITS);
    if (rc != ABN_OK) return rc;
    ABN_REQUIRE(x && off && len && shift && A && B && c0 && li && lt && ids, "%s: null pointer", what);
    rc = own_check();
    if (rc != ABN_OK) return rc;
    const ChainWs hw = chain_ws(n_utt, 0, K, frame_bytes, 0);
    ChainRegion a;
    rc = chain_region(what, ws_fn, ws, ws_bytes, hw, &a);
    if (rc != ABN_OK) return rc;
    p->g = hmm_score_params(x, T, D, shift, A, B, c0, K);     // (K <= 128: one tile of components)
    p->li = li; p->lt = lt; p->off = off; p->len = len; p->n_utt = (int)n_utt;
    p->ids = ids; p->log_prob = log_prob; p->n_switch = n_switch; p->n_good = n_good;
    p->ws = a.ws; p->per_wg = a.per_wg;
    p->ks = a.ks; p->cap = a.cap;
    *grid = hw.grid;
    return ABN_OK;
}

}  // namespace abn
