// utt_chain.h -- the host side of the per-utterance chain kernels, written once: km_viterbi_kernel (kmeans.hip:
// abn_kmeans_viterbi), hmm_viterbi_kernel and hmm_fb_kernel (hmm.hip: abn_hmm_viterbi, abn_hmm_forward_backward[_stats]),
// hmm_dense_kernel (hmm_dense.hip: abny_hmm_dense_forward_backward), hmm_dense_vit_kernel and hmm_dense_dur_kernel
// (hmm_dense_vit.hip: abnz_hmm_dense_viterbi, abnw_hmm_dense_viterbi_dur).
// All of them launch min(n_utt, 256) persistent workgroups that loop over the utterances and give each workgroup a
// 256-byte aligned region of the workspace: a slab [128][ks] of scores, then so many bytes per frame of the longest
// utterance, then a tail.  Here: that geometry (chain_ws), its split of a caller's workspace (chain_region), the size
// checks with the callers' limits in their messages (chain_check_sizes, chain_ws_bytes), the NQ list (nq_for,
// for_each_nq) and the launch of a sticky max-product kernel (vit_launch; km_viterbi_dur_kernel and
// hmm_viterbi_dur_kernel, the two with a minimum unit duration, go through vit_dur_launch with one kernel set per
// register capacity and the same workspace geometry).  The kernels themselves stay in their files: shared
// device code (one slab phase, one max-product kernel over a model type) gave the same bits but measured 5 to 11 %
// slower for hmm_fb_kernel and km_viterbi_kernel (profiles/hmm_*_time_shared_chain.json).
// Nor is a small helper free once it takes a kernel's LDS arrays: moving only the wave-key reduction that the two kernels
// of hmm_dense_vit.hip share into a __forceinline__ function with red_k[par] as a pointer changed about 29 000 of the
// translation unit's 65 000 lines of gfx950 assembly.  What takes and returns values (fixed_sum.h) moved byte for byte.
#pragma once
#include "common.h"

#include <type_traits>

namespace abn {

constexpr int UC_B = 128;                  // frames per block = the edge of both score tiles (KM_B, GM_B)
constexpr int UC_GRID = 256;               // one workgroup per CU (the score tile keeps the register file to itself)
constexpr int UC_MAX_LEN = 1 << 20;

// State k = 256 q + thread, q < NQ: the power of two that covers K.
static inline int nq_for(int64_t K)
{
    int nq = 1;
    while (nq * 256 < K) nq <<= 1;
    return nq;
}
// f(std::integral_constant<int, NQ>) for every NQ a kernel is instantiated with: the opt-in calls it for all of them, a
// launch compares each with nq_for(K).
template <class F>
static inline void for_each_nq(F&& f)
{
    f(std::integral_constant<int, 1>{});
    f(std::integral_constant<int, 2>{});
    f(std::integral_constant<int, 4>{});
    f(std::integral_constant<int, 8>{});
    f(std::integral_constant<int, 16>{});
}
static inline void chain_opt_in(const void* kernel, size_t bytes)
{
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// The workspace of a launch: per workgroup the slab [128][ks], per_frame bytes for each of max_len frames and `tail`
// bytes, rounded up to 256.  The max-product kernels keep the stay words and prevj per frame (vit_frame_bytes).
struct ChainWs { int64_t slab_bytes, per_frame, tail, per_wg; int grid, ks, kw; };
static inline int64_t vit_frame_bytes(int64_t K) { return 8LL * 4 * nq_for(K) + 4; }
static inline ChainWs chain_ws(int64_t n_utt, int64_t max_len, int64_t K, int64_t per_frame, int64_t tail)
{
    ChainWs w;
    w.grid = (int)(n_utt < UC_GRID ? n_utt : UC_GRID);
    w.ks = (int)((K + UC_B - 1) / UC_B) * UC_B;
    w.kw = 4 * nq_for(K);
    w.slab_bytes = (int64_t)sizeof(float) * UC_B * w.ks;
    w.per_frame = per_frame;
    w.tail = tail;
    w.per_wg = align_up(w.slab_bytes + max_len * per_frame + tail, 256);
    return w;
}

// The limits of an entry and the functions that report them, for the messages.
struct ChainLimits { int max_d; const char* max_d_fn; int max_k; const char* max_k_fn; const char* max_len_fn; };

static inline int chain_check_sizes(const char* what, int64_t n_utt, int64_t K, int64_t D, const ChainLimits& lim)
{
    ABN_REQUIRE(n_utt >= 1 && n_utt < (1LL << 31), "%s: n_utt = %lld out of range", what, (long long)n_utt);
    ABN_REQUIRE(K >= 1 && D >= 1, "%s: K = %lld, D = %lld out of range", what, (long long)K, (long long)D);
    if (D > lim.max_d || K > lim.max_k) {
        set_error("%s: D = %lld, K = %lld, supported D <= %d (%s), K <= %d (%s)", what, (long long)D, (long long)K, lim.max_d,
                  lim.max_d_fn, lim.max_k, lim.max_k_fn);
        return ABN_E_UNSUPPORTED;
    }
    return ABN_OK;
}

// What a *_ws_bytes entry returns: the bytes of the whole grid, or -1 with the error set.
static inline int64_t chain_ws_bytes(const char* what, int64_t n_utt, int64_t max_len, int64_t K, int64_t D,
                                     const ChainLimits& lim, int64_t per_frame, int64_t tail)
{
    if (chain_check_sizes(what, n_utt, K, D, lim) != ABN_OK) return -1;
    if (max_len < 0 || max_len > UC_MAX_LEN) {
        set_error("%s: max_len = %lld, supported 0 .. %d (%s)", what, (long long)max_len, UC_MAX_LEN, lim.max_len_fn);
        return -1;
    }
    const ChainWs w = chain_ws(n_utt, max_len, K, per_frame, tail);
    return w.per_wg * w.grid;
}

// A caller's workspace split into the grid's regions, or the refusal of a workspace that holds no frame.  ws_fn names
// the sizing entry in the message.
struct ChainRegion {
    char* ws; int64_t per_wg;               // bytes of a workgroup's region
    int ks, kw, cap;                        // slab row stride (floats), stay words per frame, frames the region holds
};
static inline int chain_region(const char* what, const char* ws_fn, void* ws, int64_t ws_bytes, const ChainWs& w, ChainRegion* a)
{
    const int64_t per_wg = ws_bytes > 0 ? (ws_bytes / w.grid) & ~255LL : 0;
    int64_t cap = (per_wg - w.slab_bytes - w.tail) / w.per_frame;
    if (!ws || cap < 1) {
        set_error("%s: workspace of %lld bytes holds no frame (%s)", what, (long long)ws_bytes, ws_fn);
        return ABN_E_WORKSPACE;
    }
    ABN_REQUIRE(aligned16(ws), "%s: the workspace must be 16-byte aligned", what);
    if (cap > UC_MAX_LEN) cap = UC_MAX_LEN;
    a->ws = static_cast<char*>(ws); a->per_wg = per_wg;
    a->ks = w.ks; a->kw = w.kw; a->cap = (int)cap;
    return ABN_OK;
}

// The launch of a max-product kernel template over w.grid workgroups: KS::template kernel<NQ, LDSS>() names its
// instantiations; the one with the slab in LDS (lds_bytes) where K <= 128, otherwise the one whose NQ covers K.
template <class KS, class P>
static int vit_launch(const char* what, const P& p, int64_t K, const ChainWs& w, size_t tile_bytes, size_t lds_bytes, void* stream)
{
    static bool attr_set[16] = {};
    if (first_use_on_device(attr_set)) {
        chain_opt_in(reinterpret_cast<const void*>(KS::template kernel<1, true>()), lds_bytes);
        for_each_nq([&](auto n) {
            constexpr int NQ = decltype(n)::value;
            chain_opt_in(reinterpret_cast<const void*>(KS::template kernel<NQ, false>()), tile_bytes);
        });
    }
    const dim3 grid((unsigned)w.grid);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (K <= UC_B) hipLaunchKernelGGL((KS::template kernel<1, true>()), grid, dim3(256), lds_bytes, st, p);
    else {
        const int nq = nq_for(K);
        for_each_nq([&](auto n) {
            constexpr int NQ = decltype(n)::value;
            if (NQ == nq) hipLaunchKernelGGL((KS::template kernel<NQ, false>()), grid, dim3(256), tile_bytes, st, p);
        });
    }
    ABN_CHECK_LAUNCH(what);
    return ABN_OK;
}

// The same for a minimum duration S: KSD<SC> is the kernel set of register capacity SC, the smallest of 1, 2, 4, 8 that
// holds S.
template <template <int> class KSD, class P>
static int vit_dur_launch(const char* what, const P& p, int S, int64_t K, const ChainWs& w, size_t tile_bytes, size_t lds_bytes,
                          void* stream)
{
    if (S == 1) return vit_launch<KSD<1>>(what, p, K, w, tile_bytes, lds_bytes, stream);
    if (S == 2) return vit_launch<KSD<2>>(what, p, K, w, tile_bytes, lds_bytes, stream);
    if (S <= 4) return vit_launch<KSD<4>>(what, p, K, w, tile_bytes, lds_bytes, stream);
    return vit_launch<KSD<8>>(what, p, K, w, tile_bytes, lds_bytes, stream);
}

}  // namespace abn
