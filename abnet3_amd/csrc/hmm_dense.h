// hmm_dense.h -- what the three kernels of the HMM with a full transition matrix share: hmm_dense_kernel (hmm_dense.hip:
// abny_hmm_dense_forward_backward), hmm_dense_vit_kernel and hmm_dense_dur_kernel (hmm_dense_vit.hip:
// abnz_hmm_dense_viterbi, abnw_hmm_dense_viterbi_dur).  All keep a [KC][KC + 1] fp32 matrix in LDS behind the score tile's
// operands, KC the capacity the kernel is instantiated with.  (Their score-only GmmP is gmm_tile.h's hmm_score_params;
// hmm_dense_kernel's sum reductions are fixed_sum.h's, shared with hmm.hip.)
#pragma once
#include "common.h"
#include "gmm_tile.h"
#include "utt_chain.h"

namespace abn {

static_assert(GM_B == UC_B, "utt_chain.h's geometry is these kernels'");
constexpr int HD_MAX_K = 128;
constexpr ChainLimits HD_LIMITS = {GM_MAX_D, "abn_gmm_max_d", HD_MAX_K, "abny_hmm_dense_max_k", "abn_hmm_max_len"};
constexpr size_t hd_trans_bytes(int kc) { return sizeof(float) * kc * (kc + 1); }
constexpr size_t hd_lds_bytes(int kc) { return GM_TILE_BYTES + hd_trans_bytes(kc); }
// 72 KiB of operand tiles + 64.5 KiB of transitions + under 8 KiB of static arrays, of the CU's 160 KiB
static_assert(hd_lds_bytes(HD_MAX_K) + 8 * 1024 <= 160 * 1024, "the transition matrix fits beside the operand tiles");

static inline int hd_kc_for(int64_t K) { return K <= 16 ? 16 : K <= 32 ? 32 : K <= 64 ? 64 : 128; }

}  // namespace abn
