/* abnet3_hip_next.h -- entries of libabnet3_hip.so that are not part of the numbered ABI yet.
 *
 * The entries below carry the prefix abnx_ (the minimum unit duration of the max-product decoders), abny_ (the HMM with
 * a full transition matrix), abnz_ (that model's max-product path), abnw_ (that path with a minimum unit duration) or abnv_
 * (the hard statistics of that model's Viterbi training) or abnu_ (explicit unit durations: the semi-Markov decoder and its
 * run statistics, ledger abnet3_amd._lib.NEXT6_SYMBOLS with tests/test_gpu_hmm_hsmm.py) or abnt_ (the in-batch contrastive
 * pair loss, ledger abnet3_amd._lib.NEXT7_SYMBOLS with tests/test_gpu_nce.py) or abns_ (the pair-free histogram of
 * within-cluster edit distances behind the full term scores, ledger abnet3_amd._lib.EVAL_SYMBOLS with
 * tests/test_tde_full_host.py and tests/test_gpu_tde_full_contract.py -- a ledger of its own, not a NEXT<n>_SYMBOLS: the
 * main argument-contract ledger enumerates those by name and demands a row in tests/test_gpu_arg_contract.py for each of
 * their entries; folding this section into that ledger is for a change that may edit those files) or abnr_ (the
 * reconstruction loss of the correspondence autoencoder, ledger abnet3_amd._lib.CAE_SYMBOLS with tests/test_cae_host.py and
 * tests/test_gpu_cae_contract.py -- a ledger of its own for the same reason) or abnq_ (batched soft-DTW over cosine cells and
 * its gradient, ledger abnet3_amd._lib.SDTW_SYMBOLS with tests/test_sdtw_host.py and tests/test_gpu_sdtw_contract.py -- a
 * ledger of its own for the same reason) and are
 * exported beside those of abnet3_hip.h, whose conventions they follow (extern "C", plain pointers and sizes, the ABN_E_*
 * return codes, abn_last_error, every refusal before any launch).
 * They do not change ABN_ABI_VERSION.  A later change folds them into abnet3_hip.h under their abn_ names, bumps the
 * version, and moves their ledgers (abnet3_amd._lib.NEXT_SYMBOLS with tests/test_gpu_vit_dur.py, abnet3_amd._lib.NEXT2_SYMBOLS
 * with tests/test_gpu_hmm_dense.py, abnet3_amd._lib.NEXT3_SYMBOLS with tests/test_gpu_hmm_dense_vit.py,
 * abnet3_amd._lib.NEXT4_SYMBOLS with tests/test_gpu_hmm_dense_dur.py, abnet3_amd._lib.NEXT5_SYMBOLS with
 * tests/test_gpu_hmm_hard.py) into the main one
 * (abnet3_amd._lib.SYMBOLS, tests/test_dirty_memory_host.py).
 */
#ifndef ABNET3_HIP_NEXT_H
#define ABNET3_HIP_NEXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Minimum unit duration for the two max-product decoders (csrc/kmeans.hip, csrc/hmm.hip, csrc/vit_wave.h) ----------
 * abn_kmeans_viterbi and abn_hmm_viterbi with one more argument: min_duration = S, 1 .. abnx_viterbi_dur_max() (8).
 * Every unit k becomes a left-to-right chain of S states with tied emissions of which only the last may repeat, so every
 * segment of a path but the utterance's last is at least S good frames long (the end of the utterance may cut the last
 * one short).  One utterance, good frames only (BAD frames get id -1 and are passed over; durations count good frames):
 * a path is a sequence of segments (k_i, n_i) and its score is
 *     sum of the frames' scores s[t, k] + lw[k_1] + lr[k_i] for each later segment + max(n_i - S, 0) ls[k_i]
 * with lw, ls, lr the caller's tables (abnx_hmm_viterbi_dur) or lw = 0, ls = 0, lr = -penalty_score
 * (abnx_kmeans_viterbi_dur).  Recurrence, fp32, every operation one rounded add or a compare; V[k][0 .. S-1] the
 * normalised previous values, E = max_k V[k][S-1] and exitj the lowest k whose U[k][S-1] was the largest (0 if all -inf):
 *     first good frame:  U[k][0] = s + lw[k], every other state -inf
 *     later good frames: U[k][0] = s + (E + lr[k]);   U[k][i] = s + V[k][i-1] for 0 < i < S-1;
 *                        a = V[k][S-1] + ls[k],  st = a > V[k][S-2] (strict; S = 1: a > E + lr[k]),
 *                        U[k][S-1] = s + (st ? a : V[k][S-2])
 *     every good frame:  N_t = max U,  V = U - N_t,  log_prob / objective = the float64 sum of the N_t in frame order.
 * The final state is the lowest k, then the largest i, with V[k][i] == 0; the traceback reads one stay bit per
 * (frame, unit) and the previous good frame's exitj per frame.  With min_duration = 1 the outputs are those of
 * abn_kmeans_viterbi / abn_hmm_viterbi bit for bit.
 *
 * Arguments, outputs, limits and the treatment of refused utterances are the twins' (abnet3_hip.h).  The workspace has the
 * twins' geometry: size it with abn_kmeans_viterbi_ws_bytes / abn_hmm_viterbi_ws_bytes.  Refusals are the twins', in the
 * twins' order; min_duration outside 1 .. abnx_viterbi_dur_max(): ABN_E_ARG -- all before any launch. */
int32_t abnx_viterbi_dur_max(void);        /* host */
int abnx_kmeans_viterbi_dur(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                            const float* shift, const float* m, const float* b, int64_t K, float penalty_score,
                            int32_t* ids, double* objective, int32_t* n_switch, void* ws, int64_t ws_bytes,
                            void* stream, int32_t min_duration);
int abnx_hmm_viterbi_dur(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                         const float* shift, const float* A, const float* B, const float* c0,
                         const float* lw, const float* ls, const float* lr, int64_t K,
                         int32_t* ids, double* log_prob, int32_t* n_switch, int32_t* n_good,
                         void* ws, int64_t ws_bytes, void* stream, int32_t min_duration);

/* ---- The HMM with a full transition matrix over a mixture's components (csrc/hmm_dense.hip) ------------------------------
 * abn_hmm_forward_backward with init [K] and trans [K][K] (row-stochastic, trans[j][k] = P(k at t | j at the previous good
 * frame)) in place of the weights and the stay; abnet3_amd/hmm.py states the recursion, tests/hmm_dense_np.py restates it.
 * x, T, D, off, len, n_utt, shift, A, B, c0, mode, post, loglik, n_good are abn_hmm_forward_backward's: the emissions are
 * its score tile's bits, BAD frames follow its rule (a zero row, passed over, counted neither as a frame nor as a
 * transition), `post` holds ahat between the sweeps, and utterances must not overlap.  The caller guarantees that every
 * entry of init and trans is at least 2^-100 (then c_t >= 2^-100 and e <= 2^100; the library does not read them on the host).
 *
 * stats: [K + 1][K] float64 or null.  Rows 0 .. K - 1 are the expected transition counts xi[j][k] = trans[j][k] G[j][k],
 * G[j][k] = the sum over the transitions (p -> t) of ahat_p[j] e_t[k]; row K is first[k] = gamma summed over the utterances'
 * first good frames.  All zero in mode 1.  Each workgroup adds its utterances' terms in utterance order into a slab of its
 * own in the workspace, and a second small launch adds the slabs in workgroup order: the same bits for the same corpus and
 * the same min(n_utt, 256).  Null: no statistics and no second launch; every other output has the same bits either way.
 *
 * K <= abny_hmm_dense_max_k() (a host query: the transition matrix, [K'][K' + 1] fp32 with K' = K rounded up to 16, 32, 64
 * or 128, lives in LDS beside the score tile's operands; at least 128), D <= abn_gmm_max_d(), an utterance of at most
 * abn_hmm_max_len() frames.  Workspace: abny_hmm_dense_ws_bytes(n_utt, max_len, K, D) bytes, 16-byte aligned, -1 with
 * abn_last_error for refused sizes (max_len beyond abn_hmm_max_len() among them); it need not be cleared.
 * Refusals, all before any launch: null pointers (stats excepted), sizes < 1 and a mode other than 0 or 1: ABN_E_ARG;
 * K or D beyond the limits: ABN_E_UNSUPPORTED; a workspace that holds no frame: ABN_E_WORKSPACE.  An utterance outside
 * 0 .. T or longer than the workspace was sized for (and so any longer than abn_hmm_max_len()) is left untouched: loglik NaN,
 * n_good -1, nothing added to stats. */
int64_t abny_hmm_dense_max_k(void);        /* host */
int64_t abny_hmm_dense_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D);      /* host */
int abny_hmm_dense_forward_backward(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                                    const float* shift, const float* A, const float* B, const float* c0,
                                    const float* init, const float* trans, int64_t K, int mode,
                                    float* post, double* loglik, int32_t* n_good, double* stats,
                                    void* ws, int64_t ws_bytes, void* stream);

/* ---- The max-product path of the HMM with a full transition matrix (csrc/hmm_dense_vit.hip) ----------------------------
 * abn_hmm_viterbi with li [K] and lt [K][K] (the float32 logarithms of init and trans, abnet3_amd.hmm.log_transitions: the
 * kernel takes no logarithm) in place of lw, ls, lr; abnet3_amd/hmm.py states the recurrence, tests/hmm_dense_vit_np.py
 * restates it.  x, T, D, off, len, n_utt, shift, A, B, c0 and the emissions (the score tile's bits), the BAD-frame rule and
 * the outputs are abn_hmm_viterbi's: ids [T] int32 (BAD frames -1, rows outside every utterance untouched), log_prob
 * [n_utt] float64, n_switch [n_utt] int32, n_good [n_utt] int32 -- the last three may be null.  One utterance, good frames
 * in order, fp32, every operation one rounded add or a compare:
 *     first good frame:  u[k] = s[k] + li[k]
 *     later good frames: c[k] = max_j (W[j] + lt[j][k]),  bp[k] = the lowest j that attains it,  u[k] = s[k] + c[k]
 *     every good frame:  M = max_k u[k],  W = u - M,  log_prob += M (a float64 sum in frame order)
 * The final state is the lowest k with W[k] == 0; backwards ids[t] = cur, cur = bp_t[cur].  The caller guarantees finite
 * tables (no NaN, no infinity).  An utterance with no good frame gives (0.0, 0, 0) and all -1.
 *
 * K <= abny_hmm_dense_max_k(), D <= abn_gmm_max_d(), an utterance of at most abn_hmm_max_len() frames.  Workspace:
 * abnz_hmm_dense_viterbi_ws_bytes(n_utt, max_len, K, D) bytes (per workgroup of min(n_utt, 256) the slab of scores and one
 * backpointer byte per frame and state of the capacity K rounds up to: 16, 32, 64 or 128), 16-byte aligned, -1 with
 * abn_last_error for refused sizes; it need not be cleared.  Refusals, all before any launch, in
 * abny_hmm_dense_forward_backward's order: T out of range, sizes < 1: ABN_E_ARG; K or D beyond the limits:
 * ABN_E_UNSUPPORTED; null pointers (the three optional outputs excepted): ABN_E_ARG; a workspace that holds no frame:
 * ABN_E_WORKSPACE; a misaligned workspace: ABN_E_ARG.  An utterance outside 0 .. T or longer than the workspace was sized
 * for is left untouched: log_prob NaN, n_switch and n_good -1. */
int64_t abnz_hmm_dense_viterbi_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D);   /* host */
int abnz_hmm_dense_viterbi(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                           const float* shift, const float* A, const float* B, const float* c0,
                           const float* li, const float* lt, int64_t K,
                           int32_t* ids, double* log_prob, int32_t* n_switch, int32_t* n_good,
                           void* ws, int64_t ws_bytes, void* stream);

/* ---- A minimum unit duration for that path (csrc/hmm_dense_vit.hip, csrc/vit_wave.h) ---------------------------------------
 * abnz_hmm_dense_viterbi with one more argument: min_duration = S, 1 .. abnx_viterbi_dur_max() (8); abnet3_amd/hmm.py
 * states the definition, tests/hmm_dense_dur_np.py restates it.  Every unit k becomes a left-to-right chain of S states with
 * tied emissions of which only the last may repeat; a unit is left only from its last state and only for a DIFFERENT unit.
 * One utterance, good frames only (BAD frames get id -1 and are passed over; durations count good frames): a path is a
 * sequence of segments (k_i, n_i), k_i != k_{i+1}, every segment but the utterance's last at least S good frames long, and
 * its score is
 *     sum of the frames' scores s[t, k] + li[k_1] + lt[k_{i-1}][k_i] for each later segment + max(n_i - S, 0) lt[k_i][k_i].
 * The maximal runs of the ids are the segments and n_switch = segments - 1.  Recurrence for S >= 2, fp32, every operation
 * one rounded add or a compare; V[k][0 .. S-1] the normalised previous values:
 *     first good frame:  U[k][0] = s + li[k], every other state -inf
 *     later good frames: ent[k] = max over j != k of (V[j][S-1] + lt[j][k]),  bp[k] = the lowest such j (strict compares in
 *                        ascending j);   U[k][0] = s + ent[k];   U[k][i] = s + V[k][i-1] for 0 < i < S-1;
 *                        a = V[k][S-1] + lt[k][k],  st = a > V[k][S-2] (strict),  U[k][S-1] = s + (st ? a : V[k][S-2])
 *     every good frame:  N_t = max U,  V = U - N_t,  log_prob = the float64 sum of the N_t in frame order.
 * The final state is the lowest k, then the largest i, with V[k][i] == 0; backwards from (k, i): i == S-1 and st set ->
 * (k, S-1); else i > 0 -> (k, i-1); else -> (bp[k], S-1), one switch.  With min_duration = 1 the entry launches
 * abnz_hmm_dense_viterbi's kernel and the outputs are that entry's bit for bit.
 *
 * Arguments, outputs, limits and the treatment of refused utterances are abnz_hmm_dense_viterbi's.  Workspace:
 * abnw_hmm_dense_viterbi_dur_ws_bytes(n_utt, max_len, K, D) bytes, the same for every S: min(n_utt, 256) regions of
 * 128 x 128 x 4 + max_len x (K' + 1) bytes rounded up to 256, K' = K rounded up to 16, 32, 64 or 128 -- the slab of
 * scores, one byte per frame and state (the backpointer in bits 0 .. 6, the stay bit in bit 7) and one byte per frame (the
 * BAD flag); 16-byte aligned, -1 with abn_last_error for refused sizes; it need not be cleared.  Refusals are
 * abnz_hmm_dense_viterbi's, in its order, with min_duration outside 1 .. abnx_viterbi_dur_max(): ABN_E_ARG behind the null
 * pointers and ahead of the workspace -- all before any launch. */
int64_t abnw_hmm_dense_viterbi_dur_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D);   /* host */
int abnw_hmm_dense_viterbi_dur(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                               const float* shift, const float* A, const float* B, const float* c0,
                               const float* li, const float* lt, int64_t K,
                               int32_t* ids, double* log_prob, int32_t* n_switch, int32_t* n_good,
                               void* ws, int64_t ws_bytes, void* stream, int32_t min_duration);

/* ---- The hard statistics of the full-transition HMM's Viterbi training (csrc/hmm_hard.hip) ------------------------------
 * From decoded unit ids (abnz_hmm_dense_viterbi, abnw_hmm_dense_viterbi_dur) the statistics of one hard-EM step;
 * abnet3_amd/hmm.py states the definition, tests/hmm_hard_np.py restates it.  x, T, D, off, len, n_utt, shift are
 * abnz_hmm_dense_viterbi's; ids [T] int32.  A frame is good if 0 <= ids[t] < K; every other id is BAD and is passed over.
 * Per utterance u let a_0 .. a_{n-1} be the ids of its good frames in frame order and S = min_duration, 1 ..
 * abnx_viterbi_dur_max():  n_good[u] = n, and
 *     counts[K][a_0] += 1 when n >= 1                                  (row K is `first`, abny_hmm_dense_forward_backward's layout)
 *     i >= 1, a_i != a_{i-1}:  counts[a_{i-1}][a_i] += 1               (a switch)
 *     i >= 1, a_i == a_{i-1}:  counts[a_i][a_i] += 1 only if i >= S and a_{i-1} = ... = a_{i-S} = a_i
 *                                                                      (a stay in the chain's last state; otherwise a forced advance)
 * -- the maximum-likelihood counts of the chain abnw_hmm_dense_viterbi_dur decodes; at S = 1 rows 0 .. K - 1 are the plain
 * bigram counts.  Durations count good frames only, nothing connects two utterances, rows outside every utterance contribute
 * nothing, utterances may lie in any order (they must not overlap).
 * sums [K][2 D + 1] float64 = [S1 | S2 | N] (abn_hmm_accumulate's layout) over the good frames of the utterances: N[k] the
 * frames with id k, S1 and S2 the sums of xc and xc^2, xc = x - shift in fp32, xc^2 rounded once; an entry whose xc^2 is not
 * finite contributes 0 to both (abn_hmm_accumulate's rule).
 *
 * counts [K + 1][K] int64 is the same for any grid, any n_ranges and any order of the utterances (integer atomics).  sums
 * uses no floating-point atomics: the frames of a range (n_ranges consecutive ranges of whole 128-row blocks of the table;
 * 0: chosen from the grid, at most 256) are added in frame order in fp32 per unit, the ranges in range order in float64 --
 * the same bits from call to call for the same inputs and n_ranges.  counts, sums, n_good and the workspace need not be
 * cleared.  Two memsets and three launches.
 *
 * K <= abny_hmm_dense_max_k(), D <= abn_gmm_max_d(), T < 2^31 - 128.  Workspace: abnv_hmm_hard_stats_ws_bytes(T, n_utt, K, D,
 * n_ranges) bytes (a copy of the good ids [T] int32 and the ranges' fp32 partials), 16-byte aligned, -1 with abn_last_error
 * for refused sizes.  Refusals, all before any launch, in this order: T out of range, sizes < 1: ABN_E_ARG; K or D beyond the
 * limits: ABN_E_UNSUPPORTED; null pointers: ABN_E_ARG; min_duration outside 1 .. abnx_viterbi_dur_max(), n_ranges outside
 * 0 .. 256: ABN_E_ARG; a short workspace: ABN_E_WORKSPACE; a misaligned one: ABN_E_ARG.  An utterance outside 0 .. T or longer
 * than abn_hmm_max_len() gets n_good -1 and adds nothing. */
int64_t abnv_hmm_hard_stats_ws_bytes(int64_t T, int64_t n_utt, int64_t K, int64_t D, int n_ranges);   /* host */
int abnv_hmm_hard_stats(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                        const float* shift, const int32_t* ids, int64_t K, int32_t min_duration, int n_ranges,
                        int64_t* counts, double* sums, int32_t* n_good, void* ws, int64_t ws_bytes, void* stream);

/* ---- Explicit unit durations: a hidden semi-Markov decoder over that model's units (csrc/hmm_hsmm.hip) -------------------
 * Prefix abnu_; ledger abnet3_amd._lib.NEXT6_SYMBOLS with tests/test_gpu_hmm_hsmm.py.  abnet3_amd/hmm.py states the
 * definition, tests/hmm_hsmm_np.py restates it.  abnz_hmm_dense_viterbi with lx [K][K] in place of lt and three more
 * arguments at the end: ld [K][L], ls [K] and L = 2 .. abnu_hmm_hsmm_max_duration() (32).  Unit k has the duration law
 *     p_k(d) = q[k][d] for d < L,   p_k(d) = q[k][L] (1 - r[k]) r[k]^(d - L) for d >= L
 * and the tables are float32 logarithms formed on the host (abnet3_amd.hmm.duration_tables, switch_log_transitions; the
 * kernel takes no logarithm, the caller guarantees finite entries):  ld[k][i-1] = log q[k][i] for i < L,
 * ld[k][L-1] = log(q[k][L] (1 - r[k])),  ls[k] = log r[k],  lx[j][k] = log(trans[j][k] / (1 - trans[j][j])) for j != k (the
 * diagonal of lx is never read), li as before.  Good frames only (BAD frames get id -1 and are passed over; durations count
 * good frames).  A path is a sequence of segments (k_i, n_i), k_i != k_{i+1}, n_i >= 1, and its score is the sum of the frames'
 * scores + li[k_1] + lx[k_{i-1}][k_i] for each later segment + log p_{k_i}(n_i) for EVERY segment, the last one included (it
 * is treated as complete).  Recurrence, fp32, every operation one rounded add or a compare; V[k][1 .. L] the normalised
 * previous values, state i = "the current segment is i frames long", state L = "L or more":
 *     first good frame:  U[k][1] = s[k] + li[k], every other state -inf
 *     later good frames: x[j] = max_i (V[j][i] + ld[j][i]),  xi[j] = the lowest i attaining it (strict, ascending i)
 *                        ent[k] = max over j != k of (x[j] + lx[j][k]),  bp[k] = the lowest such j (strict, ascending j)
 *                        U[k][1] = s[k] + ent[k];   U[k][i] = s[k] + V[k][i-1] for 1 < i < L
 *                        a = V[k][L] + ls[k],  st = a > V[k][L-1] (strict),  U[k][L] = s[k] + (st ? a : V[k][L-1])
 *     every good frame:  N_t = max U,  V = U - N_t,  log_prob += N_t (float64, frame order)
 *     after the last:    F = max (V[k][i] + ld[k][i]), final = the lowest k, then the lowest i, attaining it;  log_prob += F
 * Backwards from (k, i) at frame t: i == L and st set -> (k, L); else i > 1 -> (k, i-1); else -> (bp[k], xi[bp[k]] as recorded
 * at frame t), one switch.  Outputs, limits and the treatment of refused utterances are abnz_hmm_dense_viterbi's.
 * Workspace: abnu_hmm_hsmm_viterbi_ws_bytes(n_utt, max_len, K, D, L) bytes, the same for every L: min(n_utt, 256) regions of
 * 128 x 128 x 4 + max_len x (2 K' + 1) bytes rounded up to 256, K' = K rounded up to 16, 32, 64 or 128 (the slab, a
 * backpointer byte with the stay bit and an xi byte per frame and unit, a BAD byte per frame); 16-byte aligned, -1 with
 * abn_last_error for refused sizes; it need not be cleared.  Refusals are abnz_hmm_dense_viterbi's, in its order, with L
 * outside 2 .. abnu_hmm_hsmm_max_duration(): ABN_E_ARG behind the null pointers and ahead of the workspace.
 *
 * abnu_hmm_run_stats: from unit ids [T] int32 the statistics that train q and r.  A frame is good if 0 <= ids[t] < K, every
 * other id is passed over.  For every maximal run, over the good frames of one utterance, of unit k with length n:
 *     dur[k][min(n, L) - 1] += 1   (int64 [K][L]),    tail[k] += max(n - L, 0)   (int64 [K]).
 * Nothing connects two utterances; rows outside every utterance count nothing; an utterance outside 0 .. T or longer than
 * abn_hmm_max_len() adds nothing.  Integer arithmetic only: the same counts for any grid and any order of the utterances.
 * dur and tail are cleared by the entry (two memsets, one launch).  Refusals, before any launch: T, n_utt or K < 1:
 * ABN_E_ARG; K beyond abny_hmm_dense_max_k(): ABN_E_UNSUPPORTED; null pointers, L out of range: ABN_E_ARG. */
int32_t abnu_hmm_hsmm_max_duration(void);  /* host */
int64_t abnu_hmm_hsmm_viterbi_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D, int32_t L);   /* host */
int abnu_hmm_hsmm_viterbi(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                          const float* shift, const float* A, const float* B, const float* c0,
                          const float* li, const float* lx, int64_t K,
                          int32_t* ids, double* log_prob, int32_t* n_switch, int32_t* n_good,
                          void* ws, int64_t ws_bytes, void* stream, const float* ld, const float* ls, int32_t L);
int abnu_hmm_run_stats(const int32_t* ids, int64_t T, const int64_t* off, const int32_t* len, int64_t n_utt, int64_t K,
                       int32_t L, int64_t* dur, int64_t* tail, void* stream);

/* ---- The in-batch contrastive pair loss, InfoNCE / NT-Xent (csrc/nce.hip) -------------------------------------------------
 * Prefix abnt_; ledger abnet3_amd._lib.NEXT7_SYMBOLS with tests/test_gpu_nce.py.  abnet3_amd/loss.py (InfoNCELoss) states the
 * definition, tests/nce_np.py restates it.  e1, e2 [B][D] fp32; y [B] of y_dtype (abn_pair_loss's codes: 0 int8, 1 int32,
 * 2 int64, 3 float32, 4 float64); groups [B] int32 or null; tau > 0.  With a^_i = e1_i / max(|e1_i|, 1e-6), b^_j likewise
 * from e2, z[i][j] = <a^_i, b^_j> / tau over the cells that are not excluded ((i, j) is excluded when j != i and
 * groups[i] == groups[j]; null: none), r[i] = (y[i] == 1), n = sum r:
 *     la[i] = log sum_j exp z[i][j],   lb[j] = log sum_i exp z[i][j],   l[i] = (la[i] + lb[i]) / 2 - z[i][i]
 *     loss = sum_i r[i] l[i], divided by n when avg;   n = 0: loss 0 and zero gradients for either avg.
 * loss [1] fp32; terms [B] fp32 or null: every l[i], anchors or not; de1, de2 [B][D] fp32, both or neither (both null:
 * forward only, the same loss bits): the gradient of loss with respect to e1 and e2, through the normalisation (the
 * projection only where the norm is at least 1e-6).  A row with y != 1 is no anchor; its vectors stay candidates.
 *
 * The B x B similarities never reach memory: exact-fp32 MFMA tiles folded into running (max, sum) pairs, then recomputed
 * and fed through LDS into the gradient GEMM.  No floating-point atomics, every sum in a fixed order: two calls on the same
 * inputs give the same bits, and swapping (e1, de1) with (e2, de2) swaps the outputs' bits (groups symmetric by
 * construction).  Padding columns and excluded cells have weight exactly 0.  The candidates of a row block are split over
 * up to 16 workgroups by the grid; ABN_NCE_SPLIT = 1 .. 16 in the environment forces the split (read at every call; the
 * results stay inside the same error bars, the bits may differ: the split moves the points where partial sums are merged).
 *
 * D <= abnt_nce_max_d() (256: the gradient accumulators of a 128-row block stay in registers), B <= 2^20.  Workspace:
 * abnt_nce_ws_bytes(B, D) bytes under the same ABN_NCE_SPLIT, 16-byte aligned, -1 with abn_last_error for refused sizes:
 * the unit rows, a handful of [B] vectors, 2 x split (max, sum) pairs per row and 2 x split gradient slabs [B][D'] (D' = D
 * rounded up to 4) -- O(B D split), split <= 16, never B x B.  It need not be cleared.  Nine launches (seven forward only).
 * Refusals, all before any launch: B < 1 or D < 1: ABN_E_ARG; D or B beyond the limits: ABN_E_UNSUPPORTED; null e1, e2, y,
 * loss or ws, a y_dtype outside 0 .. 4, tau not finite or <= 0 (or so small that 1 / tau is not a finite float), only one of
 * de1 / de2, a misaligned workspace: ABN_E_ARG. */
int64_t abnt_nce_max_d(void);              /* host */
int64_t abnt_nce_ws_bytes(int64_t B, int64_t D);      /* host */
int abnt_nce_loss(const float* e1, const float* e2, const void* y, int y_dtype, const int32_t* groups, int64_t B, int64_t D,
                  float tau, int avg, float* loss, float* terms, float* de1, float* de2, void* ws, void* stream);

/* ---- The histogram of within-cluster edit distances, without a pair table (csrc/edit_hist.hip) ------------------------------
 * Prefix abns_; ledger abnet3_amd._lib.EVAL_SYMBOLS with tests/test_tde_full_host.py and tests/test_gpu_tde_full_contract.py
 * (the top comment says why it is no NEXT<n>_SYMBOLS).  abnet3_amd/tde.py states the definition, tests/tde_full_np.py restates
 * it.  sym [rows] int32 is the symbol table; token t (n_tokens of them, flat in cluster order) has the transcription
 * sym[tok_off[t] .. tok_off[t] + tok_n[t]), lies in file tok_file[t] between tok_on[t] and tok_end[t] (float64 seconds) and
 * belongs to group tok_group[t] (a speaker id; tok_group null: one group).  tok_off int64, tok_n / tok_file / tok_group
 * int32, all DEVICE arrays.  cl_first [n_clusters + 1] int64 is a HOST array read during the call: cluster c holds the tokens
 * cl_first[c] .. cl_first[c + 1].  For every unordered pair (a, b) of tokens of one cluster:
 *     same file and min(tok_end[a], tok_end[b]) > max(tok_on[a], tok_on[b]):  nothing (the pair overlaps itself)
 *     else counts[0] += 1;   both tok_n == 0:  counts[1] += 1 and nothing more
 *     else hist[g][d][L] += 1 with d the Levenshtein distance (unit costs; a side of length 0 gives d = L), L = max(tok_n[a],
 *     tok_n[b]) and g = (tok_group[a] != tok_group[b]).
 * hist [2][M + 1][M + 1] int64 and counts [2] int64 are OVERWRITTEN: neither they nor the workspace need be cleared.  M,
 * 1 .. abns_edit_hist_max_len() (256), is the caller's bound on every tok_n.  Integer atomics only (32-bit in LDS, flushed
 * into 64-bit global ones long before a counter could wrap): the same counts for any grid, any order of the tokens inside a
 * cluster and any order of the clusters.  ABN_EDIT_HIST_BLOCKS = 1 .. 65536 in the environment forces the number of
 * workgroups (read at every call; default 4096).
 *
 * No array grows with the number of pairs.  Workspace: abns_edit_cluster_hist_ws_bytes(n_tokens, n_clusters, n_pairs) bytes
 * (16 + 20 bytes per cluster rounded up to 256: the prefix of C(size, 2) over the clusters that hold a pair; n_tokens and
 * n_pairs only have to be in range), 16-byte aligned, -1 with abn_last_error for negative sizes or more than 2^31 - 1 tokens
 * or clusters.  Refusals by ABN_E_ARG before any launch: M out of range, a negative size, more than 2^31 - 1 tokens or
 * clusters, a null pointer (sym may be null when rows == 0, the token columns when n_tokens == 0, tok_group always), a
 * misaligned workspace, a cl_first that does not start at 0, end at n_tokens or that decreases; a short workspace:
 * ABN_E_WORKSPACE.  The tokens are then checked by a launch of their own, for whose answer the call WAITS on the stream (the
 * entry is not for graph capture): a token with tok_n outside 0 .. M or tok_off outside 0 .. rows - tok_n makes the call
 * return ABN_E_ARG with hist and counts untouched (only the workspace has been written). */
int64_t abns_edit_hist_max_len(void);      /* host */
int64_t abns_edit_cluster_hist_ws_bytes(int64_t n_tokens, int64_t n_clusters, int64_t n_pairs);   /* host */
int abns_edit_cluster_hist(const int32_t* sym, int64_t rows, const int64_t* tok_off, const int32_t* tok_n,
                           const int32_t* tok_file, const double* tok_on, const double* tok_end, const int32_t* tok_group,
                           int64_t n_tokens, const int64_t* cl_first, int64_t n_clusters, int64_t M, int64_t* hist,
                           int64_t* counts, void* ws, int64_t ws_bytes, void* stream);

/* ---- The reconstruction loss of the correspondence autoencoder and its gradient (csrc/recon.hip) ----------------------------
 * Prefix abnr_; ledger abnet3_amd._lib.CAE_SYMBOLS with tests/test_cae_host.py and tests/test_gpu_cae_contract.py (the top
 * comment says why it is no NEXT<n>_SYMBOLS).  abnet3_amd/loss.py (CorrespondenceLoss) states the definition,
 * tests/cae_np.py restates it.  r1, r2 [B][D] fp32: the decoder's outputs for tower 1 and tower 2; x1, x2 [B][D] fp32: the
 * network's inputs; y [B] with abn_pair_loss's dtype codes (0 int8, 1 int32, 2 int64, 3 float32, 4 float64), "same" is
 * y == 1.  With s = (symmetric != 0):
 *     mode 0 (correspondence): R = {i : y[i] == 1},  t[i] = |r1[i] - x2[i]|^2 + s |r2[i] - x1[i]|^2
 *     mode 1 (autoencoder):    R = every row, y is not read (it may be null),  t[i] = |r1[i] - x1[i]|^2 + s |r2[i] - x2[i]|^2
 *     loss = c sum over R of t[i],  c = 1, or with avg 1 / (|R| D (1 + s)): the mean squared error per reconstructed element;
 *     |R| = 0: loss 0 and zero gradients for either avg.
 * loss [1] fp32; terms [B] fp32 or null: t[i], exactly 0 for a row outside R; dr1, dr2 [B][D] fp32, both or neither (both
 * null: value only, the same loss bits): the gradient of loss with respect to r1 and r2 -- 2 c (r - target) on a row of R,
 * exact zeros elsewhere, dr2 all zeros when symmetric == 0.  EVERY element of loss, terms, dr1 and dr2 is overwritten.
 *
 * One half-wave per row; differences, row sums and the total in float64, each rounded to fp32 once.  Under avg in mode 0 the
 * rows of R are counted on the device by a launch of the call's own: no read-back and no stream wait, the entry can be
 * captured into a graph.  No floating-point atomics and no ticket counter; every sum has one order that depends on (B, D)
 * alone: the same bits from call to call, for aligned and misaligned tables, and for any grid.  ABN_RECON_ROWS = 1 .. 4096 in
 * the environment forces the rows one workgroup walks (read at every call; default 8, a row per half-wave).  Swapping
 * (r1, x2, dr1) with (r2, x1, dr2) under symmetric != 0 gives the same loss bits and the swapped gradients.  16-byte loads
 * and stores only where D % 4 == 0 and r1, r2, x1, x2 (and dr1, dr2 when given) are 16-byte aligned.
 *
 * D <= abnr_recon_max_d() (16384), B <= 2^22.  Workspace: abnr_recon_ws_bytes(B, D) bytes (16 + 8 B: the scale and one
 * float64 per row), 16-byte aligned, -1 with abn_last_error for refused sizes.  It need not be cleared.  Two launches, three
 * under avg in mode 0.  Refusals, all before any launch: B < 1 or D < 1: ABN_E_ARG; D or B beyond the limits:
 * ABN_E_UNSUPPORTED; null r1, r2, x1, x2, loss or ws, a null y in mode 0, a y_dtype outside 0 .. 4, a mode outside 0 .. 1,
 * only one of dr1 / dr2, a misaligned workspace: ABN_E_ARG. */
int64_t abnr_recon_max_d(void);            /* host */
int64_t abnr_recon_ws_bytes(int64_t B, int64_t D);    /* host */
int abnr_recon_loss(const float* r1, const float* r2, const float* x1, const float* x2, const void* y, int y_dtype, int64_t B,
                    int64_t D, int mode, int symmetric, int avg, float* loss, float* terms, float* dr1, float* dr2, void* ws,
                    void* stream);

/* ---- Batched soft-DTW over cosine cells and its gradient (csrc/softdtw.hip) ------------------------------------------------
 * Prefix abnq_; ledger abnet3_amd._lib.SDTW_SYMBOLS with tests/test_sdtw_host.py and tests/test_gpu_sdtw_contract.py (the top
 * comment says why it is no NEXT<n>_SYMBOLS).  abnet3_amd/softdtw.py and abnet3_amd/loss.py (SoftDTWLoss) are the callers,
 * tests/sdtw_np.py restates the definition in float64.
 *
 * e [R][D] fp32: one table of rows.  Problem p of P is two runs of its rows, x_i = e[off1[p] + i], i < n1[p], and
 * y_j = e[off2[p] + j], j < n2[p] (the runs of one problem or of different problems may overlap or coincide).  off1, off2
 * [P] int64 and n1, n2 [P] int32 are DEVICE arrays.  With x^_i = x_i / max(|x_i|, 1e-6), y^_j likewise (the norm in float64),
 * c[i][j] = <x^_i, y^_j>, d[i][j] = 1 - c[i][j], gamma > 0 and
 *     softmin(a, b, c) = -gamma log(exp(-a / gamma) + exp(-b / gamma) + exp(-c / gamma))   (about the minimum: +inf adds 0)
 *     r[0][0] = 0, every other r[0][.] and r[.][0] = +inf,  r[i][j] = d[i-1][j-1] + softmin(r[i-1][j-1], r[i-1][j], r[i][j-1])
 * abnq_softdtw_forward writes value[p] = r[n1[p]][n2[p]] (fp32, every element).  With keep != 0 it leaves in the workspace
 * what abnq_softdtw_backward needs; with keep == 0 it does not, and the workspace may be smaller.
 *
 * abnq_softdtw_backward takes the same problem arguments, the workspace of a forward with keep != 0 on them, and w [P] fp32,
 * w[p] = d loss / d value[p].  With E[n][m] = 1 and, i and j descending,
 *     E[i][j] = E[i+1][j] exp((r[i+1][j] - r[i][j] - d[i+1][j]) / gamma) + E[i][j+1] exp((r[i][j+1] - r[i][j] - d[i][j+1]) / gamma)
 *             + E[i+1][j+1] exp((r[i+1][j+1] - r[i][j] - d[i+1][j+1]) / gamma)          (terms outside the matrix are 0)
 * it writes the gradients of sum_p w[p] value[p] with respect to the rows as BLOCKS IN PROBLEM ORDER: g1 [sum n1][D], problem
 * p's rows at sum of n1[0 .. p-1], and g2 [sum n2][D] likewise:
 *     g1[i] = -(w / |x_i|) (sum_j E[i][j] y^_j - (sum_j E[i][j] c[i][j]) x^_i)      where |x_i| >= 1e-6,
 *     g1[i] = -(w 1e6) sum_j E[i][j] y^_j                                             below the clamp,      g2[j] symmetric.
 * Every element of g1 and g2 is written, no two problems touch one address, nothing needs clearing; w[p] == 0 gives a block
 * of exact zeros.  Folding the blocks into a gradient of e is the caller's (abnet3_amd/softdtw.py: two ordered index_add_).
 *
 * c is fp32: the cosine formed in float64 from the fp32 rows and rounded once.  The recurrences for r and E, the norms, x^, y^ and
 * every sum of the gradients are float64; r and E are stored as float64.  No floating-point atomics, every sum has one fixed
 * order: the same bits from call to call, and a problem's bits depend neither on P, nor on its position, nor on its
 * neighbours, nor on the grid (ABN_SDTW_GRID = 1 .. 2048 in the environment forces the workgroups, read at every call;
 * default 2048).  One workgroup of four waves per problem; the forward is two launches, the backward one.
 *
 * Limits: n1[p], n2[p] in 1 .. abnq_softdtw_max_len() (256), D in 1 .. abnq_softdtw_max_d() (1024), P <= 2^24, R < 2^40.
 * Workspace: abnq_softdtw_ws_bytes(n1_host, n2_host, P, D, keep) bytes EXACTLY, from HOST copies of the lengths, -1 with
 * abn_last_error for a refused size.  With N = sum n1 + sum n2, cells = sum n1 n2, and every part rounded up to 16 bytes:
 *     64 (header) + 24 (P + 1) (prefix sums) + 16 N (1 / max(|x|, 1e-6) and |x|) + 4 cells (c)
 *     + with keep: 8 cells (r) + 8 cells (E)
 * (nothing in it is D wide: the rows are read from e, which must therefore be unchanged between a forward and its backward)
 * 16-byte aligned; it need not be cleared.  The header records P, R, D, the sums, gamma, keep and a 32-bit hash of e's address
 * and of off1, n1, off2, n2 of the last forward; the backward compares them with its own arguments.
 * Refusals, all before any launch (the entries copy the four device arrays -- the backward also the header -- to the host,
 * in one copy when off1, off2, n1, n2 lie end to end in one allocation, and WAIT for the stream: they are not for graph capture): P < 0, D < 1, R out of range, gamma not finite or not > 0: ABN_E_ARG;
 * D or P beyond the limits: ABN_E_UNSUPPORTED; (P > 0:) a null or misaligned pointer (e, n1, n2, value, w, g1, g2: 4 bytes, off1,
 * off2: 8, ws: 16): ABN_E_ARG; a length < 1: ABN_E_ARG, > max_len: ABN_E_UNSUPPORTED; off < 0 or off + n > R: ABN_E_ARG;
 * ws_bytes too small: ABN_E_WORKSPACE; a backward on a workspace without a forward, with a forward of keep == 0 or of another
 * problem: ABN_E_ARG.  P == 0 is a successful no-op (no pointer is looked at). */
int64_t abnq_softdtw_max_len(void);        /* host */
int64_t abnq_softdtw_max_d(void);          /* host */
int64_t abnq_softdtw_ws_bytes(const int32_t* n1_host, const int32_t* n2_host, int64_t P, int64_t D, int keep);   /* host */
int abnq_softdtw_forward(const float* e, int64_t R, int64_t D, const int64_t* off1, const int32_t* n1, const int64_t* off2,
                         const int32_t* n2, int64_t P, float gamma, float* value, void* ws, int64_t ws_bytes, int keep,
                         void* stream);
int abnq_softdtw_backward(const float* e, int64_t R, int64_t D, const int64_t* off1, const int32_t* n1, const int64_t* off2,
                          const int32_t* n2, int64_t P, float gamma, const float* w, float* g1, float* g2, void* ws,
                          int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ABNET3_HIP_NEXT_H */
