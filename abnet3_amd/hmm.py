"""Sticky-HMM smoothing of Gaussian posteriorgrams on the MI355X: forward-backward over a fitted mixture's components.

    python -m abnet3_amd.hmm fit-stay GMM.npz FEATURES MODEL.npz [--stay P] [--n-iter N] [--tol T]
    python -m abnet3_amd.hmm fit GMM.npz FEATURES MODEL.npz [--stay P] [--n-iter N] [--tol T] [--params mvws]
    python -m abnet3_amd.hmm transform MODEL.npz FEATURES OUT [--mode smooth|filter]
    python -m abnet3_amd.hmm decode MODEL.npz FEATURES OUT [--min-duration S]      (a full-transition MODEL: no minimum)
    python -m abnet3_amd.hmm fit-trans MODEL_OR_GMM.npz FEATURES OUT.npz [--n-iter N] [--params mvti] [--alpha A]
                                                                         [--viterbi [--min-duration S]]

``GmmPosteriorgram`` treats every frame on its own, so its posteriors flicker.  An HMM over the mixture's components
with a single "stay" probability is the smallest acoustic-unit model that has a likelihood: its forward-backward pass
gives smoothed [rows, K] posteriors for the KL routes (``ABXEvaluator(distance='kl')``, ``QbeSearcher(distance='kl')``),
a sequence likelihood, and the expected number of stays, from which the stay probability is fitted by EM
(``fit_stay``); ``fit`` re-estimates the means, variances and weights under the HMM as well (Baum-Welch).  The
reference has no such model; the definition is the build's own ("parity unpinned") and
tests/hmm_np.py and tests/hmm_bw_np.py restate it in numpy.

The definition this module computes, over a fitted mixture (weights w, means, variances, shift of gmm.py):

* States: the K components.  Initial distribution: w.  Transitions: a[j, k] = rho [j == k] + (1 - rho) w[k]: with
  probability rho the unit stays, otherwise it is redrawn from the weights (and may come back the same).  rho = 0 is
  the frame-independent mixture exactly; w is the stationary distribution and the chain is reversible.
* Emissions: logN[t, k] = c0[k] + sum_d xc A + sum_d xc^2 B with gmm.py's xc, A, B (fp32, one GEMM of depth 2D + 1 on the
  matrix cores) and c0[k] = -0.5 sum_d (log(2 pi v) + m^2 / v): gmm.py's c without log w, rounded once from float64,
  finite for a component of weight 0.
* Device inputs: w32 = float32(w), rho as one float32; 1 - rho is taken in fp32.
* BAD frames (gmm.py's rule: a non-finite value in x or in xc^2): the output row is all zeros, the chain passes over
  the frame -- the previous good frame is its successor's predecessor --, and it counts neither as a frame nor as a
  transition.
* Scaled recursion per utterance over its good frames in order, fp32:
    m_t = max over {k : w32[k] > 0} of logN[t, k],   bt[t, k] = exp(logN[t, k] - m_t),
    pred_t = w32 at the first good frame, else rho ahat_prev + (1 - rho) w32,
    u = bt[t] pred_t,   c_t = sum_k u,   ahat_t = u / c_t,      loglik = sum_t (log c_t + m_t)  (float64 sum).
  Backward from the last good frame with bhat = 1:  gamma_t = ahat_t bhat;  entering frame t from its predecessor p,
    stays += sum_k rho ahat_p[k] bt[t, k] bhat[k] / c_t,   e = bt[t] bhat / c_t,   bhat <- rho e + (1 - rho) sum_k w32[k] e[k].
  mode 'smooth' gives gamma, mode 'filter' ahat (no backward sweep, stays 0).
* Range: 0 <= rho < 1 and float32(1 - rho) min{w32 > 0} >= 2^-100 (ValueError otherwise): then c_t >= 2^-100 and
  e <= 2^100, and nothing in the chain underflows to zero or overflows.
* EM for rho, the mixture fixed: rho_new = sum_u stays_u / sum_u max(n_good_u - 1, 0), clipped to [0, 0.9999]; the
  log-likelihood does not decrease from one iteration to the next.
* Baum-Welch (``fit``).  The model as a generative story: z_first ~ w; at every later good frame the unit stays with
  probability rho, otherwise it is redrawn from w; emissions are diagonal Gaussians.  The complete data hold the
  switch variable, so the E-step needs, per component k, over all good frames and with gamma the smoothed posteriors,
    N[k] = sum_t gamma_t(k),   S1[k][d] = sum_t gamma_t(k) xc,   S2[k][d] = sum_t gamma_t(k) xc^2
  (xc = fl32(x - shift) and xc^2 taken in fp32, as gmm.py does; the sums on the fp32 matrix cores, then float64), and
    stay_k[k] = sum over the transitions (p -> t) of rho ahat_p[k] e_t[k]
  with the e of the backward sweep above: the per-component terms of `stays`.  The M-step, host float64:
    means, variances:  m = S1 / N,  v = max(S2 / N - m^2, var_floor gv[d]); a component with N < min_count keeps its mean
      and variance (gmm.py's rule, with the mixture's var_floor, min_count and gv_).  With the means held fixed the
      variance is the second moment about the mean in force, S2 / N - 2 m S1 / N + m^2, floored the same way.
    weights:  draws[k] = max(N[k] - stay_k[k], 0), the expected number of times k was drawn from w, as a first frame or
      as a redraw (one that lands on the same unit counts);  w = draws / sum draws.  A weight below WEIGHT_MIN = 2^-80
      is set to exactly 0 and the rest are renormalised, so the range condition above cannot fail in the middle of a
      fit; such a component is retired for good (its gamma is 0 from then on), ``n_retired_`` counts the weights of 0.
    stay:  rho = sum_k stay_k / sum_u max(n_good_u - 1, 0), clipped to [0, 0.9999], as ``fit_stay`` does.
  Any subset of the four may be held fixed (params): each update maximises the expected complete-data log-likelihood
  in its own parameters, so the likelihood still does not decrease (a generalised EM).

On the device the recursion is one launch for the whole corpus (abn_hmm_forward_backward, csrc/hmm.hip): persistent
workgroups, one utterance at a time, one sum reduction per frame and sweep.  The output table holds ahat between the
sweeps, so there is no T x K array beyond it.  A Baum-Welch iteration is that launch with the per-component stays
(abn_hmm_forward_backward_stats) and abn_hmm_accumulate, which reads the gamma table once as the A operand of
abn_gmm_accumulate's statistics GEMM.  Limits: K <= abn_hmm_max_k(), D <= abn_gmm_max_d(), an utterance of at most
abn_hmm_max_len() frames; utterances must not overlap.  Left out: duration distributions for THIS model (its max-product
path has a minimum duration, below; the full-transition model's has explicit unit durations, at the end).

The max-product path (``viterbi``, ``StickyHmmPosteriorgram.decode`` / ``quantize``; abn_hmm_viterbi, one launch;
tests/hmm_vit_np.py restates it).  The model, the emissions and the BAD-frame rule are the ones above.

* Log tables ``viterbi_tables(w, stay) -> (lw, ls, lr)``, each [K] float32, computed on the host in float64 from
  w32 = float32(w), r = float32(stay) and omr = float32(1) - r and rounded once:
    lw = log w32,   ls = log(r + omr w32),   lr = log(omr w32);
  lw and lr are -inf where w32 == 0 (ls too when stay == 0); check_stay's range condition applies.  The kernel takes no
  logarithm.
* Recurrence per utterance over its good frames in order, fp32; every operation is one rounded add or a compare, so
  contraction cannot change it.  s = logN[t, :] are the score tile's bits.
    first good frame:  u[k] = s[k] + lw[k]
    later frames:      a = W[k] + ls[k],  st[k] = a > lr[k]  (strict: a tie goes to the switch),
                       u[k] = s[k] + (st[k] ? a : lr[k])
    every good frame:  M = max_k u[k],  j* its lowest index,  W[k] = u[k] - M,  log_prob += M  (float64 sum);
                       the frame records st[.] and the PREVIOUS good frame's j*.
  max_j (delta[j] + log a[j, k]) = max(delta[k] + ls[k], max_j delta[j] + lr[k]) because ls >= lr, so this is the exact
  max-product recursion.  A component of weight 0 has u = -inf throughout and is never chosen.
* Traceback from the last good frame's j*: a frame keeps cur while st[cur] is set, otherwise cur becomes that frame's
  recorded predecessor.
* Outputs: ids [T] int32 (BAD frames -1; rows outside every utterance keep what they held), log_prob [n_utt] float64 (the
  log joint probability of the best path and the good frames), n_switch [n_utt] int32 (the changes of id between
  consecutive good frames), n_good [n_utt] int32.  A refused utterance (outside 0 .. T, or longer than the workspace was
  sized for) is left untouched: log_prob NaN, n_switch and n_good -1.
* Minimum duration (``min_duration`` = S, an integer 1 .. 8, default 1 = the recurrence above; abnx_hmm_viterbi_dur,
  csrc/vit_wave.h; tests/vit_dur_np.py restates it): the minimum-duration topology of HMM acoustic-unit discovery.  Every
  component becomes a left-to-right chain of S states with tied emissions of which only the last may repeat.  Good frames
  only (durations count good frames): a path is a sequence of segments (k_i, n_i), every segment but the utterance's last
  has n_i >= S (the end of the utterance may cut the last one short), and its score is the sum of the frames' scores
  + lw[k_1] + lr[k_i] for each later segment + max(n_i - S, 0) ls[k_i]: forced advances cost nothing, only the frames
  beyond the S-th pay the stay term.  Recurrence, fp32, one rounded add or a compare per operation; V[k][0 .. S-1] the
  normalised previous values, E = max_k V[k][S-1], exitj the lowest k whose U[k][S-1] was the largest (0 if all -inf):
    first good frame:   U[k][0] = s + lw[k], every other state -inf
    later good frames:  U[k][0] = s + (E + lr[k]);   U[k][i] = s + V[k][i-1] for 0 < i < S-1;
                        a = V[k][S-1] + ls[k],  st = a > V[k][S-2]  (strict: a tie goes to the advance),
                        U[k][S-1] = s + (st ? a : V[k][S-2])
    every good frame:   N_t = max over all (k, i) of U,  V = U - N_t,  log_prob = the sum of the N_t in float64.
  The final state is the lowest k, then the largest i, with V[k][i] == 0.  Stored per frame: the st bits and the previous
  good frame's exitj.  Going backwards: in state S-1 a set bit keeps (k, S-1) and a clear bit goes to (k, S-2); from state
  i, 0 < i < S-1, to (k, i-1); from state 0 to (exitj, S-1).  n_switch = the changes of id.  Where S ls[k] < lr[k] (a
  small stay and a large S) closing a unit and entering it again beats staying; the ids do not show such a boundary, and
  every run of ids but the last is >= S either way.  log_prob is then the score above, not a log joint probability of
  the sticky chain.  Left out: a maximum duration, untied emission states (a duration distribution per unit exists for the
  full-transition model only, at the end); S is untuned on real speech.
* At stay = 0 all three tables are equal and the recurrence is argmax_k fl32(s[k] + lw[k]) frame by frame: the mixture's
  hard assignment.

The full-transition model (``dense_forward_backward``, ``TransitionHmmPosteriorgram``; abny_hmm_dense_forward_backward,
csrc/hmm_dense.hip; tests/hmm_dense_np.py restates it).  Over a fitted mixture (means, variances, shift; the mixture
weights play no part):

* States: the K components.  init [K] float32; trans [K][K] float32, row-stochastic,
  trans[j][k] = P(k at t | j at the previous good frame).
* Range: every entry of init and trans is at least 2^-100 (ValueError otherwise, as check_stay does).
* Emissions: the sticky model's logN[t, k] from c0, A, B: the same score tile, the same bits.  m_t = max_k logN[t, k],
  bt = exp(logN - m_t).  With the range: c_t >= 2^-100 and e <= 2^100, as in the sticky chain.
* BAD frames follow the sticky rule exactly: the output row is zero, the chain passes over the frame, and it counts
  neither as a frame nor as a transition.
* Forward, fp32, per utterance over its good frames:
    pred = init at the first good frame, else pred[k] = sum_j ahat_prev[j] trans[j][k],
    u = bt pred,   c_t = sum_k u,   ahat = u / c_t,      loglik = sum_t (log c_t + m_t)  (float64 sum).
* Backward from the last good frame with bhat = 1:  gamma_t = ahat_t bhat;  entering frame t from its predecessor p,
    e = bt[t] bhat / c_t,   G[j][k] += ahat_p[j] e[k],   bhat[j] <- sum_k trans[j][k] e[k].
  The expected transition counts are xi[j][k] = trans[j][k] G[j][k]; first[k] += gamma at the utterance's first good frame.
* mode 'smooth' gives gamma, mode 'filter' ahat (no backward sweep, the statistics zero).
* M-step on the host, float64, with a pseudo-count alpha >= 0 (``transition_update``):
    trans[j][k] = (xi[j][k] + alpha) / (sum_k xi[j][k] + K alpha),   init[k] = (first[k] + alpha) / (sum first + K alpha);
  a row of trans with no mass and alpha = 0 keeps its old values.  After the update every entry below
  TRANS_MIN = 2^-80 is raised to it and the row is renormalised once, so the range condition cannot fail in the middle
  of a fit.  Means and variances follow ``fit``'s rule above, from abn_hmm_accumulate on the gamma table.  alpha is untuned.
* The K-term dot products run in the kernel's own fixed order: thread t of 256 takes own = t mod K' (K' = K rounded up to
  16, 32, 64 or 128) and the slice t div K' of K'^2 / 256 consecutive indices of the other side, adds its products in
  ascending order with fused multiply-adds, and the 256 / K' partial sums are added slice 0 first.
* Limits: K <= abny_hmm_dense_max_k() (128: the matrix lives in LDS), D <= abn_gmm_max_d(), an utterance of at most
  abn_hmm_max_len() frames; utterances must not overlap.  Left out: sparse or banded matrices, K above the LDS limit
  (forward-backward itself has no duration states: the explicit durations at the end are the max-product path's alone).
  Nothing here is tuned or measured on real speech.

The max-product path of the full-transition model (``dense_viterbi``, ``TransitionHmmPosteriorgram.decode`` / ``quantize``;
abnz_hmm_dense_viterbi, csrc/hmm_dense_vit.hip, one launch; tests/hmm_dense_vit_np.py restates it).  Model, emissions and
BAD-frame rule are those of the full-transition model: s = logN[t, :] are the score tile's bits; a BAD frame gets id -1, the
chain passes over it, and it counts neither as a frame nor as a transition.

* Log tables ``log_transitions(init, trans) -> (li [K], lt [K][K])``, float32, computed on the host in float64 from the
  float32 init / trans and rounded once.  check_transitions' range applies (every entry >= 2^-100), so every logarithm is
  finite; ``dense_viterbi`` refuses tables that hold NaN, +inf or -inf (ValueError).  The kernel takes no logarithm.
* Recurrence per utterance over its good frames in order, fp32; every operation is one rounded add or a compare, so
  contraction cannot change it.
    first good frame:   u[k] = s[k] + li[k]
    later good frames:  c[k] = max_j (W[j] + lt[j][k]),  bp[k] = the lowest j that attains the max,  u[k] = s[k] + c[k]
    every good frame:   M = max_k u[k],  W = u - M,  log_prob += M  (a float64 sum in frame order)
  The final state is the lowest k with W[k] == 0.
* Traceback from the final state over the good frames backwards: ids[t] = cur, then cur = bp_t[cur].  Among all optimal
  paths this is the smallest one when read from the last frame to the first.
* Outputs (abn_hmm_viterbi's): ids [T] int32 (BAD frames -1; rows outside every utterance keep what they held), log_prob
  [n_utt] float64, n_switch [n_utt] int32 (the changes of id between consecutive good frames), n_good [n_utt] int32.  An
  utterance with no good frame gives (0.0, 0, 0) and all -1.  A refused utterance (outside 0 .. T, or longer than the
  workspace was sized for) is left untouched: log_prob NaN, n_switch and n_good -1.
* Minimum duration (``min_duration`` = S, an integer 1 .. 8, default 1 = the recurrence above; abnw_hmm_dense_viterbi_dur,
  csrc/hmm_dense_vit.hip with csrc/vit_wave.h's chain step; tests/hmm_dense_dur_np.py restates it).  Every unit k becomes a
  left-to-right chain of S states with tied emissions of which only the last may repeat; a unit is left only from its last
  state and only for a DIFFERENT unit.  Good frames only (durations count good frames): a path is a sequence of segments
  (k_i, n_i) with k_i != k_{i+1}, every segment but the utterance's last has n_i >= S, and its score is the sum of the
  frames' scores + li[k_1] + lt[k_{i-1}][k_i] for each later segment + max(n_i - S, 0) lt[k_i][k_i].  Adjacent segments
  differ, so the maximal runs of the ids ARE the segments and n_switch = segments - 1 (the sticky model's "re-entering the
  same unit" cannot happen).  Recurrence for S >= 2, fp32, one rounded add or a compare per operation; V[k][0 .. S-1] the
  normalised previous values:
    first good frame:   U[k][0] = s + li[k], every other state -inf
    later good frames:  ent[k] = max over j != k of (V[j][S-1] + lt[j][k]),  bp[k] = the lowest such j
                        (strict compares in ascending j; K = 1: ent = -inf, bp irrelevant)
                        U[k][0] = s + ent[k];   U[k][i] = s + V[k][i-1] for 0 < i < S-1
                        a = V[k][S-1] + lt[k][k],  st = a > V[k][S-2]  (strict: a tie goes to the advance)
                        U[k][S-1] = s + (st ? a : V[k][S-2])
    every good frame:   N_t = max over all (k, i) of U,  V = U - N_t,  log_prob += N_t  (float64, frame order)
  The final state is the lowest k, then the largest i, with V[k][i] == 0.  Going backwards from (k, i): i == S-1 and st set
  -> (k, S-1); else i > 0 -> (k, i-1); else -> (bp[k], S-1), one switch.  S = 1 is NOT this recurrence (its diagonal sits
  inside the argmax): min_duration = 1 makes the call without it, and abnw_hmm_dense_viterbi_dur launches that kernel.
  log_prob is the score above, not a log joint probability of the K-state chain.  Left out: a maximum duration, untied
  emission states; S is untuned on real speech.  (A duration distribution per unit: the explicit durations below.)
* Limits: the full-transition model's.  Left out: sparse or banded matrices, K above the LDS limit.  Nothing here is tuned
  or measured on real speech.

Viterbi training of the full-transition model (``hard_stats``, ``TransitionHmmPosteriorgram.fit_viterbi``;
abnv_hmm_hard_stats, csrc/hmm_hard.hip; tests/hmm_hard_np.py restates it): hard EM on the decoded path itself (segmental
k-means, Juang & Rabiner 1990), the alternative to ``fit``'s smoothed posteriors and the only one that trains the model
``decode(min_duration=S)`` runs.

* The hard statistics of unit ids [T] int32.  A frame is good if 0 <= ids[t] < K; every other id is BAD and is passed over
  (the decoders write -1).  Per utterance u, a_0 .. a_{n-1} the ids of its good frames in order, S = min_duration:
    n_good[u] = n;   counts[K][a_0] += 1 when n >= 1   (row K is `first`, the layout of dense_forward_backward's stats)
    i >= 1, a_i != a_{i-1}:  counts[a_{i-1}][a_i] += 1   (a switch)
    i >= 1, a_i == a_{i-1}:  counts[a_i][a_i] += 1 only if i >= S and a_{i-1} = ... = a_{i-S} = a_i   (a stay in the chain's
                             last state; otherwise the frame is a forced advance and counts nothing)
  A run of n frames gives max(n - S, 0) stays: exactly the lt[k][k] terms of the minimum-duration score above, so the counts,
  normalised by rows, maximise that score of the path over row-stochastic matrices.  At S = 1 rows 0 .. K - 1 are
  ``bigram_counts``.  Nothing connects two utterances; rows outside every utterance contribute nothing.
    sums [K, 2D + 1] float64 = [S1 | S2 | N] over the good frames: N[k] the frames with id k, S1 / S2 the sums of xc and
    xc^2, xc = fl32(x - shift), xc^2 rounded once; an entry whose xc^2 is not finite contributes 0 (``accumulate``'s rule).
* counts is integer arithmetic throughout: the same for any grid, any n_ranges and any order of the utterances.  sums: per
  range of whole 128-row blocks and per unit the frames are added in frame order in fp32, the ranges in range order in
  float64; no floating-point atomics, the same bits for the same inputs and n_ranges.  So the fp32 error of an entry is at
  most 2^-24 x (the longest partial's frames) x (the sum of the |terms|), the bar tests/test_gpu_hmm_hard.py holds it to.
* ``fit_viterbi``: iteration i decodes under the current parameters (``dense_viterbi`` with min_duration),
  viterbi_log_probs[i] = the mean best-path log probability per good frame, then ``hard_stats`` on the decoded ids, ONE
  read-back, ``baum_welch_update`` on the sums and ``transition_update`` on the counts (both unchanged).  Each half maximises
  the path score in its own arguments, so viterbi_log_probs does not decrease beyond the decoder's rounding slack (the
  variance floor, min_count, alpha > 0 and TRANS_MIN are the usual exceptions).  It stops when the gain is below tol or when
  no id changed (counted on the device).  No T x K table is allocated.
* Left out: Viterbi training of the sticky model, whose stay and redraw share one log term (use
  ``TransitionHmmPosteriorgram.from_sticky``); K above the LDS limit.  Nothing here is tuned or measured on real speech.

Explicit unit durations: a hidden semi-Markov model (HSMM) over the same units (``hsmm_viterbi``, ``run_stats``,
``duration_update``, ``TransitionHmmPosteriorgram.set_durations`` / ``decode(durations=True)`` / ``fit_viterbi(params='mvtid',
max_duration=L)``; abnu_hmm_hsmm_viterbi and abnu_hmm_run_stats, csrc/hmm_hsmm.hip; tests/hmm_hsmm_np.py restates it).
Emissions, BAD-frame rule, init and trans are the full-transition model's; durations count good frames only (a BAD frame gets
id -1, the chain passes over it, and it counts as nothing).

* A path is a sequence of segments (k_i, n_i) with k_i != k_{i+1} and n_i >= 1: the maximal runs of the ids are the segments
  and n_switch = segments - 1.  Unit k has a duration law with a free head of L - 1 values and a geometric tail, L an integer
  2 .. 32 (``hsmm_max_duration``): with q[k][1..L] summing to 1 and r[k] in (0, 1),
    p_k(d) = q[k][d] for d < L,     p_k(d) = q[k][L] (1 - r[k]) r[k]^(d - L) for d >= L,
  so every utterance has a finite-score path for every K >= 1 and a long silence needs no artificial split.
* Host-made float32 tables, float64 logarithms rounded once: ``duration_tables(q, r) -> (ld [K, L], ls [K])`` with
  ld[k][i] = log q[k][i] for i < L, ld[k][L] = log(q[k][L] (1 - r[k])), ls[k] = log r[k]; ``switch_log_transitions(init, trans)
  -> (li, lx)`` with lx[j][k] = log(trans[j][k] / (1 - trans[j][j])) for j != k (the diagonal is never read).  Every q, r and
  1 - r must be at least 2^-100 (ValueError), so every entry is finite; the kernel takes no logarithm.
  ``geometric_durations(trans, L)`` is the law under which this model scores a path as the plain one does (r = trans[k][k]),
  up to log(1 - r) of the LAST unit: the score below closes the utterance's last segment.
* The score of a path: the sum of the frames' scores + li[k_1] + lx[k_{i-1}][k_i] for each later segment + log p_{k_i}(n_i)
  for every segment INCLUDING the utterance's last, which is treated as complete, not censored.
* Recurrence over an utterance's good frames, fp32, every operation one rounded add or one compare.  V[k][1..L] are the
  normalised previous values; state i = "in unit k, the current segment is i frames long", state L = "L or more":
    first good frame:   U[k][1] = s[k] + li[k], every other state -inf
    later good frames:  x[j] = max_i (V[j][i] + ld[j][i]),  xi[j] = the lowest i attaining it  (strict compares, ascending i)
                        ent[k] = max over j != k of (x[j] + lx[j][k]),  bp[k] = the lowest such j  (strict, ascending j;
                        K = 1: -inf);   U[k][1] = s[k] + ent[k];   U[k][i] = s[k] + V[k][i-1] for 1 < i < L
                        a = V[k][L] + ls[k],  st = a > V[k][L-1]  (strict: a tie goes to the advance)
                        U[k][L] = s[k] + (st ? a : V[k][L-1])
    every good frame:   N_t = max over (k, i) of U,  V = U - N_t,  log_prob += N_t  (float64, frame order)
    after the last:     F = max over (k, i) of (V[k][i] + ld[k][i]),  final = the lowest k, then the lowest i, attaining it;
                        log_prob += F
  Traceback from (k, i) at frame t: i == L and st set -> (k, L); otherwise i > 1 -> (k, i - 1); otherwise -> (bp[k],
  xi[bp[k]] as recorded at frame t), one switch.  Outputs are ``dense_viterbi``'s, refused utterances included.
* ``run_stats(ids, off, lens, K, L) -> (dur [K, L], tail [K])``, int64, one small launch: for every maximal run, over an
  utterance's good frames (0 <= id < K), of unit k with length n, dur[k][min(n, L) - 1] += 1 and tail[k] += max(n - L, 0).
  Integer arithmetic: the same for any grid and any order of the utterances.
* ``duration_update(dur, tail, q, r, alpha)`` on the host, float64: q[k][d] = (dur[k][d] + alpha) / (sum_d dur[k] + L alpha),
  r[k] = (tail[k] + alpha) / (tail[k] + dur[k][L-1] + 2 alpha) -- at alpha = 0 the maximiser of the duration part of the
  paths' score; a unit without any run at alpha = 0 keeps its old law; then the floor TRANS_MIN and one renormalisation.
* ``fit_viterbi(params='mvtid', max_duration=L)``: the letter d (this method only) learns the durations.  Iteration i decodes
  with ``hsmm_viterbi``, takes ``hard_stats`` at min_duration = 1 and ``run_stats`` on the same ids, reads back once, and
  applies ``baum_welch_update``, ``transition_update`` (both unchanged: the diagonal of the counts receives the stays, and
  the off-diagonal ratio of a row is the maximum-likelihood lx) and ``duration_update``.  ``transform``, ``score`` and ``fit``
  ignore the durations.
* L and alpha are untuned, and nothing here is measured on real speech.  Left out: K above the LDS limit, L above 32,
  duration laws in forward-backward.
"""
import argparse
import copy
import sys

import numpy as np
import torch

from . import _lib
from . import _utt
from . import gmm as _gmm

MODES = {'smooth': 0, 'filter': 1}
STAY_MAX = 0.9999
TINY = 2.0 ** -100
WEIGHT_MIN = 2.0 ** -80
PARAMS = 'mvws'
TRANS_MIN = 2.0 ** -80
DENSE_PARAMS = 'mvti'
HSMM_PARAMS = 'mvtid'
HSMM_MAX_DURATION = 32
DUR_TAIL_MAX = 1.0 - 2.0 ** -24


def max_len():
    return int(_lib.load().abn_hmm_max_len())


def max_k():
    return int(_lib.load().abn_hmm_max_k())


def emission_offsets(m, v):
    """c0 [K] float32 of float64 centred means and variances [K, D]: gmm.score_tables' c without log w."""
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return (-0.5 * (np.log(2.0 * np.pi * v) + m * m / v).sum(axis=1)).astype(np.float32)


def check_stay(who, stay, w32=None):
    """float32(stay) as a Python float, or ValueError: 0 <= stay < 1 and, with the weights, the range condition."""
    try:
        r = np.float32(stay)
    except (TypeError, ValueError):
        raise ValueError('%s: stay = %r, a number in [0, 1) is needed' % (who, stay))
    if not (np.isfinite(r) and 0.0 <= r < 1.0):
        raise ValueError('%s: stay = %r, a number in [0, 1) is needed' % (who, stay))
    if w32 is not None:
        w32 = np.asarray(w32, dtype=np.float32)
        pos = w32[w32 > 0]
        if not np.isfinite(w32).all() or (w32 < 0).any() or not len(pos):
            raise ValueError('%s: the weights must be finite, >= 0 and not all 0' % who)
        if float(np.float32(1.0) - r) * float(pos.min()) < TINY:
            raise ValueError('%s: (1 - stay) * min weight = %g is below 2^-100: the scaled recursion would underflow'
                             % (who, float(np.float32(1.0) - r) * float(pos.min())))
    return float(r)


def check_params(who, params):
    """The letters of `params` as a set, or ValueError: a non-empty string over 'mvws' without a repeat."""
    if not isinstance(params, str) or not params or len(set(params)) != len(params) or not set(params) <= set(PARAMS):
        raise ValueError('%s: params = %r, a non-empty choice of the letters of %r is needed '
                         '(m means, v variances, w weights, s stay)' % (who, params, PARAMS))
    return set(params)


def forward_backward(table, off, lens, shift, A, B, c0, w, stay, mode='smooth', out=None, want_stays=True, want_stay_k=False):
    """(post [T, K] fp32, loglik [n_utt] float64, stays [n_utt] float64 or None, n_good [n_utt] int32), device tensors,
    of the recursion the module docstring defines (abn_hmm_forward_backward, one launch).  off, lens: the utterances'
    first rows and lengths (host sequences or device tensors); they must not overlap.  Rows outside every utterance
    keep what `out` held (0 in a fresh table).  want_stay_k: a fifth element, stay_k [n_utt, K] float64, the
    per-component terms of stays (abn_hmm_forward_backward_stats; the four others are the same bits)."""
    lib = _lib.load()
    if mode not in MODES:
        raise ValueError('hmm.forward_backward: mode = %r, one of %s' % (mode, sorted(MODES)))
    T, D = _utt.table_shape('hmm.forward_backward', table)
    K = c0.shape[0]
    if A.shape != (K, D) or B.shape != (K, D) or shift.shape != (D,) or w.shape != (K,) or any(
            t.dtype != torch.float32 for t in (shift, A, B, c0, w)):
        raise ValueError('hmm.forward_backward: shift [D], A [K, D], B [K, D], c0 [K], w [K] float32 are needed')
    if K < 1 or K > max_k():
        raise ValueError('hmm.forward_backward: K = %d, the kernel takes 1 .. %d (abn_hmm_max_k)' % (K, max_k()))
    rho = check_stay('hmm.forward_backward', stay, w.cpu().numpy())
    off_h, len_h, n_utt, longest = _utt.utterance_spans('hmm.forward_backward', off, lens, T, max_len(), 'abn_hmm_max_len')
    table = _gmm._check_table('hmm.forward_backward', table)
    _lib.require_device(shift, A, B, c0, w)
    out = _utt.posterior_table('hmm.forward_backward', out, T, K, table.device)
    ll = torch.zeros(n_utt, dtype=torch.float64, device=table.device)
    st = torch.zeros(n_utt, dtype=torch.float64, device=table.device) if want_stays else None
    ng = torch.zeros(n_utt, dtype=torch.int32, device=table.device)
    sk = torch.zeros((n_utt, K), dtype=torch.float64, device=table.device) if want_stay_k else None
    if T and n_utt and longest:
        ws, off_d, len_d = _utt.workspace('hmm.forward_backward', lib.abn_hmm_ws_bytes, off_h, len_h, longest, K, D, table.device)
        head = [_lib.ptr(table), T, D, _lib.ptr(off_d), _lib.ptr(len_d), n_utt, _lib.ptr(shift), _lib.ptr(A), _lib.ptr(B),
                _lib.ptr(c0), _lib.ptr(w), K, rho, MODES[mode], _lib.ptr(out), _lib.ptr(ll), _lib.ptr(st), _lib.ptr(ng)]
        tail = [_lib.ptr(ws), ws.numel(), _lib.stream()]
        if want_stay_k:
            _lib.check(lib.abn_hmm_forward_backward_stats(*(head + [_lib.ptr(sk)] + tail)), 'abn_hmm_forward_backward_stats')
        else:
            _lib.check(lib.abn_hmm_forward_backward(*(head + tail)), 'abn_hmm_forward_backward')
    return (out, ll, st, ng, sk) if want_stay_k else (out, ll, st, ng)


def _emission_shapes(who, table, shift, A, B, c0):
    """(T, D, K) of a [T, D] float32 table and the emission tables that fit it, or ValueError."""
    T, D = _utt.table_shape(who, table)
    K = c0.shape[0]
    if A.shape != (K, D) or B.shape != (K, D) or shift.shape != (D,) or any(t.dtype != torch.float32 for t in (shift, A, B, c0)):
        raise ValueError('%s: shift [D], A [K, D], B [K, D], c0 [K] float32 are needed' % who)
    return T, D, K


def viterbi_tables(w, stay):
    """(lw, ls, lr), each [K] float32: the log tables of the max-product path (module docstring), computed on the host in
    float64 from w32 = float32(w), r = float32(stay) and omr = float32(1) - r and rounded once.  ValueError through
    check_stay (0 <= stay < 1 and the range condition)."""
    w32 = np.asarray(w, dtype=np.float32).ravel()
    r = np.float32(check_stay('hmm.viterbi_tables', stay, w32))
    omr = np.float32(1.0) - r
    w64 = w32.astype(np.float64)
    with np.errstate(divide='ignore'):
        lw = np.log(w64)
        ls = np.log(np.float64(r) + np.float64(omr) * w64)
        lr = np.log(np.float64(omr) * w64)
    lw[w32 == 0], lr[w32 == 0] = -np.inf, -np.inf
    return lw.astype(np.float32), ls.astype(np.float32), lr.astype(np.float32)


def _check_log_tables(who, lw, ls, lr, K):
    """The host checks of the three log tables (host arrays come back): [K] float32, lr <= ls, lw and lr -inf at the
    same places and not everywhere, ls finite wherever lw is, and nothing NaN or +inf."""
    for t in (lw, ls, lr):
        if not isinstance(t, torch.Tensor) or t.shape != (K,) or t.dtype != torch.float32:
            raise ValueError('%s: lw, ls, lr [K] float32 tensors are needed (hmm.viterbi_tables)' % who)
    a, b, c = (t.detach().cpu().numpy() for t in (lw, ls, lr))
    if np.isnan(a).any() or np.isnan(b).any() or np.isnan(c).any() or (a == np.inf).any() or (b == np.inf).any() or \
            (c == np.inf).any():
        raise ValueError('%s: the log tables must not hold NaN or +inf' % who)
    dead = np.isneginf(a)
    if not np.array_equal(dead, np.isneginf(c)):
        raise ValueError('%s: lw and lr must be -inf at the same components (those of weight 0)' % who)
    if dead.all():
        raise ValueError('%s: lw is -inf everywhere: no component has a weight' % who)
    if not np.isfinite(b[~dead]).all():
        raise ValueError('%s: ls must be finite at every component of positive weight' % who)
    if not (c <= b).all():
        raise ValueError('%s: lr <= ls is needed (a stay is at least as likely as a redraw of the same unit)' % who)


def viterbi(table, off, lens, shift, A, B, c0, lw, ls, lr, ids=None, want_log_prob=True, min_duration=1):
    """(ids [T] int32, log_prob [n_utt] float64 or None, n_switch [n_utt] int32 or None, n_good [n_utt] int32), device
    tensors, of the max-product recurrence the module docstring defines (abn_hmm_viterbi, one launch).  off, lens: the
    utterances' first rows and lengths (host sequences or device tensors); they must not overlap.  lw, ls, lr: the log
    tables of ``viterbi_tables``.  Rows outside every utterance keep what `ids` held (-1 in a fresh `ids`).
    min_duration = S > 1: every unit lasts at least S good frames (abnx_hmm_viterbi_dur, the same workspace); 1 is
    abn_hmm_viterbi itself."""
    lib = _lib.load()
    who = 'hmm.viterbi'
    min_duration = _utt.check_min_duration(who, min_duration)
    T, D, K = _emission_shapes(who, table, shift, A, B, c0)
    if K < 1 or K > max_k():
        raise ValueError('%s: K = %d, the kernel takes 1 .. %d (abn_hmm_max_k)' % (who, K, max_k()))
    _check_log_tables(who, lw, ls, lr, K)
    off_h, len_h, n_utt, longest = _utt.utterance_spans(who, off, lens, T, max_len(), 'abn_hmm_max_len')
    _utt.check_ids(who, ids, T)
    table = _gmm._check_table(who, table)
    _lib.require_device(shift, A, B, c0, lw, ls, lr)
    ids, lp, nsw, ng = _utt.path_results(ids, T, n_utt, want_log_prob, table.device)
    if T and n_utt and longest:
        ws, off_d, len_d = _utt.workspace(who, lib.abn_hmm_viterbi_ws_bytes, off_h, len_h, longest, K, D, table.device)
        args = (_lib.ptr(table), T, D, _lib.ptr(off_d), _lib.ptr(len_d), n_utt, _lib.ptr(shift), _lib.ptr(A), _lib.ptr(B),
                _lib.ptr(c0), _lib.ptr(lw), _lib.ptr(ls), _lib.ptr(lr), K, _lib.ptr(ids), _lib.ptr(lp), _lib.ptr(nsw), _lib.ptr(ng),
                _lib.ptr(ws), ws.numel(), _lib.stream())
        if min_duration == 1:
            _lib.check(lib.abn_hmm_viterbi(*args), 'abn_hmm_viterbi')
        else:
            _lib.check(lib.abnx_hmm_viterbi_dur(*(args + (min_duration,))), 'abnx_hmm_viterbi_dur')
    return ids, lp, nsw, ng


def accumulate(table, post, shift, n_ranges=0):
    """sums [K, 2D + 1] float64 = [S1 | S2 | N] on the device: the sum over the rows of post[t, k] [xc | xc^2 | 1]
    (abn_hmm_accumulate: `post` is read once; fp32 slabs per frame range, then float64 in range order; the same bits for
    the same n_ranges).  A non-finite entry of the table contributes 0; forward_backward leaves zero rows at BAD frames."""
    lib = _lib.load()
    T, D = _utt.table_shape('hmm.accumulate', table)
    if not isinstance(post, torch.Tensor) or post.dim() != 2 or post.dtype != torch.float32 or post.shape[0] != T or \
            not post.is_contiguous():
        raise ValueError('hmm.accumulate: post must be a contiguous [T, K] float32 tensor with the table\'s %d rows' % T)
    K = post.shape[1]
    if not isinstance(shift, torch.Tensor) or shift.shape != (D,) or shift.dtype != torch.float32:
        raise ValueError('hmm.accumulate: shift [D] float32 is needed')
    if K < 1 or K > max_k():
        raise ValueError('hmm.accumulate: K = %d, the kernel takes 1 .. %d (abn_hmm_max_k)' % (K, max_k()))
    if not 0 <= int(n_ranges) <= 256:
        raise ValueError('hmm.accumulate: n_ranges = %r, 0 (chosen from the grid) .. 256' % (n_ranges,))
    table = _gmm._check_table('hmm.accumulate', table)
    _lib.require_device(post, shift)
    sums = torch.zeros((K, 2 * D + 1), dtype=torch.float64, device=table.device)
    if T:
        need = lib.abn_hmm_accumulate_ws_bytes(T, K, D, int(n_ranges))
        if need < 0:
            raise ValueError('hmm.accumulate: %s' % lib.abn_last_error().decode('utf-8', 'replace'))
        ws = torch.empty(max(int(need), 16), dtype=torch.uint8, device=table.device)
        _lib.check(lib.abn_hmm_accumulate(_lib.ptr(table), T, D, _lib.ptr(shift), _lib.ptr(post), K, int(n_ranges),
                                          _lib.ptr(sums), _lib.ptr(ws), ws.numel(), _lib.stream()), 'abn_hmm_accumulate')
    return sums


def baum_welch_update(sums, stay_k_total, n_trans, means, variances, gv, var_floor=0.01, min_count=1.0, params=PARAMS,
                      weights=None, stay=None, stays_total=None):
    """The M-step of the module docstring on the host, float64: (weights, means, variances, stay, n_retired).
    sums [K, 2D + 1] = [S1 | S2 | N] and stay_k_total [K] are the corpus totals, n_trans = sum_u max(n_good_u - 1, 0);
    means are centred (mean - shift), as the statistics are.  A parameter whose letter is not in `params` comes back
    as given: `weights` and `stay` are the current ones (needed when held fixed).  stays_total: the kernel's own sum of
    the stays, used for the stay instead of sum_k stay_k when given (``fit_stay``'s number).  The returned stay is a
    float32 value that passes check_stay with the returned weights, or ValueError."""
    who = 'hmm.baum_welch_update'
    p = check_params(who, params)
    sums = np.asarray(sums, dtype=np.float64)
    m, v = np.array(means, dtype=np.float64), np.array(variances, dtype=np.float64)
    K, D = m.shape
    sk = np.asarray(stay_k_total, dtype=np.float64)
    if sums.shape != (K, 2 * D + 1) or v.shape != (K, D) or sk.shape != (K,) or np.shape(gv) != (D,):
        raise ValueError('%s: sums [K, 2D + 1], stay_k_total [K], means and variances [K, D], gv [D] are needed' % who)
    N, S1, S2 = sums[:, 2 * D], sums[:, :D], sums[:, D:2 * D]
    keep = (N < min_count)[:, None]                      # a starved component keeps its mean and variance
    floor = float(var_floor) * np.asarray(gv, dtype=np.float64)[None, :]
    with np.errstate(all='ignore'):
        m1 = S1 / N[:, None]
        if 'v' in p:
            raw = S2 / N[:, None] - m1 * m1 if 'm' in p else S2 / N[:, None] - 2.0 * m * m1 + m * m
            v = np.where(keep, v, np.maximum(raw, floor))
        if 'm' in p:
            m = np.where(keep, m, m1)
    if 'w' in p:
        draws = np.maximum(N - sk, 0.0)
        if not np.isfinite(draws).all() or not draws.sum() > 0:
            raise ValueError('%s: the expected draws are not finite or all 0' % who)
        w = draws / draws.sum()
        w[w < WEIGHT_MIN] = 0.0
        w = w / w.sum()
    else:
        if weights is None:
            raise ValueError('%s: the current weights are needed when params has no w' % who)
        w = np.array(weights, dtype=np.float64)
    if 's' in p:
        if n_trans < 1:
            raise ValueError('%s: no utterance has two good frames: the stay probability cannot be estimated' % who)
        num = float(sk.sum()) if stays_total is None else float(stays_total)
        stay = min(max(num / float(n_trans), 0.0), STAY_MAX)
    elif stay is None:
        raise ValueError('%s: the current stay is needed when params has no s' % who)
    return w, m, v, check_stay(who, stay, w.astype(np.float32)), int((w == 0).sum())


def stay_update(stays, n_good):
    """The EM update of rho from the utterances' expected stays and good-frame counts (host or device arrays)."""
    host = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    trans = np.maximum(host(n_good).astype(np.int64) - 1, 0).sum()
    if trans < 1:
        raise ValueError('hmm: no utterance has two good frames: the stay probability cannot be estimated')
    return float(min(max(host(stays).astype(np.float64).sum() / float(trans), 0.0), STAY_MAX))


def dense_max_k():
    return int(_lib.load().abny_hmm_dense_max_k())


def check_transitions(who, init, trans):
    """(init [K], trans [K, K]) as float32 host arrays, or ValueError: finite, every entry at least 2^-100 (as float32),
    and init and every row of trans summing to 1 within 1e-3."""
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    try:
        i32, t32 = host(init).astype(np.float32), host(trans).astype(np.float32)
    except (TypeError, ValueError):
        raise ValueError('%s: init [K] and trans [K, K] arrays of numbers are needed' % who)
    if i32.ndim != 1 or t32.shape != (len(i32), len(i32)) or not len(i32):
        raise ValueError('%s: init [K] and trans [K, K] are needed, not %s and %s' % (who, i32.shape, t32.shape))
    if not (np.isfinite(i32).all() and np.isfinite(t32).all()):
        raise ValueError('%s: init and trans must be finite' % who)
    low = min(float(i32.min()), float(t32.min()))
    if low < TINY:
        raise ValueError('%s: the smallest entry of init and trans is %g, below 2^-100: the scaled recursion would underflow'
                         % (who, low))
    sums = np.concatenate([[i32.astype(np.float64).sum()], t32.astype(np.float64).sum(axis=1)])
    if np.abs(sums - 1.0).max() > 1e-3:
        raise ValueError('%s: init and every row of trans must sum to 1 (the worst is off by %g)' % (who, np.abs(sums - 1.0).max()))
    return i32, t32


def sticky_transitions(w, stay):
    """(init, trans) float32 of the sticky model over weights w: init = float32(w), trans[j][k] = r [j == k] + (1 - r) w32[k]
    with r = float32(stay) and 1 - r taken in float32, formed in float64 and rounded once.  ValueError naming the
    components if a weight is 0 (the full-transition model has no retired components), and through check_stay."""
    w32 = np.asarray(w, dtype=np.float32).ravel()
    r = np.float32(check_stay('hmm.sticky_transitions', stay, w32))
    if (w32 <= 0).any():
        raise ValueError('hmm.sticky_transitions: the components %s have weight 0; a full transition matrix needs every entry '
                         '>= 2^-100' % np.flatnonzero(w32 <= 0).tolist())
    omr = np.float32(1.0) - r
    trans = np.float64(omr) * w32.astype(np.float64)[None, :] + np.float64(r) * np.eye(len(w32))
    return w32.copy(), trans.astype(np.float32)


def dense_forward_backward(table, off, lens, shift, A, B, c0, init, trans, mode='smooth', out=None, want_stats=False):
    """(post [T, K] fp32, loglik [n_utt] float64, n_good [n_utt] int32[, stats [K + 1, K] float64]), device tensors, of the
    full-transition recursion the module docstring defines (abny_hmm_dense_forward_backward: one launch, and a second
    small one for the statistics).  off, lens: the utterances' first rows and lengths (host sequences or device tensors);
    they must not overlap.  init [K], trans [K, K]: float32 device tensors.  Rows outside every utterance keep what `out`
    held (0 in a fresh table).  stats: rows 0 .. K - 1 the expected transition counts xi, row K `first`."""
    lib = _lib.load()
    who = 'hmm.dense_forward_backward'
    if mode not in MODES:
        raise ValueError('%s: mode = %r, one of %s' % (who, mode, sorted(MODES)))
    T, D, K = _emission_shapes(who, table, shift, A, B, c0)
    if not isinstance(init, torch.Tensor) or not isinstance(trans, torch.Tensor) or init.shape != (K,) or trans.shape != (K, K) or \
            init.dtype != torch.float32 or trans.dtype != torch.float32:
        raise ValueError('%s: init [K] and trans [K, K] float32 tensors are needed' % who)
    if K < 1 or K > dense_max_k():
        raise ValueError('%s: K = %d, the kernel takes 1 .. %d (abny_hmm_dense_max_k)' % (who, K, dense_max_k()))
    check_transitions(who, init, trans)
    off_h, len_h, n_utt, longest = _utt.utterance_spans(who, off, lens, T, max_len(), 'abn_hmm_max_len')
    table = _gmm._check_table(who, table)
    _lib.require_device(shift, A, B, c0, init, trans)
    out = _utt.posterior_table(who, out, T, K, table.device)
    ll = torch.zeros(n_utt, dtype=torch.float64, device=table.device)
    ng = torch.zeros(n_utt, dtype=torch.int32, device=table.device)
    stats = torch.zeros((K + 1, K), dtype=torch.float64, device=table.device) if want_stats else None
    if T and n_utt and longest:
        ws, off_d, len_d = _utt.workspace(who, lib.abny_hmm_dense_ws_bytes, off_h, len_h, longest, K, D, table.device)
        _lib.check(lib.abny_hmm_dense_forward_backward(
            _lib.ptr(table), T, D, _lib.ptr(off_d), _lib.ptr(len_d), n_utt, _lib.ptr(shift), _lib.ptr(A), _lib.ptr(B), _lib.ptr(c0),
            _lib.ptr(init), _lib.ptr(trans), K, MODES[mode], _lib.ptr(out), _lib.ptr(ll), _lib.ptr(ng), _lib.ptr(stats),
            _lib.ptr(ws), ws.numel(), _lib.stream()), 'abny_hmm_dense_forward_backward')
    return (out, ll, ng, stats) if want_stats else (out, ll, ng)


def log_transitions(init, trans):
    """(li [K], lt [K, K]) float32: the log tables of the full-transition model's max-product path (module docstring),
    computed on the host in float64 from float32(init), float32(trans) and rounded once.  ValueError through
    check_transitions (finite, every entry >= 2^-100, rows summing to 1): every logarithm is finite."""
    i32, t32 = check_transitions('hmm.log_transitions', init, trans)
    return np.log(i32.astype(np.float64)).astype(np.float32), np.log(t32.astype(np.float64)).astype(np.float32)


def _check_dense_log_tables(who, li, lt, K):
    """The host checks of li [K] and lt [K, K]: float32 tensors that hold no NaN and no infinity."""
    if not isinstance(li, torch.Tensor) or not isinstance(lt, torch.Tensor) or li.shape != (K,) or lt.shape != (K, K) or \
            li.dtype != torch.float32 or lt.dtype != torch.float32:
        raise ValueError('%s: li [K] and lt [K, K] float32 tensors are needed (hmm.log_transitions)' % who)
    a, b = li.detach().cpu().numpy(), lt.detach().cpu().numpy()
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        raise ValueError('%s: the log tables must not hold NaN, +inf or -inf (every entry of init and trans is >= 2^-100)' % who)


def _dense_viterbi_sizing(lib, min_duration):
    """The *_ws_bytes entry of the decoder ``_dense_viterbi_launch`` runs for this min_duration."""
    return lib.abnz_hmm_dense_viterbi_ws_bytes if min_duration == 1 else lib.abnw_hmm_dense_viterbi_dur_ws_bytes


def _dense_viterbi_launch(lib, table, off_d, len_d, n_utt, shift, A, B, c0, li, lt, K, ids, lp, nsw, ng, min_duration, ws):
    """abnz_hmm_dense_viterbi (min_duration 1) or abnw_hmm_dense_viterbi_dur on checked arguments and a workspace of
    ``_dense_viterbi_sizing``'s entry; fills ids, lp, nsw (either may be None) and ng."""
    T, D = table.shape
    args = (_lib.ptr(table), T, D, _lib.ptr(off_d), _lib.ptr(len_d), n_utt, _lib.ptr(shift), _lib.ptr(A), _lib.ptr(B),
            _lib.ptr(c0), _lib.ptr(li), _lib.ptr(lt), K, _lib.ptr(ids), _lib.ptr(lp), _lib.ptr(nsw), _lib.ptr(ng),
            _lib.ptr(ws), ws.numel(), _lib.stream())
    if min_duration == 1:
        _lib.check(lib.abnz_hmm_dense_viterbi(*args), 'abnz_hmm_dense_viterbi')
    else:
        _lib.check(lib.abnw_hmm_dense_viterbi_dur(*(args + (min_duration,))), 'abnw_hmm_dense_viterbi_dur')


def dense_viterbi(table, off, lens, shift, A, B, c0, li, lt, ids=None, want_log_prob=True, min_duration=1):
    """(ids [T] int32, log_prob [n_utt] float64 or None, n_switch [n_utt] int32 or None, n_good [n_utt] int32), device
    tensors, of the full-transition max-product recurrence the module docstring defines (abnz_hmm_dense_viterbi, one
    launch).  off, lens: the utterances' first rows and lengths (host sequences or device tensors); they must not overlap.
    li, lt: the log tables of ``log_transitions``.  Rows outside every utterance keep what `ids` held (-1 in a fresh
    `ids`).  min_duration = S > 1: every unit lasts at least S good frames (abnw_hmm_dense_viterbi_dur, a workspace of its
    own geometry); 1 is exactly the call without it."""
    lib = _lib.load()
    who = 'hmm.dense_viterbi'
    min_duration = _utt.check_min_duration(who, min_duration)
    T, D, K = _emission_shapes(who, table, shift, A, B, c0)
    if K < 1 or K > dense_max_k():
        raise ValueError('%s: K = %d, the kernel takes 1 .. %d (abny_hmm_dense_max_k)' % (who, K, dense_max_k()))
    _check_dense_log_tables(who, li, lt, K)
    off_h, len_h, n_utt, longest = _utt.utterance_spans(who, off, lens, T, max_len(), 'abn_hmm_max_len')
    _utt.check_ids(who, ids, T)
    table = _gmm._check_table(who, table)
    _lib.require_device(shift, A, B, c0, li, lt)
    ids, lp, nsw, ng = _utt.path_results(ids, T, n_utt, want_log_prob, table.device)
    if T and n_utt and longest:
        ws, off_d, len_d = _utt.workspace(who, _dense_viterbi_sizing(lib, min_duration), off_h, len_h, longest, K, D, table.device)
        _dense_viterbi_launch(lib, table, off_d, len_d, n_utt, shift, A, B, c0, li, lt, K, ids, lp, nsw, ng, min_duration, ws)
    return ids, lp, nsw, ng


def floor_rows(p):
    """float64: every entry below TRANS_MIN raised to it and each row renormalised once (a vector is one row)."""
    p = np.array(p, dtype=np.float64)
    p[p < TRANS_MIN] = TRANS_MIN
    return p / p.sum(axis=-1, keepdims=True)


def transition_update(stats, trans, init, alpha=1e-3, params='ti'):
    """The transition M-step of the module docstring on the host, float64: (trans [K, K], init [K]) from stats [K + 1, K]
    (rows 0 .. K - 1 xi, row K first) with the pseudo-count alpha >= 0.  A part whose letter (t, i) is not in `params` comes
    back as given; a row without mass at alpha = 0 keeps its old values; then the floor TRANS_MIN and one renormalisation."""
    who = 'hmm.transition_update'
    stats = np.asarray(stats, dtype=np.float64)
    old_t, old_i = np.array(trans, dtype=np.float64), np.array(init, dtype=np.float64)
    K = len(old_i)
    if stats.shape != (K + 1, K) or old_t.shape != (K, K):
        raise ValueError('%s: stats [K + 1, K], trans [K, K] and init [K] are needed' % who)
    if not (isinstance(alpha, (int, float, np.floating, np.integer)) and np.isfinite(alpha) and alpha >= 0):
        raise ValueError('%s: alpha = %r, a number >= 0 is needed' % (who, alpha))
    if not np.isfinite(stats).all() or (stats < 0).any():
        raise ValueError('%s: the statistics are not finite or negative' % who)
    new_t, new_i = old_t, old_i
    if 't' in params:
        den = stats[:K].sum(axis=1) + K * alpha
        with np.errstate(all='ignore'):
            new_t = np.where((den > 0)[:, None], (stats[:K] + alpha) / den[:, None], old_t)
        new_t = floor_rows(new_t)
    if 'i' in params:
        den = stats[K].sum() + K * alpha
        new_i = floor_rows((stats[K] + alpha) / den) if den > 0 else floor_rows(old_i)
    return new_t, new_i


def bigram_counts(ids_by_name, K):
    """int64 [K][K] on the host: the unit bigrams of ``decode`` / ``segment`` output ({name: ids}), BAD frames (-1) passed
    over.  A data-driven start for TransitionHmmPosteriorgram: trans = counts + alpha, each row normalised."""
    K = int(K)
    counts = np.zeros((K, K), dtype=np.int64)
    seqs = ids_by_name.values() if isinstance(ids_by_name, dict) else ids_by_name
    for ids in seqs:
        a = np.asarray(ids).ravel().astype(np.int64)
        a = a[a >= 0]
        if len(a) and a.max() >= K:
            raise ValueError('hmm.bigram_counts: unit id %d with K = %d' % (int(a.max()), K))
        if len(a) > 1:
            np.add.at(counts, (a[:-1], a[1:]), 1)
    return counts


def _hard_stats_launch(lib, table, off_d, len_d, n_utt, shift, ids, K, min_duration, n_ranges, ws):
    """abnv_hmm_hard_stats on checked arguments: (counts, sums, n_good) from torch.empty (the entry clears what it needs)."""
    T, D = table.shape
    counts = torch.empty((K + 1, K), dtype=torch.int64, device=table.device)
    sums = torch.empty((K, 2 * D + 1), dtype=torch.float64, device=table.device)
    ng = torch.empty(n_utt, dtype=torch.int32, device=table.device)
    _lib.check(lib.abnv_hmm_hard_stats(_lib.ptr(table), T, D, _lib.ptr(off_d), _lib.ptr(len_d), n_utt, _lib.ptr(shift), _lib.ptr(ids), K,
                                       min_duration, n_ranges, _lib.ptr(counts), _lib.ptr(sums), _lib.ptr(ng), _lib.ptr(ws), ws.numel(),
                                       _lib.stream()), 'abnv_hmm_hard_stats')
    return counts, sums, ng


def _hard_stats_workspace(who, lib, T, n_utt, K, D, n_ranges, device):
    need = lib.abnv_hmm_hard_stats_ws_bytes(T, n_utt, K, D, n_ranges)
    if need < 0:
        raise ValueError('%s: %s' % (who, lib.abn_last_error().decode('utf-8', 'replace')))
    return torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)


def _check_n_ranges(who, n_ranges):
    if isinstance(n_ranges, bool) or not isinstance(n_ranges, (int, np.integer)) or not 0 <= int(n_ranges) <= 256:
        raise ValueError('%s: n_ranges = %r, an integer 0 (chosen from the grid) .. 256 is needed' % (who, n_ranges))
    return int(n_ranges)


def hard_stats(table, off, lens, shift, ids, K, min_duration=1, n_ranges=0):
    """(counts [K + 1, K] int64, sums [K, 2D + 1] float64, n_good [n_utt] int32), device tensors: the hard statistics the
    module docstring defines, of the unit ids `ids` ([T] int32 on the device; what ``dense_viterbi`` decodes) over the
    utterances off, lens of the [T, D] table (abnv_hmm_hard_stats: three launches).  counts: rows 0 .. K - 1 the transition
    counts of the chain ``dense_viterbi(min_duration=S)`` decodes (at S = 1 ``bigram_counts``), row K the utterances' first
    units -- ``transition_update``'s stats.  sums = [S1 | S2 | N] -- ``baum_welch_update``'s.  An id outside 0 .. K - 1 is a BAD
    frame; rows outside every utterance contribute nothing.  n_ranges: as in ``accumulate``."""
    lib = _lib.load()
    who = 'hmm.hard_stats'
    min_duration = _utt.check_min_duration(who, min_duration)
    n_ranges = _check_n_ranges(who, n_ranges)
    T, D = _utt.table_shape(who, table)
    if not isinstance(shift, torch.Tensor) or shift.shape != (D,) or shift.dtype != torch.float32:
        raise ValueError('%s: shift [D] float32 is needed' % who)
    if not isinstance(ids, torch.Tensor) or ids.shape != (T,) or ids.dtype != torch.int32 or not ids.is_contiguous():
        raise ValueError('%s: ids must be a contiguous [T] int32 tensor, one id per row of the table' % who)
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= int(K) <= dense_max_k():
        raise ValueError('%s: K = %r, the kernel takes 1 .. %d (abny_hmm_dense_max_k)' % (who, K, dense_max_k()))
    K = int(K)
    if D < 1 or D > int(lib.abn_gmm_max_d()):
        raise ValueError('%s: D = %d, the kernel takes 1 .. %d (abn_gmm_max_d)' % (who, D, int(lib.abn_gmm_max_d())))
    off_h, len_h, n_utt, longest = _utt.utterance_spans(who, off, lens, T, max_len(), 'abn_hmm_max_len')
    table = _gmm._check_table(who, table)
    _lib.require_device(shift, ids)
    if not (T and n_utt):
        return (torch.zeros((K + 1, K), dtype=torch.int64, device=table.device),
                torch.zeros((K, 2 * D + 1), dtype=torch.float64, device=table.device),
                torch.zeros(n_utt, dtype=torch.int32, device=table.device))
    ws = _hard_stats_workspace(who, lib, T, n_utt, K, D, n_ranges, table.device)
    off_d, len_d = torch.from_numpy(off_h).to(table.device), torch.from_numpy(len_h.astype(np.int32)).to(table.device)
    return _hard_stats_launch(lib, table, off_d, len_d, n_utt, shift, ids, K, min_duration, n_ranges, ws)


def check_dense_params(who, params):
    """The letters of `params` as a set, or ValueError: a non-empty string over 'mvti' without a repeat."""
    if not isinstance(params, str) or not params or len(set(params)) != len(params) or not set(params) <= set(DENSE_PARAMS):
        raise ValueError('%s: params = %r, a non-empty choice of the letters of %r is needed '
                         '(m means, v variances, t transitions, i init)' % (who, params, DENSE_PARAMS))
    return set(params)


# ---- explicit unit durations (the module docstring's semi-Markov decoder) -------------------------------------------------
def hsmm_max_duration():
    return int(_lib.load().abnu_hmm_hsmm_max_duration())


def check_max_duration(who, L):
    """L as an int, or ValueError: an integer 2 .. HSMM_MAX_DURATION."""
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or not 2 <= int(L) <= HSMM_MAX_DURATION:
        raise ValueError('%s: max_duration = %r, an integer 2 .. %d is needed (abnu_hmm_hsmm_max_duration)'
                         % (who, L, HSMM_MAX_DURATION))
    return int(L)


def check_hsmm_params(who, params):
    """The letters of `params` as a set, or ValueError: a non-empty string over 'mvtid' without a repeat."""
    if not isinstance(params, str) or not params or len(set(params)) != len(params) or not set(params) <= set(HSMM_PARAMS):
        raise ValueError('%s: params = %r, a non-empty choice of the letters of %r is needed '
                         '(m means, v variances, t transitions, i init, d durations)' % (who, params, HSMM_PARAMS))
    return set(params)


def check_durations(who, q, r):
    """(q [K, L], r [K]) as float64 host arrays, or ValueError: finite, every q, r and 1 - r at least 2^-100, L within
    2 .. HSMM_MAX_DURATION and every row of q summing to 1 within 1e-3."""
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    try:
        q64, r64 = host(q).astype(np.float64), host(r).astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError('%s: q [K, L] and r [K] arrays of numbers are needed' % who)
    if q64.ndim != 2 or r64.shape != (q64.shape[0],) or not q64.shape[0]:
        raise ValueError('%s: q [K, L] and r [K] are needed, not %s and %s' % (who, q64.shape, r64.shape))
    check_max_duration(who, q64.shape[1])
    if not (np.isfinite(q64).all() and np.isfinite(r64).all()):
        raise ValueError('%s: q and r must be finite' % who)
    low = min(float(q64.min()), float(r64.min()), float((1.0 - r64).min()))
    if low < TINY:
        raise ValueError('%s: the smallest of q, r and 1 - r is %g, below 2^-100: a log table would not be finite' % (who, low))
    off = np.abs(q64.sum(axis=1) - 1.0).max()
    if off > 1e-3:
        raise ValueError('%s: every row of q must sum to 1 (the worst is off by %g)' % (who, off))
    return q64, r64


def geometric_durations(trans, L):
    """(q [K, L], r [K]) float64: the duration law under which the semi-Markov model IS the plain full-transition model
    (up to the utterance's last segment, which the semi-Markov score closes): r[k] = trans[k][k], q[k][d] = (1 - r) r^(d-1)
    for d < L and q[k][L] = r^(L-1)."""
    L = check_max_duration('hmm.geometric_durations', L)
    t = np.asarray(trans.detach().cpu().numpy() if isinstance(trans, torch.Tensor) else trans, dtype=np.float64)
    if t.ndim != 2 or t.shape[0] != t.shape[1] or not t.shape[0]:
        raise ValueError('hmm.geometric_durations: trans [K, K] is needed, not %s' % (t.shape,))
    r = np.diag(t).copy()
    if not np.isfinite(r).all() or (r <= 0).any() or (r >= 1).any():
        raise ValueError('hmm.geometric_durations: every trans[k][k] must lie inside (0, 1)')
    q = np.empty((len(r), L), dtype=np.float64)
    q[:, :L - 1] = (1.0 - r)[:, None] * r[:, None] ** np.arange(L - 1)[None, :]
    q[:, L - 1] = r ** (L - 1)
    return q, r


def duration_tables(q, r):
    """(ld [K, L], ls [K]) float32: ld[k][i-1] = log q[k][i] for i < L, ld[k][L-1] = log(q[k][L] (1 - r[k])), ls[k] = log r[k],
    float64 logarithms rounded once.  ValueError through check_durations: every entry is finite."""
    q64, r64 = check_durations('hmm.duration_tables', q, r)
    ld = np.log(q64)
    ld[:, -1] = np.log(q64[:, -1] * (1.0 - r64))
    return np.ascontiguousarray(ld.astype(np.float32)), np.log(r64).astype(np.float32)


def switch_log_transitions(init, trans):
    """(li [K], lx [K, K]) float32: li as ``log_transitions`` gives it, lx[j][k] = log(trans[j][k] / (1 - trans[j][j])) for
    j != k -- where the chain goes GIVEN that it leaves j --, float64 from float32(init), float32(trans), rounded once.  The
    diagonal of lx is never read and holds 0.  Where float32(trans[j][j]) is so near 1 that 1 - trans[j][j] is below 2^-100
    (a unit the training data never leaves, its other entries at the floor), the row's off-diagonal sum stands for it: the
    same quantity for a stochastic row, and never 0.  ValueError through check_transitions."""
    who = 'hmm.switch_log_transitions'
    i32, t32 = check_transitions(who, init, trans)
    t = t32.astype(np.float64)
    K = len(i32)
    leave = 1.0 - np.diag(t)
    leave = np.where(leave >= TINY, leave, np.where(np.eye(K, dtype=bool), 0.0, t).sum(axis=1))
    with np.errstate(all='ignore'):
        lx = np.log(t / np.where(leave > 0, leave, 1.0)[:, None])        # (leave is 0 only for K = 1, whose lx is all diagonal)
    lx[np.arange(K), np.arange(K)] = 0.0
    return np.log(i32.astype(np.float64)).astype(np.float32), np.ascontiguousarray(lx.astype(np.float32))


def _check_hsmm_log_tables(who, li, lx, ld, ls, K):
    """The host checks of the four log tables: float32 tensors of the right shapes that hold no NaN and no infinity.
    Returns L."""
    ok = all(isinstance(a, torch.Tensor) and a.dtype == torch.float32 for a in (li, lx, ld, ls))
    if not ok or li.shape != (K,) or lx.shape != (K, K) or ls.shape != (K,) or ld.dim() != 2 or ld.shape[0] != K:
        raise ValueError('%s: li [K], lx [K, K], ld [K, L] and ls [K] float32 tensors are needed (hmm.switch_log_transitions, '
                         'hmm.duration_tables)' % who)
    L = check_max_duration(who, int(ld.shape[1]))
    if not all(np.isfinite(a.detach().cpu().numpy()).all() for a in (li, lx, ld, ls)):
        raise ValueError('%s: the log tables must not hold NaN, +inf or -inf' % who)
    return L


def _hsmm_viterbi_launch(lib, table, off_d, len_d, n_utt, shift, A, B, c0, li, lx, ld, ls, K, L, ids, lp, nsw, ng, ws):
    """abnu_hmm_hsmm_viterbi on checked arguments and a workspace of abnu_hmm_hsmm_viterbi_ws_bytes."""
    T, D = table.shape
    _lib.check(lib.abnu_hmm_hsmm_viterbi(
        _lib.ptr(table), T, D, _lib.ptr(off_d), _lib.ptr(len_d), n_utt, _lib.ptr(shift), _lib.ptr(A), _lib.ptr(B), _lib.ptr(c0),
        _lib.ptr(li), _lib.ptr(lx), K, _lib.ptr(ids), _lib.ptr(lp), _lib.ptr(nsw), _lib.ptr(ng), _lib.ptr(ws), ws.numel(),
        _lib.stream(), _lib.ptr(ld), _lib.ptr(ls), L), 'abnu_hmm_hsmm_viterbi')


def hsmm_viterbi(table, off, lens, shift, A, B, c0, li, lx, ld, ls, ids=None, want_log_prob=True):
    """(ids [T] int32, log_prob [n_utt] float64 or None, n_switch [n_utt] int32 or None, n_good [n_utt] int32), device
    tensors, of the semi-Markov recurrence the module docstring defines (abnu_hmm_hsmm_viterbi, one launch): ``dense_viterbi``
    with explicit unit durations.  li, lx: ``switch_log_transitions``; ld [K, L], ls [K]: ``duration_tables``; L is ld's width.
    Everything else as in ``dense_viterbi``."""
    lib = _lib.load()
    who = 'hmm.hsmm_viterbi'
    T, D, K = _emission_shapes(who, table, shift, A, B, c0)
    if K < 1 or K > dense_max_k():
        raise ValueError('%s: K = %d, the kernel takes 1 .. %d (abny_hmm_dense_max_k)' % (who, K, dense_max_k()))
    L = _check_hsmm_log_tables(who, li, lx, ld, ls, K)
    off_h, len_h, n_utt, longest = _utt.utterance_spans(who, off, lens, T, max_len(), 'abn_hmm_max_len')
    _utt.check_ids(who, ids, T)
    table = _gmm._check_table(who, table)
    _lib.require_device(shift, A, B, c0, li, lx, ld, ls)
    ids, lp, nsw, ng = _utt.path_results(ids, T, n_utt, want_log_prob, table.device)
    if T and n_utt and longest:
        sizing = lambda n, m, k, d: lib.abnu_hmm_hsmm_viterbi_ws_bytes(n, m, k, d, L)
        ws, off_d, len_d = _utt.workspace(who, sizing, off_h, len_h, longest, K, D, table.device)
        _hsmm_viterbi_launch(lib, table, off_d, len_d, n_utt, shift, A, B, c0, li, lx, ld, ls, K, L, ids, lp, nsw, ng, ws)
    return ids, lp, nsw, ng


def _run_stats_launch(lib, ids, off_d, len_d, n_utt, K, L):
    """abnu_hmm_run_stats on checked arguments: (dur, tail) from torch.empty (the entry clears them)."""
    dur = torch.empty((K, L), dtype=torch.int64, device=ids.device)
    tail = torch.empty(K, dtype=torch.int64, device=ids.device)
    _lib.check(lib.abnu_hmm_run_stats(_lib.ptr(ids), ids.shape[0], _lib.ptr(off_d), _lib.ptr(len_d), n_utt, K, L, _lib.ptr(dur),
                                      _lib.ptr(tail), _lib.stream()), 'abnu_hmm_run_stats')
    return dur, tail


def run_stats(ids, off, lens, K, L):
    """(dur [K, L] int64, tail [K] int64), device tensors: the run statistics of the unit ids `ids` ([T] int32 on the device)
    over the utterances off, lens (abnu_hmm_run_stats, one launch).  For every maximal run, over an utterance's good frames,
    of unit k with length n: dur[k][min(n, L) - 1] += 1 and tail[k] += max(n - L, 0).  An id outside 0 .. K - 1 is a BAD
    frame and is passed over; rows outside every utterance count nothing."""
    lib = _lib.load()
    who = 'hmm.run_stats'
    if not isinstance(ids, torch.Tensor) or ids.dim() != 1 or ids.dtype != torch.int32 or not ids.is_contiguous():
        raise ValueError('%s: ids must be a contiguous [T] int32 tensor' % who)
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= int(K) <= dense_max_k():
        raise ValueError('%s: K = %r, the kernel takes 1 .. %d (abny_hmm_dense_max_k)' % (who, K, dense_max_k()))
    K, L = int(K), check_max_duration(who, L)
    T = ids.shape[0]
    off_h, len_h, n_utt, _ = _utt.utterance_spans(who, off, lens, T, max_len(), 'abn_hmm_max_len')
    _lib.require_device(ids)
    if not (T and n_utt):
        return torch.zeros((K, L), dtype=torch.int64, device=ids.device), torch.zeros(K, dtype=torch.int64, device=ids.device)
    off_d, len_d = torch.from_numpy(off_h).to(ids.device), torch.from_numpy(len_h.astype(np.int32)).to(ids.device)
    return _run_stats_launch(lib, ids, off_d, len_d, n_utt, K, L)


def duration_update(dur, tail, q, r, alpha=1e-3):
    """The duration M-step of the module docstring on the host, float64: (q [K, L], r [K]) from the run statistics with the
    pseudo-count alpha >= 0:  q[k][d] = (dur[k][d] + alpha) / (sum_d dur[k] + L alpha),
    r[k] = (tail[k] + alpha) / (tail[k] + dur[k][L-1] + 2 alpha).  A unit without any run at alpha = 0 keeps its old law (and a
    unit without a run of L or more its old r).  Then every q below TRANS_MIN is raised to it and the row renormalised
    once, and r is kept inside TRANS_MIN .. DUR_TAIL_MAX = 1 - 2^-24 (below 1 as a float32 too)."""
    who = 'hmm.duration_update'
    old_q, old_r = check_durations(who, q, r)
    K, L = old_q.shape
    dur, tail = np.asarray(dur, dtype=np.float64), np.asarray(tail, dtype=np.float64)
    if dur.shape != (K, L) or tail.shape != (K,):
        raise ValueError('%s: dur [K, L] and tail [K] are needed for q [%d, %d]' % (who, K, L))
    if not (isinstance(alpha, (int, float, np.floating, np.integer)) and np.isfinite(alpha) and alpha >= 0):
        raise ValueError('%s: alpha = %r, a number >= 0 is needed' % (who, alpha))
    if not (np.isfinite(dur).all() and np.isfinite(tail).all()) or (dur < 0).any() or (tail < 0).any():
        raise ValueError('%s: the statistics are not finite or negative' % who)
    den = dur.sum(axis=1) + L * alpha
    rden = tail + dur[:, L - 1] + 2.0 * alpha
    with np.errstate(all='ignore'):
        new_q = np.where((den > 0)[:, None], (dur + alpha) / den[:, None], old_q)
        new_r = np.where(rden > 0, (tail + alpha) / rden, old_r)
    return floor_rows(new_q), np.clip(new_r, TRANS_MIN, DUR_TAIL_MAX)


class _MixtureHmm(object):
    """What the two models over a fitted GmmPosteriorgram share: the emission tables, the corpus plumbing of transform /
    score / decode / quantize, the scaffold of the training loops and the mixture's part of the file.  A subclass supplies
    ``_forward_backward(table, lens, mode) -> (post, loglik, n_good)`` and
    ``_max_product(table, lens, min_duration) -> (ids, log_prob, n_switch, n_good)``, device tensors of its own chain.
    The messages name the subclass."""

    def __init__(self, gmm):
        if not isinstance(gmm, _gmm.GmmPosteriorgram) or gmm.weights_ is None:
            raise ValueError('%s: a fitted GmmPosteriorgram is needed' % type(self).__name__)
        self.gmm = gmm
        self.log_likelihoods = []
        self.n_bad_ = self.n_starved_ = 0
        self.last_log_prob_ = self.last_n_switch_ = self.last_n_good_ = None
        self._tables = None

    def _emission_tables(self, device):
        """(shift, A, B, c0) on the device, rounded once from the mixture's float64 parameters."""
        g = self.gmm
        shift, A, B, _ = g.device_tables(device)
        m = g.means_ - g.shift_.astype(np.float64)
        return shift, A, B, torch.from_numpy(emission_offsets(m, g.variances_)).to(device)

    def _utterances(self, corpus):
        """(device table, DeviceCorpus or None, lens int64 [n_utt])"""
        who = type(self).__name__
        table, dc = _gmm.GmmPosteriorgram._corpus(corpus)
        if dc is not None:
            lens = [dc.length[k] for k in dc.names]
        elif isinstance(corpus, dict):
            lens = [np.asarray(f).shape[0] for f in corpus.values()]
        else:
            lens = [table.shape[0]] if isinstance(table, torch.Tensor) and table.dim() == 2 else []
        if isinstance(table, torch.Tensor) and table.dim() == 2 and table.dtype == torch.float32:      # (host checks first)
            if table.shape[1] != self.gmm.shift_.shape[0]:
                raise ValueError('%s: the table has D = %d, the model D = %d' % (who, table.shape[1], self.gmm.shift_.shape[0]))
            if len(lens) and max(lens) > max_len():
                raise ValueError('%s: an utterance of %d frames, the kernel takes up to %d '
                                 '(abn_hmm_max_len); pass a corpus of utterances' % (who, max(lens), max_len()))
        table = _gmm._check_table(who, table)
        return table, dc, np.asarray(lens, dtype=np.int64)

    @staticmethod
    def _like(dc, out):
        """A table of one row per frame as the corpus came: for a DeviceCorpus a new one with its names, lengths and times."""
        from .dataloader import DeviceCorpus
        return out if dc is None else DeviceCorpus.from_table(out, dc.names, [dc.length[k] for k in dc.names], dc.times)

    def transform(self, corpus, mode='smooth'):
        """The smoothed (mode='filter': filtered) posterior table [rows, K] on the device; for a DeviceCorpus a new
        DeviceCorpus with the same names, lengths and times."""
        table, dc, lens = self._utterances(corpus)
        return self._like(dc, self._forward_backward(table, lens, mode)[0])

    def score(self, corpus):
        """The mean log-likelihood per good frame."""
        table, _, lens = self._utterances(corpus)
        _, ll, ng = self._forward_backward(table, lens, 'filter')
        ll_sum, n = torch.stack([ll.sum(), ng.to(torch.float64).sum()]).cpu().tolist()
        return ll_sum / max(1.0, n)

    def _decode_ids(self, corpus, min_duration=1, **how):
        """(device ids [rows] int32, DeviceCorpus or None, names or None, lens); fills last_log_prob_ / last_n_switch_ /
        last_n_good_ / n_bad_.  `how`: what a subclass's ``_max_product`` takes beside the minimum duration."""
        min_duration = _utt.check_min_duration(type(self).__name__, min_duration)
        table, dc, lens = self._utterances(corpus)
        names = list(dc.names) if dc is not None else list(corpus) if isinstance(corpus, dict) else None
        ids, lp, nsw, ng = self._max_product(table, lens, min_duration, **how)
        self.last_log_prob_, self.last_n_switch_, self.last_n_good_ = lp.cpu().numpy(), nsw.cpu().numpy(), ng.cpu().numpy()
        self.n_bad_ = int(lens.sum() - self.last_n_good_.sum())
        return ids, dc, names, lens

    def decode(self, corpus, min_duration=1, **how):
        """The unit ids of the model's best path, int32, -1 for a BAD frame: {name: host array [length]} in corpus order for
        a DeviceCorpus, a dict or a file; for a [T, D] table, which is ONE utterance, the device tensor [T].  The
        subclasses' docstrings say what each one's path and ``last_*_`` are."""
        ids, _, names, lens = self._decode_ids(corpus, min_duration, **how)
        return ids if names is None else _gmm._split_rows(ids.cpu().numpy(), zip(names, lens))

    def quantize(self, corpus, min_duration=1, **how):
        """Each frame replaced by the mean of its decoded component (uncentred: m + shift), [rows, D] float32 on the
        device, a BAD frame a row of zeros; for a DeviceCorpus a new DeviceCorpus with the same names, lengths and times
        (what KMeansQuantizer.quantize gives ``ABXEvaluator(parallel='zero')``).  min_duration (and, for the full-transition
        model, durations=True): as in ``decode``."""
        ids, dc, _, _ = self._decode_ids(corpus, min_duration, **how)
        means = torch.from_numpy(self.gmm.means_.astype(np.float32)).to(ids.device)
        out = means[ids.clamp(min=0).to(torch.int64)]
        out[ids < 0] = 0.0
        return self._like(dc, out)

    # -- training: the scaffold of the fit loops ------------------------------------------------------------------
    def _training_copy(self, device):
        """(g, shift64, dev, shift): a copy of the mixture with float64 parameters of its own (the GmmPosteriorgram this
        object was made from stays untouched), its shift in float64, the float32 uploader and the shift on the device."""
        g = copy.copy(self.gmm)
        g.weights_, g.means_, g.variances_ = (np.array(a, dtype=np.float64) for a in (g.weights_, g.means_, g.variances_))
        g.log_likelihoods, g._tables = list(g.log_likelihoods), None
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
        return g, g.shift_.astype(np.float64), dev, dev(g.shift_)

    def _adopt(self, g, p, shift64, m, v, w=None):
        """The trained copy becomes ``self.gmm``, with those of the centred means m, variances v and weights w that the
        letters p name."""
        if 'w' in p:
            g.weights_ = w
        if 'm' in p:
            g.means_ = m + shift64
        if 'v' in p:
            g.variances_ = v
        self.gmm, self._tables = g, None

    # -- files ----------------------------------------------------------------------------------------------------
    def _mixture_fields(self):
        """The arrays of the mixture's own file (GmmPosteriorgram.load reads them), for ``save``."""
        g = self.gmm
        return dict(weights=g.weights_, means=g.means_, variances=g.variances_, shift=g.shift_, gv=g.gv_,
                    log_likelihoods=np.asarray(g.log_likelihoods, dtype=np.float64),
                    n_components=g.n_components, n_iter=g.n_iter, tol=g.tol, var_floor=g.var_floor,
                    min_count=g.min_count, seed=g.seed)


class StickyHmmPosteriorgram(_MixtureHmm):
    """transform / decode / quantize / score / fit_stay / fit of the sticky HMM the module docstring defines, over a fitted GmmPosteriorgram.

    corpus arguments: a DeviceCorpus, a {name: [T, D]} dict, the path of an h5features file -- each file an utterance --
    or a [T, D] float32 device table, which is ONE utterance."""

    def __init__(self, gmm, stay=0.9):
        super().__init__(gmm)
        self.stay_ = check_stay('StickyHmmPosteriorgram', stay, gmm.weights_.astype(np.float32))
        self.n_retired_ = 0

    def whoami(self):
        return {'params': {'stay': self.stay_, 'gmm': self.gmm.whoami()}, 'class_name': self.__class__.__name__}

    def device_tables(self, device):
        """(shift, A, B, c0, w32) on the device, rounded once from the mixture's float64 parameters."""
        if self._tables is None or self._tables[0].device != device:
            w = torch.from_numpy(self.gmm.weights_.astype(np.float32)).to(device)
            self._tables = self._emission_tables(device) + (w,)
        return self._tables

    def _run(self, table, lens, mode, stay=None, out=None, want_stays=True):
        off = _utt.starts(lens)
        return forward_backward(table, off, lens, *self.device_tables(table.device),
                                stay=self.stay_ if stay is None else stay, mode=mode, out=out, want_stays=want_stays)

    def _forward_backward(self, table, lens, mode):
        post, ll, _, ng = self._run(table, lens, mode, want_stays=False)
        return post, ll, ng

    def _max_product(self, table, lens, min_duration):
        shift, A, B, c0, w = self.device_tables(table.device)
        lw, ls, lr = (torch.from_numpy(a).to(table.device) for a in viterbi_tables(self.gmm.weights_, self.stay_))
        return viterbi(table, _utt.starts(lens), lens, shift, A, B, c0, lw, ls, lr, min_duration=min_duration)

    def decode(self, corpus, min_duration=1):
        """The unit ids of the best path (the module docstring's max-product recurrence), int32, -1 for a BAD frame:
        {name: host array [length]} in corpus order for a DeviceCorpus, a dict or a file -- what KMeansQuantizer.segment
        returns, so kmeans.unit_sequences / bitrate / segments, eskmeans.landmarks_from_units and tde.unit_boundaries take
        it as it is --; for a [T, D] table, which is ONE utterance, the device tensor [T].  ``last_log_prob_`` (float64),
        ``last_n_switch_`` and ``last_n_good_`` (int32) hold the utterances' log joint probabilities, switch counts and
        good-frame counts; ``n_bad_`` the BAD frames.  min_duration = S (an integer 1 .. 8): every unit but an
        utterance's last lasts at least S good frames (the module docstring's minimum-duration recurrence)."""
        return super().decode(corpus, min_duration)

    def fit_stay(self, corpus, n_iter=10, tol=1e-4):
        """EM on the stay probability, the mixture fixed, from the current ``stay_``.  Iteration i runs forward-backward
        under the current stay -- ``log_likelihoods[i]`` is its mean log-likelihood per good frame -- and then applies the
        update.  After at most n_iter iterations, or as soon as log_likelihoods[i] - log_likelihoods[i - 1] < tol, it stops
        (the last update is then not applied: ``stay_`` is the stay the last likelihood was computed under, or the
        update of the n_iter-th).  One T x K scratch table is allocated; one read-back of four numbers per iteration."""
        table, _, lens = self._utterances(corpus)
        scratch = torch.zeros((table.shape[0], self.gmm.n_components), dtype=torch.float32, device=table.device)
        w32 = self.gmm.weights_.astype(np.float32)
        self.log_likelihoods = []
        rho = self.stay_
        for it in range(int(n_iter)):
            _, ll, st, ng = self._run(table, lens, 'smooth', stay=rho, out=scratch)
            good = ng.clamp(min=0).to(torch.float64)
            ll_sum, n, ntr, stays = torch.stack([ll.sum(), good.sum(), (good - 1.0).clamp(min=0.0).sum(), st.sum()]).cpu().tolist()
            if ntr < 1:
                raise ValueError('StickyHmmPosteriorgram.fit_stay: no utterance has two good frames')
            self.log_likelihoods.append(ll_sum / n)
            self.n_bad_ = int(lens.sum() - n)
            if it > 0 and self.log_likelihoods[-1] - self.log_likelihoods[-2] < tol:
                break
            rho = check_stay('StickyHmmPosteriorgram.fit_stay', min(max(stays / ntr, 0.0), STAY_MAX), w32)
        self.stay_ = rho
        return self

    def fit(self, corpus, n_iter=10, tol=1e-4, params=PARAMS, n_ranges=0):
        """Baum-Welch from the current mixture and ``stay_``: any subset of the `m`eans, `v`ariances, `w`eights and the
        `s`tay (params) by the M-step of the module docstring.  The mixture is COPIED first: the GmmPosteriorgram this
        object was made from is untouched, ``self.gmm`` is the trained copy.  Iteration i runs forward-backward with the
        per-component stays and the statistics GEMM under the current parameters -- ``log_likelihoods[i]`` is their mean
        log-likelihood per good frame --, reads the sums, the summed stays, the likelihood and the counts back once, and
        applies the update; the stopping rule is ``fit_stay``'s (the parameters are those of the last likelihood, or the
        update of the n_iter-th).  One T x K scratch table is allocated."""
        p = check_params('StickyHmmPosteriorgram.fit', params)                    # (host checks first)
        table, _, lens = self._utterances(corpus)
        g, shift64, dev, shift = self._training_copy(table.device)
        K, D = g.means_.shape
        scratch = torch.zeros((table.shape[0], K), dtype=torch.float32, device=table.device)
        off = _utt.starts(lens)
        w, m, v, rho = g.weights_, g.means_ - shift64, g.variances_, self.stay_
        need_sums = bool(p & set('mvw'))
        self.log_likelihoods = []
        for it in range(int(n_iter)):
            A, B, _ = _gmm.score_tables(w, m, v)
            _, ll, st, ng, sk = forward_backward(table, off, lens, shift, dev(A), dev(B), dev(emission_offsets(m, v)), dev(w), rho,
                                                 'smooth', out=scratch, want_stay_k=True)
            good = ng.clamp(min=0).to(torch.float64)
            head = torch.stack([ll.sum(), good.sum(), (good - 1.0).clamp(min=0.0).sum(), st.sum()])
            sums = accumulate(table, scratch, shift, n_ranges) if need_sums else torch.zeros((K, 2 * D + 1), dtype=torch.float64,
                                                                                            device=table.device)
            back = torch.cat([head, sk.sum(dim=0), sums.flatten()]).cpu().numpy()      # the iteration's one read-back
            ll_sum, n, ntr, stays = back[:4].tolist()
            if ntr < 1:
                raise ValueError('StickyHmmPosteriorgram.fit: no utterance has two good frames')
            self.log_likelihoods.append(ll_sum / n)
            self.n_bad_ = int(lens.sum() - n)
            if it > 0 and self.log_likelihoods[-1] - self.log_likelihoods[-2] < tol:
                break
            sums_h = back[4 + K:].reshape(K, 2 * D + 1)
            if need_sums:
                self.n_starved_ = int((sums_h[:, 2 * D] < g.min_count).sum())
            w, m, v, rho, self.n_retired_ = baum_welch_update(sums_h, back[4:4 + K], ntr, m, v, g.gv_, g.var_floor, g.min_count,
                                                              params, weights=w, stay=rho, stays_total=stays)
        self._adopt(g, p, shift64, m, v, w)
        self.stay_ = rho
        return self

    # -- files ----------------------------------------------------------------------------------------------------
    def save(self, path):
        with open(path, 'wb') as f:
            np.savez(f, **self._mixture_fields(), stay=np.float64(self.stay_),
                     stay_log_likelihoods=np.asarray(self.log_likelihoods, dtype=np.float64))

    @classmethod
    def load(cls, path):
        g = _gmm.GmmPosteriorgram.load(path)
        with np.load(path) as z:
            if 'stay' not in z.files:
                raise ValueError('%s: not a StickyHmmPosteriorgram file (no stay)' % path)
            self = cls(g, float(z['stay']))
            self.log_likelihoods = [float(v) for v in z['stay_log_likelihoods']]
        return self


class TransitionHmmPosteriorgram(_MixtureHmm):
    """transform / decode / quantize / score / fit of the full-transition HMM the module docstring defines, over a fitted GmmPosteriorgram
    (its means, variances and shift; its weights only seed the default start).

    trans, init: the start; by default the sticky matrix of the mixture's weights and `stay` (``sticky_transitions``).
    alpha: the pseudo-count of the transition M-step (untuned).  corpus arguments: as StickyHmmPosteriorgram's."""

    def __init__(self, gmm, trans=None, init=None, stay=0.9, alpha=1e-3):
        super().__init__(gmm)
        if not (isinstance(alpha, (int, float, np.floating, np.integer)) and np.isfinite(alpha) and alpha >= 0):
            raise ValueError('TransitionHmmPosteriorgram: alpha = %r, a number >= 0 is needed' % (alpha,))
        K = gmm.means_.shape[0]
        if trans is None or init is None:
            i0, t0 = sticky_transitions(gmm.weights_, stay)
            init = i0 if init is None else init
            trans = t0 if trans is None else trans
        i32, t32 = check_transitions('TransitionHmmPosteriorgram', init, trans)
        if len(i32) != K:
            raise ValueError('TransitionHmmPosteriorgram: init [%d] and trans for a mixture of K = %d components' % (len(i32), K))
        self.trans_, self.init_ = t32.astype(np.float64), i32.astype(np.float64)
        self.alpha = float(alpha)
        self.viterbi_log_probs = []
        self.last_n_changed_ = None
        self.dur_ = self.dur_tail_ = None                     # q [K, L] and r [K] of the explicit durations; None: the model has none

    def set_durations(self, q=None, r=None, max_duration=None):
        """Gives the model explicit unit durations (the module docstring's semi-Markov decoder): ``dur_`` = q [K, L] and
        ``dur_tail_`` = r [K], float64, checked as ``duration_tables`` checks them; or max_duration = L alone for the
        geometric start ``geometric_durations(trans_, L)``, under which ``decode(durations=True)`` scores what ``decode()``
        scores (up to the last segment's end).  ``transform``, ``score`` and ``fit`` ignore the durations."""
        who = 'TransitionHmmPosteriorgram.set_durations'
        if (q is None) != (r is None) or (q is None) == (max_duration is None):
            raise ValueError('%s: either q [K, L] and r [K], or max_duration = L, is needed' % who)
        if q is None:
            q, r = geometric_durations(self.trans_, check_max_duration(who, max_duration))
        q64, r64 = check_durations(who, q, r)
        if q64.shape[0] != self.trans_.shape[0]:
            raise ValueError('%s: q [%d, L] for a model of K = %d units' % (who, q64.shape[0], self.trans_.shape[0]))
        self.dur_, self.dur_tail_ = q64.copy(), r64.copy()
        return self

    @classmethod
    def from_sticky(cls, h, alpha=1e-3):
        """The full-transition model that equals a fitted StickyHmmPosteriorgram; ValueError naming the components if a
        weight is 0."""
        if not isinstance(h, StickyHmmPosteriorgram):
            raise ValueError('TransitionHmmPosteriorgram.from_sticky: a StickyHmmPosteriorgram is needed')
        w = np.asarray(h.gmm.weights_)
        if (w.astype(np.float32) <= 0).any():
            raise ValueError('TransitionHmmPosteriorgram.from_sticky: the components %s have weight 0'
                             % np.flatnonzero(w.astype(np.float32) <= 0).tolist())
        return cls(h.gmm, stay=h.stay_, alpha=alpha)

    def whoami(self):
        return {'params': {'alpha': self.alpha, 'gmm': self.gmm.whoami()}, 'class_name': self.__class__.__name__}

    def device_tables(self, device):
        """(shift, A, B, c0, init32, trans32) on the device, rounded once from the float64 parameters."""
        if self._tables is None or self._tables[0].device != device:
            init = torch.from_numpy(self.init_.astype(np.float32)).to(device)
            trans = torch.from_numpy(np.ascontiguousarray(self.trans_.astype(np.float32))).to(device)
            self._tables = self._emission_tables(device) + (init, trans)
        return self._tables

    def _forward_backward(self, table, lens, mode):
        return dense_forward_backward(table, _utt.starts(lens), lens, *self.device_tables(table.device), mode=mode)

    def _with_durations(self, min_duration, durations):
        """`durations` as a bool, or ValueError: the model has none, or a min_duration > 1 came with them (host checks)."""
        who = type(self).__name__
        if durations and self.dur_ is None:
            raise ValueError('%s: durations=True, but the model has no durations (set_durations, or fit_viterbi with the '
                             'letter d)' % who)
        if durations and _utt.check_min_duration(who, min_duration) != 1:
            raise ValueError('%s: durations=True takes no min_duration (%d): the duration law is the model\'s own'
                             % (who, min_duration))
        return bool(durations)

    def _max_product(self, table, lens, min_duration, durations=False):
        shift, A, B, c0, _, _ = self.device_tables(table.device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(table.device)
        if self._with_durations(min_duration, durations):
            li, lx = switch_log_transitions(self.init_, self.trans_)
            ld, ls = duration_tables(self.dur_, self.dur_tail_)
            return hsmm_viterbi(table, _utt.starts(lens), lens, shift, A, B, c0, up(li), up(lx), up(ld), up(ls))
        li, lt = (up(a) for a in log_transitions(self.init_, self.trans_))
        return dense_viterbi(table, _utt.starts(lens), lens, shift, A, B, c0, li, lt, min_duration=min_duration)

    def decode(self, corpus, min_duration=1, durations=False):
        """The unit ids of the best path (the module docstring's full-transition max-product recurrence), int32, -1 for a
        BAD frame: {name: host array [length]} in corpus order for a DeviceCorpus, a dict or a file -- what
        KMeansQuantizer.segment and StickyHmmPosteriorgram.decode return, so kmeans.unit_sequences / bitrate / segments,
        eskmeans.landmarks_from_units, tde.unit_boundaries and hmm.bigram_counts take it as it is --; for a [T, D] table,
        which is ONE utterance, the device tensor [T].  ``last_log_prob_`` (float64), ``last_n_switch_`` and
        ``last_n_good_`` (int32) hold the utterances' log joint probabilities, switch counts and good-frame counts;
        ``n_bad_`` the BAD frames.  min_duration = S (an integer 1 .. 8): every unit but an utterance's last lasts at least
        S good frames (the module docstring's minimum duration of this model; with S > 1 ``last_log_prob_`` is that
        definition's score); 1 is the recurrence without it.  durations=True: the semi-Markov path under the model's own
        duration law ``dur_`` / ``dur_tail_`` (``last_log_prob_`` is that definition's score); ValueError if the model has
        none, or together with min_duration > 1."""
        return super().decode(corpus, min_duration, durations=self._with_durations(min_duration, durations))

    def quantize(self, corpus, min_duration=1, durations=False):
        """``_MixtureHmm.quantize`` of the path ``decode`` with the same arguments gives."""
        return super().quantize(corpus, min_duration, durations=self._with_durations(min_duration, durations))

    def _adopt_transitions(self, trans, init):
        self.trans_, self.init_ = np.array(trans, dtype=np.float64), np.array(init, dtype=np.float64)

    def fit(self, corpus, n_iter=10, tol=1e-4, params=DENSE_PARAMS, n_ranges=0):
        """Baum-Welch from the current parameters: any subset of the `m`eans, `v`ariances, `t`ransitions and the `i`nit
        (params).  The mixture is COPIED first: the GmmPosteriorgram this object was made from is untouched, ``self.gmm``
        is the trained copy.  Iteration i runs forward-backward with the statistics and the statistics GEMM under the
        current parameters -- ``log_likelihoods[i]`` is their mean log-likelihood per good frame --, reads everything back
        once, and applies the update; the stopping rule is StickyHmmPosteriorgram.fit's.  Fills ``log_likelihoods``,
        ``n_bad_``, ``n_starved_``, ``trans_`` and ``init_``.  One T x K scratch table is allocated."""
        who = 'TransitionHmmPosteriorgram.fit'
        p = check_dense_params(who, params)                                        # (host checks first)
        table, _, lens = self._utterances(corpus)
        g, shift64, dev, shift = self._training_copy(table.device)
        K, D = g.means_.shape
        scratch = torch.zeros((table.shape[0], K), dtype=torch.float32, device=table.device)
        off = _utt.starts(lens)
        m, v, trans, init = g.means_ - shift64, g.variances_, self.trans_, self.init_
        mv = ''.join(c for c in 'mv' if c in p)
        self.log_likelihoods = []
        for it in range(int(n_iter)):
            A, B, _ = _gmm.score_tables(np.full(K, 1.0 / K), m, v)
            _, ll, ng, stats = dense_forward_backward(table, off, lens, shift, dev(A), dev(B), dev(emission_offsets(m, v)), dev(init),
                                                      dev(trans), 'smooth', out=scratch, want_stats=True)
            good = ng.clamp(min=0).to(torch.float64)
            head = torch.stack([ll.sum(), good.sum(), (good - 1.0).clamp(min=0.0).sum()])
            sums = accumulate(table, scratch, shift, n_ranges) if mv else torch.zeros((K, 2 * D + 1), dtype=torch.float64,
                                                                                      device=table.device)
            back = torch.cat([head, stats.flatten(), sums.flatten()]).cpu().numpy()      # the iteration's one read-back
            ll_sum, n, ntr = back[:3].tolist()
            if n < 1:
                raise ValueError('%s: the corpus has no good frame' % who)
            if 't' in p and ntr < 1:
                raise ValueError('%s: no utterance has two good frames: the transitions cannot be estimated' % who)
            self.log_likelihoods.append(ll_sum / n)
            self.n_bad_ = int(lens.sum() - n)
            if it > 0 and self.log_likelihoods[-1] - self.log_likelihoods[-2] < tol:
                break
            stats_h = back[3:3 + (K + 1) * K].reshape(K + 1, K)
            sums_h = back[3 + (K + 1) * K:].reshape(K, 2 * D + 1)
            if mv:
                self.n_starved_ = int((sums_h[:, 2 * D] < g.min_count).sum())
                _, m, v, _, _ = baum_welch_update(sums_h, np.zeros(K), ntr, m, v, g.gv_, g.var_floor, g.min_count, mv,
                                                  weights=np.full(K, 1.0 / K), stay=0.0)
            trans, init = transition_update(stats_h, trans, init, self.alpha, ''.join(c for c in 'ti' if c in p))
        self._adopt(g, p, shift64, m, v)
        self._adopt_transitions(trans, init)
        return self

    def fit_viterbi(self, corpus, n_iter=10, tol=1e-4, params=DENSE_PARAMS, min_duration=1, n_ranges=0, max_duration=None):
        """Viterbi training (hard EM, segmental k-means) from the current parameters: any subset of the `m`eans,
        `v`ariances, `t`ransitions and the `i`nit (params), on a COPY of the mixture exactly as ``fit``.  Iteration i decodes
        the corpus under the current parameters (``dense_viterbi`` with min_duration) -- ``viterbi_log_probs[i]`` is the mean
        best-path log probability per good frame --, takes the hard statistics of the decoded ids (``hard_stats``, the same
        min_duration), reads everything back ONCE, and applies ``baum_welch_update`` to the sums and ``transition_update``
        to the counts.  It stops after n_iter iterations, as soon as viterbi_log_probs[i] - viterbi_log_probs[i - 1] < tol,
        or when no id changed since the previous iteration (counted on the device; the parameters are then those of the
        last decoding).  Fills ``viterbi_log_probs``, ``n_bad_``, ``n_starved_``, ``last_n_changed_`` (the ids that
        differed from the previous iteration's; all rows in the first), ``trans_`` and ``init_``.  No T x K table is
        allocated: two [T] id buffers and the two workspaces.

        Explicit durations (the module docstring's semi-Markov decoder): with the letter `d` in params (this method only;
        ``fit`` refuses it) or with max_duration = L, iteration i decodes with ``hsmm_viterbi``, takes ``hard_stats`` at
        min_duration = 1 and ``run_stats`` on the same ids, still reads back once, and applies ``duration_update`` beside the
        two updates above when `d` is named.  The start is the model's own law (``set_durations``) if its width is L or no
        max_duration is given, otherwise ``geometric_durations(trans_, L)``; ``dur_`` and ``dur_tail_`` are filled.
        min_duration must then be 1."""
        who = 'TransitionHmmPosteriorgram.fit_viterbi'
        p = check_hsmm_params(who, params)                                         # (host checks first)
        S = _utt.check_min_duration(who, min_duration)
        hsmm = 'd' in p or max_duration is not None
        q = r = None
        if hsmm:
            if S != 1:
                raise ValueError('%s: explicit durations take no min_duration (%d)' % (who, S))
            if max_duration is None and self.dur_ is None:
                raise ValueError('%s: the letter d needs max_duration = L, or a model that has durations' % who)
            if max_duration is not None and (self.dur_ is None or self.dur_.shape[1] != check_max_duration(who, max_duration)):
                q, r = geometric_durations(self.trans_, max_duration)
            else:
                q, r = self.dur_, self.dur_tail_
            q, r = check_durations(who, q, r)
            L = q.shape[1]
        n_ranges = _check_n_ranges(who, n_ranges)
        table, _, lens = self._utterances(corpus)
        lib = _lib.load()
        K, D = self.gmm.means_.shape
        if K > dense_max_k():
            raise ValueError('%s: K = %d, the kernel takes 1 .. %d (abny_hmm_dense_max_k)' % (who, K, dense_max_k()))
        T = table.shape[0]
        off_h, len_h, n_utt, longest = _utt.utterance_spans(who, _utt.starts(lens), lens, T, max_len(), 'abn_hmm_max_len')
        if not (T and n_utt and longest):
            raise ValueError('%s: the corpus has no frame' % who)
        g, shift64, dev, shift = self._training_copy(table.device)
        sizing = (lambda n, m, k, d: lib.abnu_hmm_hsmm_viterbi_ws_bytes(n, m, k, d, L)) if hsmm else _dense_viterbi_sizing(lib, S)
        vws, off_d, len_d = _utt.workspace(who, sizing, off_h, len_h, longest, K, D, table.device)
        hws = _hard_stats_workspace(who, lib, T, n_utt, K, D, n_ranges, table.device)
        ids, lp, nsw, ng = _utt.path_results(None, T, n_utt, True, table.device)
        ids = [ids, torch.full_like(ids, -1)]                 # (two buffers: an iteration's ids are compared with the last's)
        m, v, trans, init = g.means_ - shift64, g.variances_, self.trans_, self.init_
        mv, ti = ''.join(c for c in 'mv' if c in p), ''.join(c for c in 'ti' if c in p)
        self.viterbi_log_probs = []
        for it in range(int(n_iter)):
            A, B, _ = _gmm.score_tables(np.full(K, 1.0 / K), m, v)
            A, B, c0 = dev(A), dev(B), dev(emission_offsets(m, v))
            cur = ids[it & 1]
            if hsmm:
                li, lx = (dev(a) for a in switch_log_transitions(init, trans))
                ld, ls = (dev(a) for a in duration_tables(q, r))
                _hsmm_viterbi_launch(lib, table, off_d, len_d, n_utt, shift, A, B, c0, li, lx, ld, ls, K, L, cur, lp, nsw, ng, vws)
            else:
                li, lt = (dev(a) for a in log_transitions(init, trans))
                _dense_viterbi_launch(lib, table, off_d, len_d, n_utt, shift, A, B, c0, li, lt, K, cur, lp, nsw, ng, S, vws)
            counts, sums, _ = _hard_stats_launch(lib, table, off_d, len_d, n_utt, shift, cur, K, S, n_ranges, hws)
            runs = torch.zeros(0, dtype=torch.float64, device=table.device)
            if hsmm:                                          # [dur | tail] behind the sums, in the same read-back
                runs = torch.cat([t.flatten() for t in _run_stats_launch(lib, cur, off_d, len_d, n_utt, K, L)]).to(torch.float64)
            changed = (cur != ids[(it + 1) & 1]).sum().to(torch.float64) if it else torch.tensor(float(T), dtype=torch.float64,
                                                                                                 device=table.device)
            head = torch.stack([lp.sum(), ng.clamp(min=0).to(torch.float64).sum(), changed])
            back = torch.cat([head, counts.flatten().to(torch.float64), sums.flatten(), runs]).cpu().numpy()      # the one read-back
            lp_sum, n, n_changed = back[:3].tolist()
            if n < 1:
                raise ValueError('%s: the corpus has no good frame' % who)
            self.viterbi_log_probs.append(lp_sum / n)
            self.n_bad_, self.last_n_changed_ = int(lens.sum() - n), int(n_changed)
            if it > 0 and (self.viterbi_log_probs[-1] - self.viterbi_log_probs[-2] < tol or n_changed == 0):
                break
            counts_h = back[3:3 + (K + 1) * K].reshape(K + 1, K)
            n_sums = K * (2 * D + 1)
            sums_h = back[3 + (K + 1) * K:3 + (K + 1) * K + n_sums].reshape(K, 2 * D + 1)
            if mv:
                self.n_starved_ = int((sums_h[:, 2 * D] < g.min_count).sum())
                _, m, v, _, _ = baum_welch_update(sums_h, np.zeros(K), 0, m, v, g.gv_, g.var_floor, g.min_count, mv,
                                                  weights=np.full(K, 1.0 / K), stay=0.0)
            trans, init = transition_update(counts_h, trans, init, self.alpha, ti)
            if 'd' in p:
                runs_h = back[3 + (K + 1) * K + n_sums:]
                q, r = duration_update(runs_h[:K * L].reshape(K, L), runs_h[K * L:], q, r, self.alpha)
        self._adopt(g, p, shift64, m, v)
        self._adopt_transitions(trans, init)
        if hsmm:
            self.dur_, self.dur_tail_ = np.array(q, dtype=np.float64), np.array(r, dtype=np.float64)
        return self

    # -- files ----------------------------------------------------------------------------------------------------
    def save(self, path):
        """The mixture's file (GmmPosteriorgram.load reads it) plus trans, init and alpha, and dur, dur_tail if the model has
        durations."""
        durations = {} if self.dur_ is None else dict(dur=self.dur_, dur_tail=self.dur_tail_)
        with open(path, 'wb') as f:
            np.savez(f, **self._mixture_fields(), **durations, trans=self.trans_, init=self.init_, alpha=np.float64(self.alpha),
                     trans_log_likelihoods=np.asarray(self.log_likelihoods, dtype=np.float64),
                     viterbi_log_probs=np.asarray(self.viterbi_log_probs, dtype=np.float64))

    @classmethod
    def load(cls, path):
        g = _gmm.GmmPosteriorgram.load(path)
        with np.load(path) as z:
            if 'trans' not in z.files or 'init' not in z.files:
                raise ValueError('%s: not a TransitionHmmPosteriorgram file (no trans)' % path)
            self = cls(g, z['trans'].astype(np.float64), z['init'].astype(np.float64), alpha=float(z['alpha']))
            self.trans_, self.init_ = z['trans'].astype(np.float64), z['init'].astype(np.float64)
            self.log_likelihoods = [float(v) for v in z['trans_log_likelihoods']]
            if 'viterbi_log_probs' in z.files:                                 # (files written before fit_viterbi have none)
                self.viterbi_log_probs = [float(v) for v in z['viterbi_log_probs']]
            if 'dur' in z.files and 'dur_tail' in z.files:                     # (files without durations load as before)
                self.dur_, self.dur_tail_ = check_durations('%s: dur' % path, z['dur'], z['dur_tail'])
        return self


def _holds(path, key):
    with np.load(path) as z:
        return key in z.files


def _report_decode(h, out, times, model, path):
    """Writes the decoded ids and prints the report; `model` is the fragment that names the chain."""
    from . import kmeans as _kmeans
    _gmm._write_named(path, out, times, as_column=True)
    n_good = int(h.last_n_good_.sum())
    if times is not None:
        seconds = sum(float(np.asarray(times[k])[-1] - np.asarray(times[k])[0]) for k in out if len(times[k]) > 1)
        rate = '%.2f bits/s' % _kmeans.bitrate(_kmeans.unit_sequences(out), seconds) if seconds > 0 else 'n/a (no duration)'
    else:
        rate = '%.2f bits/s at 100 frames/s' % _kmeans.bitrate(_kmeans.unit_sequences(out), max(n_good, 1) / 100.0)
    print('%d files, %d frames (%d BAD), K = %d, %s, %d switches, bitrate %s, mean log-probability %.6f per good frame -> %s'
          % (len(out), sum(v.shape[0] for v in out.values()), h.n_bad_, h.gmm.n_components, model,
             int(h.last_n_switch_.sum()), rate, float(h.last_log_prob_.sum()) / max(n_good, 1), path))
    return 0


def _report_transform(h, feats, times, mode, model, path):
    """Writes the posteriorgrams and prints the report; `model` as in ``_report_decode``."""
    post = h.transform(feats, mode).cpu().numpy()
    out = _gmm._split_rows(post, ((k, v.shape[0]) for k, v in feats.items()))
    _gmm._write_named(path, out, times)
    print('%d files, %d frames, K = %d, %s -> %s' % (len(out), post.shape[0], post.shape[1], model, path))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m abnet3_amd.hmm', description='Sticky-HMM smoothing of Gaussian posteriorgrams')
    sub = ap.add_subparsers(dest='cmd', required=True)
    f = sub.add_parser('fit-stay', help='fit the stay probability of a saved mixture on FEATURES and save the model')
    f.add_argument('gmm', help='a GmmPosteriorgram .npz (python -m abnet3_amd.gmm fit)')
    f.add_argument('features', help='h5features file, or an .npz of name -> [T, D]')
    f.add_argument('model', help='the .npz to write')
    f.add_argument('--stay', type=float, default=0.9, help='where EM starts')
    f.add_argument('--n-iter', type=int, default=10)
    f.add_argument('--tol', type=float, default=1e-4)
    b = sub.add_parser('fit', help='Baum-Welch from a saved mixture on FEATURES: means, variances, weights and the stay')
    b.add_argument('gmm', help='a GmmPosteriorgram .npz (python -m abnet3_amd.gmm fit)')
    b.add_argument('features', help='h5features file, or an .npz of name -> [T, D]')
    b.add_argument('model', help='the .npz to write')
    b.add_argument('--stay', type=float, default=0.9, help='where EM starts')
    b.add_argument('--n-iter', type=int, default=10)
    b.add_argument('--tol', type=float, default=1e-4)
    b.add_argument('--params', default=PARAMS, help='the letters of what is re-estimated: m means, v variances, w weights, s stay')
    t = sub.add_parser('transform', help='smoothed posteriorgrams of FEATURES under a saved model')
    t.add_argument('model')
    t.add_argument('features', help='h5features file, or an .npz of name -> [T, D]')
    t.add_argument('out', help='.npz of name -> [T, K], or an h5features file (when the input has times)')
    t.add_argument('--mode', choices=sorted(MODES), default='smooth')
    d = sub.add_parser('decode', help='unit ids of the best path of FEATURES under a saved model')
    d.add_argument('model')
    d.add_argument('features', help='h5features file, or an .npz of name -> [T, D]')
    d.add_argument('out', help='.npz of name -> [T] ids, or an h5features file (when the input has times)')
    d.add_argument('--min-duration', type=int, default=1, metavar='S',
                   help='every unit lasts at least S frames (1 .. 8; default 1, no minimum)')
    d.add_argument('--durations', action='store_true', help='decode under the explicit unit durations a full-transition model holds')
    ft = sub.add_parser('fit-trans', help='Baum-Welch of the full-transition model on FEATURES, from a saved model or mixture')
    ft.add_argument('model', help='a TransitionHmmPosteriorgram, StickyHmmPosteriorgram or GmmPosteriorgram .npz: where EM starts')
    ft.add_argument('features', help='h5features file, or an .npz of name -> [T, D]')
    ft.add_argument('out', help='the .npz to write')
    ft.add_argument('--stay', type=float, default=0.9, help='the sticky start over a plain mixture')
    ft.add_argument('--n-iter', type=int, default=10)
    ft.add_argument('--tol', type=float, default=1e-4)
    ft.add_argument('--params', default=DENSE_PARAMS, help='the letters of what is re-estimated: m means, v variances, t transitions, i init')
    ft.add_argument('--alpha', type=float, default=1e-3, help='pseudo-count of the transition update (untuned)')
    ft.add_argument('--viterbi', action='store_true', help='Viterbi training (hard EM on the decoded path) instead of Baum-Welch')
    ft.add_argument('--min-duration', type=int, default=1, metavar='S',
                    help='with --viterbi: train the model whose every unit lasts at least S frames (1 .. 8; default 1)')
    ft.add_argument('--max-duration', type=int, default=None, metavar='L',
                    help='with --viterbi: train explicit unit durations, a free law up to L frames and a geometric tail '
                         '(2 .. 32; add the letter d to --params to learn it; untuned)')
    args = ap.parse_args(argv)
    if args.cmd == 'fit':
        check_params('python -m abnet3_amd.hmm fit', args.params)
    feats, times = _gmm._read_features(args.features)
    if args.cmd == 'fit-trans':
        if _holds(args.model, 'trans'):
            h = TransitionHmmPosteriorgram.load(args.model)
            h.alpha = float(args.alpha)
        elif _holds(args.model, 'stay'):
            h = TransitionHmmPosteriorgram.from_sticky(StickyHmmPosteriorgram.load(args.model), alpha=args.alpha)
        else:
            h = TransitionHmmPosteriorgram(_gmm.GmmPosteriorgram.load(args.model), stay=args.stay, alpha=args.alpha)
        if args.max_duration is not None and not args.viterbi:
            raise ValueError('python -m abnet3_amd.hmm fit-trans: --max-duration %d needs --viterbi (Baum-Welch ignores the '
                             'durations)' % args.max_duration)
        if args.viterbi:
            h.fit_viterbi(feats, args.n_iter, args.tol, args.params, min_duration=args.min_duration, max_duration=args.max_duration)
            h.save(args.out)
            if h.dur_ is not None:
                print('explicit durations up to L = %d frames: the modes of the units\' laws %s, mean tail stay %.4f'
                      % (h.dur_.shape[1], (np.argmax(h.dur_, axis=1) + 1).tolist(), float(h.dur_tail_.mean())))
            print('K = %d transitions after %d iterations of Viterbi training (params %s, alpha %g, min duration %d), mean best-path '
                  'log-probability %.6f, %d ids changed in the last, %d BAD frames, %d starved, mean self-transition %.4f'
                  % (h.trans_.shape[0], len(h.viterbi_log_probs), args.params, h.alpha, args.min_duration, h.viterbi_log_probs[-1],
                     h.last_n_changed_, h.n_bad_, h.n_starved_, float(np.diag(h.trans_).mean())))
            return 0
        if args.min_duration != 1:
            raise ValueError('python -m abnet3_amd.hmm fit-trans: --min-duration %d needs --viterbi (Baum-Welch has no minimum '
                             'duration)' % args.min_duration)
        h.fit(feats, args.n_iter, args.tol, args.params)
        h.save(args.out)
        print('K = %d transitions after %d iterations (params %s, alpha %g), mean log-likelihood %.6f, %d BAD frames, %d starved, '
              'mean self-transition %.4f' % (h.trans_.shape[0], len(h.log_likelihoods), args.params, h.alpha, h.log_likelihoods[-1],
                                             h.n_bad_, h.n_starved_, float(np.diag(h.trans_).mean())))
        return 0
    if args.cmd == 'fit':
        h = StickyHmmPosteriorgram(_gmm.GmmPosteriorgram.load(args.gmm), args.stay).fit(feats, args.n_iter, args.tol, args.params)
        h.save(args.model)
        print('stay %.6f after %d iterations (params %s), mean log-likelihood %.6f, %d BAD frames, %d starved, %d retired'
              % (h.stay_, len(h.log_likelihoods), args.params, h.log_likelihoods[-1], h.n_bad_, h.n_starved_, h.n_retired_))
        return 0
    if args.cmd == 'fit-stay':
        h = StickyHmmPosteriorgram(_gmm.GmmPosteriorgram.load(args.gmm), args.stay).fit_stay(feats, args.n_iter, args.tol)
        h.save(args.model)
        print('stay %.6f after %d iterations, mean log-likelihood %.6f, %d BAD frames'
              % (h.stay_, len(h.log_likelihoods), h.log_likelihoods[-1], h.n_bad_))
        return 0
    dense = _holds(args.model, 'trans')
    h = (TransitionHmmPosteriorgram if dense else StickyHmmPosteriorgram).load(args.model)
    model = 'full transitions' if dense else 'stay %.4f' % h.stay_
    if args.cmd == 'decode':
        if dense and args.min_duration != 1:
            raise ValueError('python -m abnet3_amd.hmm decode: %s holds a full transition matrix, whose max-product path '
                             'has no minimum duration; --min-duration %d needs a sticky model' % (args.model, args.min_duration))
        if args.durations and not (dense and h.dur_ is not None):
            raise ValueError('python -m abnet3_amd.hmm decode: --durations needs a full-transition model that holds dur; %s has none'
                             % args.model)
        if args.durations:
            model += ', explicit durations up to %d' % h.dur_.shape[1]
            return _report_decode(h, h.decode(feats, durations=True), times, model, args.out)
        out = h.decode(feats) if dense else h.decode(feats, min_duration=args.min_duration)
        return _report_decode(h, out, times, model, args.out)
    return _report_transform(h, feats, times, args.mode, model, args.out)


if __name__ == '__main__':
    sys.exit(main())
