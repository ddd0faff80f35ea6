"""The hard statistics of the full-transition HMM's Viterbi training (abnv_hmm_hard_stats, hmm.hard_stats) and the training
loop around them (TransitionHmmPosteriorgram.fit_viterbi) restated in numpy with explicit loops, in float64 (test
infrastructure only): the reference their tests compare the kernel with.

The definition.  A frame is good if 0 <= ids[t] < K; every other id is BAD and is passed over.  Per utterance u let
a_0 .. a_{n-1} be the ids of its good frames in frame order and S = min_duration:
    n_good[u] = n;   counts[K][a_0] += 1 when n >= 1                          (row K: the utterances' first units)
    i >= 1, a_i != a_{i-1}:  counts[a_{i-1}][a_i] += 1                        (a switch)
    i >= 1, a_i == a_{i-1}:  counts[a_i][a_i] += 1 only if i >= S and a_{i-1} = ... = a_{i-S} = a_i
                                                                              (a stay in the chain's last state)
Nothing connects two utterances, rows outside every utterance contribute nothing, an utterance outside 0 .. T gets n_good -1.
sums [K][2D + 1] = [S1 | S2 | N] over the good frames of the utterances: xc = fl32(x - shift), sq = fl32(xc xc) (one
rounding each, taken in float32 as the kernel takes them), an entry whose sq is not finite contributes 0 to both; the sums
themselves are float64 here.

The bar of a float comparison (`sums_bar`).  The kernel adds the terms of a (range, unit) partial one after the other in fp32
and the partials in float64.  A sequential fp32 sum of n terms differs from the exact sum by at most (n - 1) 2^-24 sum|terms|
to first order -- n 2^-24 sum|terms| covers the higher orders for n < 2^20 --, a partial is at most N[k] frames long, and the
float64 steps are 2^-29 times smaller than that: per unit k and column c the bar is 2^-24 N[k] sum over k's frames of
|term|.  It holds for every n_ranges, so two n_ranges differ by at most twice the bar.  Derived, not measured.
"""
import numpy as np

import hmm_dense_dur_np as dd
import hmm_dense_vit_np as dv

U24 = 2.0 ** -24


def counts_one(ids, K, S):
    """(counts int64 [K + 1, K], n_good) of one utterance's ids: a loop over the frames, a loop over the S previous good ids."""
    counts = np.zeros((K + 1, K), dtype=np.int64)
    a = [int(v) for v in np.asarray(ids).ravel() if 0 <= int(v) < K]
    for i, k in enumerate(a):
        if i == 0:
            counts[K, k] += 1
        elif a[i - 1] != k:
            counts[a[i - 1], k] += 1
        else:
            stay = i >= S
            for s in range(1, S + 1):
                stay = stay and a[i - s] == k
            if stay:
                counts[k, k] += 1
    return counts, len(a)


def terms(x, shift):
    """(xc, sq) float32 [T, D]: the kernel's two roundings and its rule for a non-finite entry."""
    with np.errstate(all='ignore'):
        xc = (np.asarray(x, dtype=np.float32) - np.asarray(shift, dtype=np.float32)[None, :]).astype(np.float32)
        sq = (xc * xc).astype(np.float32)
    bad = ~np.isfinite(sq)
    xc, sq = xc.copy(), sq.copy()
    xc[bad], sq[bad] = 0.0, 0.0
    return xc, sq


def hard_stats(x, off, lens, shift, ids, K, S=1, with_abs=False):
    """(counts int64 [K + 1, K], sums float64 [K, 2D + 1], n_good int32 [n_utt]); with_abs: a fourth element, the sums of
    the |terms| in sums' layout (for `sums_bar`)."""
    x = np.asarray(x, dtype=np.float32)
    T, D = x.shape
    ids = np.asarray(ids)
    counts = np.zeros((K + 1, K), dtype=np.int64)
    sums = np.zeros((K, 2 * D + 1), dtype=np.float64)
    mags = np.zeros((K, 2 * D + 1), dtype=np.float64)
    ng = np.zeros(len(off), dtype=np.int32)
    xc, sq = terms(x, shift)
    xc, sq = xc.astype(np.float64), sq.astype(np.float64)
    for u, (o, n) in enumerate(zip(off, lens)):
        o, n = int(o), int(n)
        if o < 0 or n < 0 or o + n > T:
            ng[u] = -1
            continue
        c, ng[u] = counts_one(ids[o:o + n], K, S)
        counts += c
        for t in range(o, o + n):
            k = int(ids[t])
            if 0 <= k < K:
                sums[k, :D] += xc[t]
                sums[k, D:2 * D] += sq[t]
                sums[k, 2 * D] += 1.0
                mags[k, :D] += np.abs(xc[t])
                mags[k, D:2 * D] += sq[t]
                mags[k, 2 * D] += 1.0
    return (counts, sums, ng, mags) if with_abs else (counts, sums, ng)


def sums_bar(mags):
    """[K, 2D + 1]: the module docstring's bar from hard_stats' with_abs sums; 0 in the count column (integers)."""
    mags = np.asarray(mags, dtype=np.float64)
    bar = U24 * mags[:, -1:] * mags
    bar[:, -1] = 0.0
    return bar


def scores64(x, shift, m, v):
    """float64 [T, K]: log N(x; m + shift, v) of the centred float64 parameters m, v [K, D] from xc = fl32(x - shift); BAD
    rows (a non-finite xc^2 in float32) are flagged in the second result."""
    xc = (np.asarray(x, dtype=np.float32) - np.asarray(shift, dtype=np.float32)[None, :]).astype(np.float32)
    with np.errstate(all='ignore'):
        bad = ~np.isfinite((xc * xc).astype(np.float32)).all(axis=1)
    z = np.where(bad[:, None], 0.0, xc.astype(np.float64))
    s = -0.5 * (np.log(2.0 * np.pi * v)[None, :, :] + (z[:, None, :] - m[None, :, :]) ** 2 / v[None, :, :]).sum(axis=2)
    return s, bad


def fit_viterbi(hmm, x, lens, shift, m, v, gv, trans, init, S=1, n_iter=10, tol=1e-4, params='mvti', alpha=0.0, var_floor=0.01,
                min_count=1.0):
    """The float64 training loop: (viterbi_log_probs, m, v, trans, init, ids of the last decoding, n_changed of the last
    iteration).  hmm: the abnet3_amd.hmm module, for its two host updates; the decoder is hmm_dense_vit_np.viterbi_one in
    float64 (S = 1) or hmm_dense_dur_np.viterbi_one (S > 1), the statistics are this file's."""
    x = np.asarray(x, dtype=np.float32)
    K, D = m.shape
    off = np.cumsum(lens) - np.asarray(lens)
    m, v = np.array(m, dtype=np.float64), np.array(v, dtype=np.float64)
    trans, init = np.array(trans, dtype=np.float64), np.array(init, dtype=np.float64)
    mv, ti = ''.join(c for c in 'mv' if c in params), ''.join(c for c in 'ti' if c in params)
    lps, prev, n_changed = [], None, x.shape[0]
    ids = None
    for it in range(n_iter):
        s, bad = scores64(x, shift, m, v)
        li, lt = np.log(init), np.log(trans)
        ids = np.full(x.shape[0], -1, dtype=np.int32)
        total, n = 0.0, 0
        for o, L in zip(off, lens):
            sl = slice(int(o), int(o) + int(L))
            if S == 1:
                r = dv.viterbi_one(s[sl], ~bad[sl], li, lt, dtype=np.float64)
            else:
                r = dd.viterbi_one(s[sl], ~bad[sl], li, lt, S)
            ids[sl] = r[0]
            # the score of the decoded path in float64 (dd.viterbi_one's own sum is over float32 steps)
            total += dd.J_runs(s[sl], r[0], ~bad[sl], li, lt, S)
            n += r[3]
        lps.append(total / n)
        n_changed = x.shape[0] if prev is None else int((ids != prev).sum())
        prev = ids
        if it > 0 and (lps[-1] - lps[-2] < tol or n_changed == 0):
            break
        counts, sums, _ = hard_stats(x, off, lens, shift, ids, K, S)
        if mv:
            _, m, v, _, _ = hmm.baum_welch_update(sums, np.zeros(K), 0, m, v, gv, var_floor, min_count, mv, weights=np.full(K, 1.0 / K),
                                                  stay=0.0)
        trans, init = hmm.transition_update(counts.astype(np.float64), trans, init, alpha, ti)
    return lps, m, v, trans, init, ids, n_changed


def planted_corpus(seed=0, n_utt=12, bad_share=0.05):
    """The planted corpus of the training tests: K = 4, D = 2, means at the corners of a square of side 6, unit variances;
    trans 0.8 on the diagonal, + 0.15 to unit (k + 1) mod 4, 0.05 spread over the others; n_utt utterances of 40 .. 119
    frames, bad_share of the frames NaN.  (x float32 [T, 2], lens, means [4, 2], trans [4, 4], true states)."""
    rng = np.random.RandomState(seed)
    K = 4
    means = np.array([[0.0, 0.0], [6.0, 0.0], [6.0, 6.0], [0.0, 6.0]])
    trans = np.full((K, K), 0.05 / (K - 1))
    trans[np.arange(K), np.arange(K)] = 0.8
    for k in range(K):
        trans[k, (k + 1) % K] += 0.15
    trans = trans / trans.sum(axis=1, keepdims=True)
    lens = rng.randint(40, 120, size=n_utt)
    xs, zs = [], []
    for L in lens:
        z = np.zeros(L, dtype=np.int64)
        z[0] = rng.randint(K)
        for t in range(1, L):
            z[t] = rng.choice(K, p=trans[z[t - 1]])
        xs.append(means[z] + rng.randn(L, 2))
        zs.append(z)
    x = np.concatenate(xs).astype(np.float32)
    z = np.concatenate(zs)
    bad = rng.rand(len(x)) < bad_share
    x[bad, rng.randint(2, size=int(bad.sum()))] = np.nan
    return x, lens, means, trans, z


def planted_start(means, seed=0):
    """The start of the training tests: means + N(0, 1), variances 2, uniform trans / init."""
    rng = np.random.RandomState(1000 + seed)
    K, D = means.shape
    return means + rng.randn(K, D), np.full((K, D), 2.0), np.full((K, K), 1.0 / K), np.full(K, 1.0 / K)
