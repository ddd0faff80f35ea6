"""The semi-Markov decoder over the full-transition model's units (abnu_hmm_hsmm_viterbi), its run statistics
(abnu_hmm_run_stats) and the duration M-step restated in numpy with explicit loops over frames, duration states and runs
(test infrastructure only): the reference the tests compare the kernel and abnet3_amd.hmm with.  tests/hmm_dense_vit_np.py
is the model without durations, tests/hmm_dense_dur_np.py the one with a minimum duration.

The definition.  One utterance, good frames only (a BAD frame gets id -1 and is passed over; durations count good frames).
A path is a sequence of segments (k_i, n_i) with k_i != k_{i+1} and n_i >= 1, so the maximal runs of a path's ids ARE its
segments and n_switch = segments - 1.  Unit k lasts d frames with log probability
    logp_k(d) = ld[k][d-1] for d < L,     logp_k(d) = ld[k][L-1] + (d - L) ls[k] for d >= L
(ld, ls: hmm.duration_tables' float32 tables), and the score of a path is
    sum of the frames' scores s[t, k] + li[k_1] + lx[k_{i-1}][k_i] for each later segment + logp_{k_i}(n_i) for EVERY segment,
the utterance's last included (it is treated as complete, not censored).

Recurrence, every operation one rounded add or a compare in the order written; V[k][1 .. L] the normalised previous values
(here V[:, i - 1]), state i = "the current segment is i frames long", state L = "L or more":
    first good frame:   U[k][1] = s[k] + li[k], every other state -inf
    later good frames:  x[j] = max_i (V[j][i] + ld[j][i]),  xi[j] = the lowest i attaining it (strict compares, ascending i)
                        ent[k] = max over j != k of (x[j] + lx[j][k]),  bp[k] = the lowest such j
                        U[k][1] = s[k] + ent[k];   U[k][i] = s[k] + V[k][i-1] for 1 < i < L
                        a = V[k][L] + ls[k],  st = a > V[k][L-1]  (strict: a tie goes to the advance)
                        U[k][L] = s[k] + (st ? a : V[k][L-1])
    every good frame:   N_t = max over (k, i) of U,  V = U - N_t,  log_prob += N_t  (float64, frame order)
    after the last:     F = max over (k, i) of (V[k][i] + ld[k][i]),  final = the lowest k, then the lowest i, attaining it;
                        log_prob += F
The max over j != k is taken as the kernel takes it: over ALL j ascending with strict compares, the diagonal candidate -inf.
Traceback from (k, i) at frame t: i == L and st set -> (k, L); otherwise i > 1 -> (k, i-1); otherwise -> (bp[k], xi[bp[k]] as
recorded at frame t), one switch -- unless t is the first good frame, where the walk ends.

`viterbi_one(..., dtype=np.float32)` is the yardstick the kernel must EQUAL on exact inputs; dtype=np.float64 the reference
optimum for float data.

The allowance of the float comparison (`delta`), in the manner of tests/hmm_dense_dur_np.py: the recurrence is exact dynamic
programming over cell values each perturbed by at most delta, so for every path |J'(a) - J64(a)| <= (n_good + 1) delta (one
cell per good frame and the closing F), and J64(a64) >= J64(a*) >= J64(a64) - 2 (n_good + 1) delta.  With smax the largest
|score| and lmax the largest |table entry|:
  * a finite V[k][i] is at least -Vmax, Vmax = 2 (L + 2)(smax + 2 lmax).  A frame changes any path's score by at most
    smax + 2 lmax in magnitude (a switch adds an ld and an lx entry), so two paths drift apart by at most 2 (smax + 2 lmax) a
    frame.  Every state may close its segment (every ld entry is finite), so state (k, i) at frame t, entered i - 1 frames
    earlier, can be compared with the path that goes from the best state of frame t - i -- or, where that state is in unit k
    itself, which k cannot be entered from, of frame t - i - 1 through any other unit for one frame -- into k: at most
    L + 1 frames of drift and the entry's tables, under (L + 2) frames' worth.  The tail state is a maximum over entry times
    and so no worse than the entry L - 1 frames back.  Nearer the utterance's start the chain begun at the first good frame
    takes the comparison's place.  (K = 1: the one chain is the maximum itself.)
  * the adds of a cell, each rounded once with relative error 2^-24 of the result's magnitude.  The entry cell has the most:
    x = V + ld (Vmax + lmax), x + lx (Vmax + 2 lmax), U = s + ent (smax + Vmax + 2 lmax), V = U - N (Vmax); a head cell has
    U = s + V', V = U - N; the tail a = V + ls, U = s + (a | V'), V = U - N; the closing F one V + ld.  Plus the score tile's
    forward bound E_score (tests/hmm_dense_vit_np.py's `score_bound`).  The float64 reference reads the same float32 tables,
    so no table rounding enters.
  So delta = max E_score + 2^-24 (smax + 5 lmax + 4 Vmax), and the bar is 2 (n_good + 1) delta: derived, not measured.
"""
import itertools

import numpy as np

U24 = 2.0 ** -24


def exit_max(V, ld):
    """(x [K], xi [K]): x[j] = max_i (V[j][i] + ld[j][i]) and the lowest state (0-based) attaining it: an explicit loop over
    the states in ascending order with strict compares."""
    x = V[:, 0] + ld[:, 0]
    xi = np.zeros(V.shape[0], dtype=np.int64)
    for i in range(1, V.shape[1]):
        c = V[:, i] + ld[:, i]
        better = c > x
        x = np.where(better, c, x)
        xi[better] = i
    return x, xi


def viterbi_one(s, good, li, lx, ld, ls, dtype=np.float32):
    """(ids int32 [n], log_prob float, n_switch int, n_good int) of one utterance: s [n, K], good [n] bool.  The loops over the
    frames and over the duration states are explicit; the K x K candidates and the K units of a frame are numpy element-wise
    operations in `dtype`, which round each element exactly as a scalar loop would."""
    f = dtype
    s, li, lx, ld, ls = (np.asarray(a, dtype=f) for a in (s, li, lx, ld, ls))
    n, K = s.shape
    L = ld.shape[1]
    assert L >= 2 and ld.shape == (K, L) and lx.shape == (K, K)
    NEG = f(-np.inf)
    ids = np.full(n, -1, dtype=np.int32)
    frames = [t for t in range(n) if good[t]]
    if not frames:
        return ids, 0.0, 0, 0
    off_diag = lx.copy()
    off_diag[np.arange(K), np.arange(K)] = NEG                         # a unit is not entered from itself
    stay = np.zeros((n, K), dtype=bool)
    bp, xis = {}, {}
    V = None
    total = 0.0
    with np.errstate(invalid='ignore', over='ignore'):
        for t in frames:
            sk = s[t]
            U = np.full((K, L), NEG, dtype=f)
            if V is None:
                U[:, 0] = sk + li
                bp[t] = None
            else:
                x, xis[t] = exit_max(V, ld)
                cand = x[:, None] + off_diag                           # [j][k]
                bp[t] = np.argmax(cand, axis=0)                        # the first of the maxima: the lowest j (0 if all -inf)
                ent = cand[bp[t], np.arange(K)]
                a = V[:, L - 1] + ls
                below = V[:, L - 2]
                stay[t] = a > below                                    # strict: a tie goes to the advance
                U[:, L - 1] = sk + np.where(stay[t], a, below)
                for i in range(L - 2, 0, -1):
                    U[:, i] = sk + V[:, i - 1]
                U[:, 0] = sk + ent
            assert U.dtype == f
            N = U.max()
            V = U - N
            assert V.dtype == f
            total += float(N)
        x, xi = exit_max(V, ld)
    k = int(np.argmax(x))                                              # the lowest k of the maximum, then its lowest state
    i = int(xi[k])
    total += float(x[k])
    n_switch = 0
    for t in reversed(frames):
        ids[t] = k
        if i == L - 1 and stay[t, k]:
            continue
        if i > 0:
            i -= 1
            continue
        if bp[t] is None:
            break
        j = int(bp[t][k])
        k, i = j, int(xis[t][j])
        n_switch += 1
    return ids, total, n_switch, len(frames)


def viterbi(s, good, off, lens, li, lx, ld, ls, ids=None, dtype=np.float32):
    """The corpus call: (ids [T] int32, log_prob [n_utt] float64, n_switch [n_utt] int32, n_good [n_utt] int32).  Rows
    outside every utterance keep what `ids` held (-7 where none is given)."""
    T = np.asarray(s).shape[0]
    out = np.full(T, -7, dtype=np.int32) if ids is None else np.array(ids, dtype=np.int32)
    lp = np.zeros(len(off), dtype=np.float64)
    nsw = np.zeros(len(off), dtype=np.int32)
    ng = np.zeros(len(off), dtype=np.int32)
    for u, (o, n) in enumerate(zip(off, lens)):
        o, n = int(o), int(n)
        out[o:o + n], lp[u], nsw[u], ng[u] = viterbi_one(s[o:o + n], good[o:o + n], li, lx, ld, ls, dtype)
    return out, lp, nsw, ng


def runs(a):
    """[(id, length)] of the maximal runs of a sequence of ids."""
    out = []
    for v in np.asarray(a).tolist():
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return [(k, n) for k, n in out]


def duration_log_prob(ld, ls, k, n):
    """logp_k(n), float64."""
    L = ld.shape[1]
    return float(ld[k, n - 1]) if n < L else float(ld[k, L - 1]) + (n - L) * float(ls[k])


def segments_score(s64, frames, segs, li, lx, ld, ls):
    """The float64 score of the segments [(k, n)], neighbours distinct, laid over the good frames `frames`."""
    total, pos, prev = 0.0, 0, None
    for k, n in segs:
        assert k != prev and n >= 1
        total += float(li[k]) if prev is None else float(lx[prev, k])
        total += duration_log_prob(ld, ls, k, n)
        for t in frames[pos:pos + n]:
            total += float(s64[t, k])
        pos += n
        prev = k
    assert pos == len(frames)
    return total


def J_runs(s64, ids, good, li, lx, ld, ls):
    """The float64 score of a path given by its ids: the maximal runs of the ids over the good frames are its segments."""
    s64 = np.asarray(s64, dtype=np.float64)
    li, lx, ld, ls = (np.asarray(a, dtype=np.float64) for a in (li, lx, ld, ls))
    frames = [t for t in range(s64.shape[0]) if good[t]]
    if not frames:
        return 0.0
    return segments_score(s64, frames, runs(np.asarray(ids)[frames]), li, lx, ld, ls)


def brute_force(s, good, li, lx, ld, ls):
    """(the largest score, the set of id tuples over the good frames attaining it) over ALL segmentations whose neighbouring
    segments differ: tiny cases only."""
    s64 = np.asarray(s, dtype=np.float64)
    li, lx, ld, ls = (np.asarray(a, dtype=np.float64) for a in (li, lx, ld, ls))
    n_all, K = s64.shape
    frames = [t for t in range(n_all) if good[t]]
    n = len(frames)
    if not n:
        return 0.0, {()}
    best, arg = -np.inf, set()

    def compositions(left):
        if left == 0:
            yield ()
            return
        for first in range(1, left + 1):
            for rest in compositions(left - first):
                yield (first,) + rest

    for comp in compositions(n):
        for units in itertools.product(range(K), repeat=len(comp)):
            if any(a == b for a, b in zip(units, units[1:])):
                continue
            v = segments_score(s64, frames, list(zip(units, comp)), li, lx, ld, ls)
            path = tuple(k for k, m in zip(units, comp) for _ in range(m))
            if v > best:
                best, arg = v, {path}
            elif v == best:
                arg.add(path)
    return float(best), arg


def run_stats(ids, off, lens, K, L):
    """(dur [K, L] int64, tail [K] int64): for every maximal run, over the good frames (0 <= id < K) of one utterance, of unit k
    with length n: dur[k][min(n, L) - 1] += 1 and tail[k] += max(n - L, 0).  Explicit loops."""
    ids = np.asarray(ids)
    dur = np.zeros((K, L), dtype=np.int64)
    tail = np.zeros(K, dtype=np.int64)
    for o, n in zip(off, lens):
        cur, length = -1, 0
        for t in range(int(o), int(o) + int(n)):
            k = int(ids[t])
            if k < 0 or k >= K:
                continue
            if k == cur:
                length += 1
                continue
            if cur >= 0:
                dur[cur, min(length, L) - 1] += 1
                tail[cur] += max(length - L, 0)
            cur, length = k, 1
        if cur >= 0:
            dur[cur, min(length, L) - 1] += 1
            tail[cur] += max(length - L, 0)
    return dur, tail


def duration_update(dur, tail, q, r, alpha, floor=2.0 ** -80):
    """hmm.duration_update restated with loops over the units, float64."""
    dur, tail = np.asarray(dur, dtype=np.float64), np.asarray(tail, dtype=np.float64)
    q, r = np.array(q, dtype=np.float64), np.array(r, dtype=np.float64)
    K, L = q.shape
    for k in range(K):
        den = dur[k].sum() + L * alpha
        if den > 0:
            for d in range(L):
                q[k, d] = (dur[k, d] + alpha) / den
        rden = tail[k] + dur[k, L - 1] + 2.0 * alpha
        if rden > 0:
            r[k] = (tail[k] + alpha) / rden
        q[k] = np.maximum(q[k], floor)
        q[k] /= q[k].sum()
        r[k] = min(max(r[k], floor), 1.0 - 2.0 ** -24)
    return q, r


def duration_score(dur, tail, q, r):
    """The duration part of the paths' score that the statistics stand for, float64: sum over the runs of logp_k(n)."""
    dur, tail = np.asarray(dur, dtype=np.float64), np.asarray(tail, dtype=np.float64)
    L = q.shape[1]
    return float((dur * np.log(q)).sum() + (dur[:, L - 1] * np.log1p(-r)).sum() + (tail * np.log(r)).sum())


def log_tables64(init, trans, q, r):
    """(li, lx, ld, ls) in float64, unrounded: the tables of hmm.switch_log_transitions and hmm.duration_tables."""
    init, trans, q, r = (np.asarray(a, dtype=np.float64) for a in (init, trans, q, r))
    K = len(init)
    with np.errstate(all='ignore'):
        lx = np.log(trans / (1.0 - np.diag(trans))[:, None]) if K > 1 else np.zeros((1, 1))
    lx[np.arange(K), np.arange(K)] = 0.0
    ld = np.log(q)
    ld[:, -1] = np.log(q[:, -1] * (1.0 - r))
    return np.log(init), lx, ld, np.log(r)


PLANTED_LENGTHS = (3, 5, 7, 14)              # with L = 8 the last unit lives in the tail
PLANTED_L = 8


def planted_corpus(seed=0, n_utt=12):
    """The planted corpus of the duration-training tests: K = 4, D = 2, means at the corners of a square of side 6, unit
    variances; every utterance a sequence of 6 .. 11 whole segments, unit k always PLANTED_LENGTHS[k] frames long, the next
    unit drawn uniformly from the other three.  (x float32 [T, 2], lens, means [4, 2], true states)."""
    rng = np.random.RandomState(seed)
    means = np.array([[0.0, 0.0], [6.0, 0.0], [6.0, 6.0], [0.0, 6.0]])
    xs, zs, lens = [], [], []
    for _ in range(n_utt):
        k, z = rng.randint(4), []
        for _ in range(rng.randint(6, 12)):
            z += [k] * PLANTED_LENGTHS[k]
            k = (k + 1 + rng.randint(3)) % 4
        z = np.array(z, dtype=np.int64)
        xs.append(means[z] + rng.randn(len(z), 2))
        zs.append(z)
        lens.append(len(z))
    return np.concatenate(xs).astype(np.float32), np.array(lens), means, np.concatenate(zs)


def fit_viterbi(hmm, x, lens, shift, m, v, gv, trans, init, q, r, n_iter=10, tol=1e-4, params='mvtid', alpha=1e-3,
                var_floor=0.01, min_count=1.0):
    """The float64 training loop with explicit durations: (viterbi_log_probs, m, v, trans, init, q, r, ids of the last
    decoding).  hmm: the abnet3_amd.hmm module, for its two unchanged host updates; the decoder is this file's viterbi_one in
    float64 on unrounded float64 tables, the statistics tests/hmm_hard_np.py's (S = 1) and this file's run_stats, the
    duration update this file's."""
    import hmm_hard_np as hh
    x = np.asarray(x, dtype=np.float32)
    K, D = m.shape
    L = np.asarray(q).shape[1]
    off = np.cumsum(lens) - np.asarray(lens)
    m, v = np.array(m, dtype=np.float64), np.array(v, dtype=np.float64)
    trans, init = np.array(trans, dtype=np.float64), np.array(init, dtype=np.float64)
    q, r = np.array(q, dtype=np.float64), np.array(r, dtype=np.float64)
    mv, ti = ''.join(c for c in 'mv' if c in params), ''.join(c for c in 'ti' if c in params)
    lps, prev, ids = [], None, None
    for it in range(n_iter):
        s, bad = hh.scores64(x, shift, m, v)
        li, lx, ld, ls = log_tables64(init, trans, q, r)
        ids = np.full(x.shape[0], -1, dtype=np.int32)
        total, n = 0.0, 0
        for o, n_u in zip(off, lens):
            sl = slice(int(o), int(o) + int(n_u))
            res = viterbi_one(s[sl], ~bad[sl], li, lx, ld, ls, dtype=np.float64)
            ids[sl] = res[0]
            total += res[1]
            n += res[3]
        lps.append(total / n)
        n_changed = x.shape[0] if prev is None else int((ids != prev).sum())
        prev = ids
        if it > 0 and (lps[-1] - lps[-2] < tol or n_changed == 0):
            break
        counts, sums, _ = hh.hard_stats(x, off, lens, shift, ids, K, 1)
        dur, tail = run_stats(ids, off, lens, K, L)
        if mv:
            _, m, v, _, _ = hmm.baum_welch_update(sums, np.zeros(K), 0, m, v, gv, var_floor, min_count, mv, weights=np.full(K, 1.0 / K),
                                                  stay=0.0)
        trans, init = hmm.transition_update(counts.astype(np.float64), trans, init, alpha, ti)
        if 'd' in params:
            q, r = duration_update(dur, tail, q, r, alpha)
    return lps, m, v, trans, init, q, r, ids


def table_max(*tables):
    return max(float(np.abs(np.asarray(a, dtype=np.float64)).max()) for a in tables)


def delta(E, smax, lmax, L):
    """The per-cell perturbation of the module docstring."""
    vmax = 2.0 * (L + 2) * (float(smax) + 2.0 * float(lmax))
    return float(np.max(E)) + U24 * (float(smax) + 5.0 * float(lmax) + 4.0 * vmax)
