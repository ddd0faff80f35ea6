"""The max-product path of the full-transition HMM with a minimum unit duration (abnw_hmm_dense_viterbi_dur) restated in
numpy with explicit loops over frames and chain states (test infrastructure only): the reference its tests compare the
kernel with.  tests/hmm_dense_vit_np.py is the model without a minimum duration, tests/vit_dur_np.py the minimum duration
of the sticky model; this file joins the two.

The definition.  One utterance, good frames only (a BAD frame gets id -1 and is passed over; durations count good frames).
Every unit k is a left-to-right chain of S states with tied emissions of which only the last may repeat; a unit is left
only from its last state and only for a DIFFERENT unit.  A path is a sequence of segments (k_i, n_i) with k_i != k_{i+1};
every segment but the utterance's last has n_i >= S (the end of the utterance may cut the last one short); its score is
    sum of the frames' scores s[t, k] + li[k_1] + lt[k_{i-1}][k_i] for each later segment + max(n_i - S, 0) lt[k_i][k_i]
with li, lt hmm.log_transitions' tables.  Adjacent segments differ, so the maximal runs of a path's ids ARE its segments
(`J_runs`), and n_switch = segments - 1: there is no "re-entering the same unit" as in tests/vit_dur_np.py.

Recurrence for S >= 2, all float32, every operation one rounded add or a compare in the order written; V[k][0 .. S-1]
holds the normalised previous values:
    first good frame:   U[k][0] = s + li[k], every other state -inf
    later good frames:  ent[k] = max over j != k of (V[j][S-1] + lt[j][k]),  bp[k] = the lowest such j
                        U[k][0] = s + ent[k];   U[k][i] = s + V[k][i-1] for 0 < i < S-1
                        a = V[k][S-1] + lt[k][k],  st = a > V[k][S-2]  (strict: a tie goes to the advance)
                        U[k][S-1] = s + (st ? a : V[k][S-2])
    every good frame:   N_t = max over all (k, i) of U,  V = U - N_t,  log_prob += N_t (float64, frame order)
The max over j != k is taken as the kernel takes it: over ALL j in ascending order with strict compares, the diagonal
candidate being -inf.  Where a finite candidate exists that is the lowest j != k of the maximum; where none does (K = 1,
or no unit has reached its last state yet) ent is -inf and bp is 0 -- never read, because a state whose value is -inf is
on no best path.  The final state is the lowest k, then the largest i, with V[k][i] == 0.  Traceback over the good
frames backwards, from state (k, i) at a frame: i == S - 1 and st set -> (k, S-1);  otherwise i > 0 -> (k, i-1);
otherwise (i == 0) -> (bp[k], S-1), one switch -- unless the frame is the first good frame, where the walk ends.

S = 1 is NOT this recurrence (the diagonal would have to join the argmax): `viterbi_one` hands it to
tests/hmm_dense_vit_np.py, whose bits abnw_hmm_dense_viterbi_dur gives with min_duration = 1.

The allowance of the float comparison (`delta`), derived as the two predecessors derive theirs: the recurrence is exact
dynamic programming over cell values (score + incoming value) each perturbed by at most delta, so for every path
|J'(a) - J64(a)| <= n_good delta, and  J64(a64) >= J64(a*) >= J'(a*) - n delta >= J'(a64) - n delta >= J64(a64) - 2 n delta;
the device sum is J'(a*) up to the same roundings.  With smax the largest |score| and lmax the largest |table entry|:
  * a finite V[k][i] is at least -Vmax, Vmax = 6 S (smax + lmax).  tests/vit_dur_np.py's argument with one more step, because
    the best exit may be k's own, which k cannot be entered from.  A frame changes any path's score by at most smax + lmax
    in magnitude, so two paths drift apart by at most 2 (smax + lmax) a frame.  State (k, i) at frame t was entered at
    t - i from the best exit j != k of t' = t - i - 1 and has since lost at most lmax + (i + 1)(2 smax + lmax) against the
    best state of t.  That exit is within 2 S (2 smax + 2 lmax) of the best state of t': take the best state of frame
    t' - (2 S - 1), let it run to its unit's last state (S - 1 frames at most), and, if that unit is k, move to any other unit
    and through its S states -- 2 S - 1 frames; nearer the utterance's start than that, a unit j != k begun at the first good
    frame (li[j] >= -lmax) is in its last state at t' after at most 2 S - 1 frames as well, or no exit is finite and nor is
    the entry.  Together: 4 S (smax + lmax) + lmax + S (2 smax + lmax) <= 6 S (smax + lmax).  (K = 1: the one chain is the
    maximum itself.)
  * the adds of a cell, each rounded once, relative error 2^-24 of the result's magnitude.  The entry cell has the most:
    W = U[j][S-1] - N (Vmax), W + lt[j][k] (Vmax + lmax) -- only the candidate that is the maximum or within a rounding of it
    matters, rounding being monotone --, U = s + ent (smax + Vmax + lmax), V = U - N (Vmax); the exit cell has a = V + lt[k][k],
    U = s + (a | V'), V = U - N; a forced cell U = s + V', V = U - N: never more than those four adds at those magnitudes.
    Plus one table entry's rounding from float64 (lmax) and the score tile's forward bound E_score
    (tests/hmm_dense_vit_np.py's `score_bound`).
  So delta = max E_score + 2^-24 (smax + 3 lmax + 4 Vmax) = max E_score + 2^-24 ((24 S + 1) smax + (24 S + 3) lmax):
  tests/vit_dur_np.py's form with the wider Vmax.  The bar is derived, not measured.
"""
import itertools

import numpy as np

import hmm_dense_vit_np as dv
import vit_dur_np

U24 = 2.0 ** -24
NEG = np.float32(-np.inf)


def viterbi_one(s, good, li, lt, S):
    """(ids int32 [L], log_prob float, n_switch int, n_good int) of one utterance: s [L, K] float32, good [L] bool.  The
    loops over the frames and over the states of a chain are explicit; the K x K candidates and the K units of a frame are
    numpy element-wise float32 operations, which round each element exactly as a scalar loop would."""
    S = int(S)
    if S == 1:
        return dv.viterbi_one(s, good, li, lt)
    s = np.asarray(s, dtype=np.float32)
    li, lt = np.asarray(li, dtype=np.float32), np.asarray(lt, dtype=np.float32)
    L, K = s.shape
    ids = np.full(L, -1, dtype=np.int32)
    frames = [t for t in range(L) if good[t]]
    if not frames:
        return ids, 0.0, 0, 0
    ls = np.diag(lt).copy()
    off_diag = lt.copy()
    off_diag[np.arange(K), np.arange(K)] = NEG                         # a unit is not entered from itself
    stay = np.zeros((L, K), dtype=bool)
    bp = {}
    V = None
    total = 0.0
    with np.errstate(invalid='ignore', over='ignore'):
        for t in frames:
            sk = s[t]
            Uv = np.full((K, S), NEG, dtype=np.float32)
            if V is None:
                Uv[:, 0] = sk + li
                bp[t] = None
            else:
                cand = V[:, S - 1][:, None] + off_diag                 # [j][k]
                bp[t] = np.argmax(cand, axis=0)                        # the first of the maxima: the lowest j (0 if all -inf)
                ent = cand[bp[t], np.arange(K)]
                a = V[:, S - 1] + ls
                below = V[:, S - 2]
                stay[t] = a > below                                    # strict: a tie goes to the advance
                last = sk + np.where(stay[t], a, below)
                for i in range(S - 2, 0, -1):
                    Uv[:, i] = sk + V[:, i - 1]
                Uv[:, 0] = sk + ent
                Uv[:, S - 1] = last
            assert Uv.dtype == np.float32
            N = Uv.max()
            V = Uv - N
            assert V.dtype == np.float32
            total += float(N)
    k = int(np.flatnonzero((V == 0).any(axis=1))[0])                   # the final state: the lowest k, then the largest i, at 0
    i = int(np.flatnonzero(V[k] == 0)[-1])
    n_switch = 0
    for t in reversed(frames):
        ids[t] = k
        if i == S - 1 and stay[t, k]:
            continue
        if i > 0:
            i -= 1
            continue
        if bp[t] is None:
            break
        k, i = int(bp[t][k]), S - 1
        n_switch += 1
    return ids, total, n_switch, len(frames)


def viterbi(s, good, off, lens, li, lt, S, ids=None):
    """The corpus call: (ids [T] int32, log_prob [n_utt] float64, n_switch [n_utt] int32, n_good [n_utt] int32).  Rows
    outside every utterance keep what `ids` held (-7 where none is given)."""
    T = np.asarray(s).shape[0]
    out = np.full(T, -7, dtype=np.int32) if ids is None else np.array(ids, dtype=np.int32)
    lp = np.zeros(len(off), dtype=np.float64)
    nsw = np.zeros(len(off), dtype=np.int32)
    ng = np.zeros(len(off), dtype=np.int32)
    for u, (o, n) in enumerate(zip(off, lens)):
        o, n = int(o), int(n)
        out[o:o + n], lp[u], nsw[u], ng[u] = viterbi_one(s[o:o + n], good[o:o + n], li, lt, S)
    return out, lp, nsw, ng


runs = vit_dur_np.runs
run_lengths_ok = vit_dur_np.run_lengths_ok


def segments_score(s64, frames, segs, li, lt, S):
    """The float64 score of the segments [(k, n)], neighbours distinct, laid over the good frames `frames`."""
    total, pos, prev = 0.0, 0, None
    for k, n in segs:
        assert k != prev
        total += float(li[k]) if prev is None else float(lt[prev, k])
        total += (n - S) * float(lt[k, k]) if n > S else 0.0
        for t in frames[pos:pos + n]:
            total += float(s64[t, k])
        pos += n
        prev = k
    return total


def J_runs(s64, ids, good, li, lt, S):
    """The float64 score of a path given by its ids: the maximal runs of the ids are its segments."""
    s64 = np.asarray(s64, dtype=np.float64)
    li, lt = np.asarray(li, dtype=np.float64), np.asarray(lt, dtype=np.float64)
    frames = [t for t in range(s64.shape[0]) if good[t]]
    if not frames:
        return 0.0
    return segments_score(s64, frames, runs(np.asarray(ids)[frames]), li, lt, S)


def brute_force(s, good, li, lt, S):
    """(the largest score, the set of id tuples over the good frames attaining it) over ALL segmentations whose
    neighbouring segments differ and of which only the last may be shorter than S: tiny cases only."""
    s64 = np.asarray(s, dtype=np.float64)
    li, lt = np.asarray(li, dtype=np.float64), np.asarray(lt, dtype=np.float64)
    L, K = s64.shape
    frames = [t for t in range(L) if good[t]]
    n = len(frames)
    if not n:
        return 0.0, {()}
    best, arg = -np.inf, set()

    def compositions(left):
        if left == 0:
            yield ()
            return
        for first in range(1, left + 1):
            if first < S and first != left:          # only the last segment may be shorter than S
                continue
            for rest in compositions(left - first):
                yield (first,) + rest

    for comp in compositions(n):
        for units in itertools.product(range(K), repeat=len(comp)):
            if any(a == b for a, b in zip(units, units[1:])):
                continue
            v = segments_score(s64, frames, list(zip(units, comp)), li, lt, S)
            path = tuple(k for k, m in zip(units, comp) for _ in range(m))
            if v > best:
                best, arg = v, {path}
            elif v == best:
                arg.add(path)
    return float(best), arg


def optimum_f64(s64, good, li, lt, S):
    """The float64 maximum over one utterance by the textbook DP over the K x S states (no normalisation, no ids)."""
    S = int(S)
    if S == 1:
        return dv.optimum_f64(s64, good, li, lt)
    s64 = np.asarray(s64, dtype=np.float64)
    li, lt = np.asarray(li, dtype=np.float64), np.asarray(lt, dtype=np.float64)
    K = s64.shape[1]
    ls = np.diag(lt).copy()
    off_diag = lt.copy()
    off_diag[np.arange(K), np.arange(K)] = -np.inf
    V = None
    with np.errstate(invalid='ignore'):
        for t in range(s64.shape[0]):
            if not good[t]:
                continue
            Un = np.full((K, S), -np.inf)
            if V is None:
                Un[:, 0] = s64[t] + li
            else:
                ent = (V[:, S - 1][:, None] + off_diag).max(axis=0)
                last = s64[t] + np.maximum(V[:, S - 1] + ls, V[:, S - 2])
                for i in range(S - 2, 0, -1):
                    Un[:, i] = s64[t] + V[:, i - 1]
                Un[:, 0] = s64[t] + ent
                Un[:, S - 1] = last
            V = Un
    return 0.0 if V is None else float(V.max())


score_bound = dv.score_bound
table_max = dv.table_max


def delta(E, smax, lmax, S):
    """The per-cell perturbation of the module docstring."""
    vmax = 6.0 * S * (float(smax) + float(lmax))
    return float(np.max(E)) + U24 * (float(smax) + 3.0 * float(lmax) + 4.0 * vmax)
