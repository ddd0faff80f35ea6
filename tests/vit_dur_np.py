"""The two max-product decoders with a minimum unit duration (abnx_kmeans_viterbi_dur, abnx_hmm_viterbi_dur) restated in
numpy with explicit loops over frames and states (test infrastructure only): the reference the minimum-duration tests compare the kernels with.

The definition.  One utterance, good frames only (a BAD frame gets id -1 and is passed over; durations count good frames).
Every unit k is a left-to-right chain of S states with tied emissions of which only the last may repeat.  A path is a
sequence of segments (k_i, n_i); every segment but the utterance's last has n_i >= S (the end of the utterance may cut the
last one short); its score is
    sum of the frames' scores s[t, k] + lw[k_1] + lr[k_i] for each later segment + max(n_i - S, 0) ls[k_i].
Tables: the sticky HMM's are hmm.viterbi_tables' (lw, ls, lr); the k-means decoder's are lw = 0, ls = 0, lr = -p with
p = fp32(penalty / 2) (`kmeans_tables`).

Recurrence, all float32, every operation one rounded add or a compare in the order written; V[k][0 .. S-1] holds the
normalised previous values, E = max_k V[k][S-1], exitj the lowest k whose U[k][S-1] was the largest (0 if all are -inf):
    first good frame:   U[k][0] = s + lw[k], every other state -inf
    later good frames:  U[k][0] = s + (E + lr[k]);   U[k][i] = s + V[k][i-1] for 0 < i < S-1;
                        a = V[k][S-1] + ls[k],  st = a > V[k][S-2]  (strict; S = 1: a > E + lr[k]),
                        U[k][S-1] = s + (st ? a : V[k][S-2])
    every good frame:   N_t = max over all (k, i) of U,  V = U - N_t,  log_prob / objective = sum of the N_t (float64).
E is formed as (max_k U[k][S-1]) - N_t, which is max_k V[k][S-1] because rounding is monotone; exitj is taken over U, so
where the subtraction rounds two different U to one V it is the lowest k of the larger U (it attains E either way).
The final state is the lowest k, then the largest i, with V[k][i] == 0.  Traceback over the good frames backwards, from
state (k, i) at a frame: i == S - 1 and st set -> (k, S-1);  otherwise i > 0 -> (k, i-1);  otherwise (i == 0) -> (that
frame's recorded exitj of the previous good frame, S-1).  n_switch = the changes of id along the path.

With S = 1 this is tests/hmm_vit_np.py's and tests/units_np.py's recurrence.

Re-entering the same unit.  Two adjacent segments of one unit k, the second of n2 frames, score ls[k] min(n2, S) - lr[k]
LESS than the one merged segment.  So where S ls[k] >= lr[k] for every k (the k-means tables always: ls = 0) the maximal
runs of a path's ids are its best segmentation and `J_runs` is the score of the ids; where it fails (a small stay
probability and a large S) the best path may close a unit and enter it again, which its ids do not show.  The run-length
property (every run of ids but an utterance's last is >= S) holds either way: merging only lengthens runs.

The allowance of the float comparison (`delta`), derived as tests/hmm_vit_np.py derives its own: the recurrence is exact
dynamic programming over cell values (score + incoming value) each perturbed by at most delta, so for every path
|J'(a) - J64(a)| <= n_good delta, and  J64(a64) >= J64(a*) >= J'(a*) - n delta >= J'(a64) - n delta >= J64(a64) - 2 n delta;
the device sum is J'(a*) up to the same roundings.  What differs from S = 1 is the magnitude of the values that are
rounded: a state inside a forced advance cannot be abandoned, so its V is not confined to (lr, 0].  With smax the largest
|score| and lmax the largest finite |table entry|:
  * a finite V[k][i] is at least -Vmax, Vmax = 4 S (smax + lmax).  (The best state S - 1 frames ago, continued in its own
    unit, is in an exit state now and has lost at most (S-1)(2 smax + 2 lmax) against any other path: E >= that.  State
    (k, i) was entered i + 1 frames ago from the best exit of then and has lost at most lmax + (i + 1)(2 smax + lmax) more.)
  * the adds of a cell, each rounded once, relative error 2^-24 of the result's magnitude: the entry cell has the most,
    E = x - N (Vmax), ent = E + lr (Vmax + lmax), U = s + ent (smax + Vmax + lmax), V = U - N (Vmax); the exit cell has
    a = V + ls, U = s + (a | V'), V = U - N, the forced cell U = s + V', V = U - N: never more than these four adds at
    these magnitudes; plus one table entry's rounding from float64 (lmax) and the score tile's forward bound E_score.
  So delta = max E_score + 2^-24 (smax + 3 lmax + 4 Vmax) = max E_score + 2^-24 ((16 S + 1) smax + (16 S + 3) lmax).
"""
import itertools

import numpy as np

U24 = 2.0 ** -24
NEG = np.float32(-np.inf)


def kmeans_tables(K, p):
    """(lw, ls, lr) [K] float32 of the penalised k-means decoder: 0, 0, -p."""
    z = np.zeros(K, dtype=np.float32)
    return z, z.copy(), np.full(K, -np.float32(p), dtype=np.float32)


def viterbi_one(s, good, lw, ls, lr, S):
    """(ids int32 [L], log_prob float, n_switch int, n_good int) of one utterance: s [L, K] float32, good [L] bool.  The
    loops over the frames and over the states of a chain are explicit; the K units of a frame are numpy element-wise
    float32 operations, which round each element exactly as a scalar loop would."""
    s = np.asarray(s, dtype=np.float32)
    lw, ls, lr = (np.asarray(a, dtype=np.float32) for a in (lw, ls, lr))
    L, K = s.shape
    S = int(S)
    ids = np.full(L, -1, dtype=np.int32)
    frames = [t for t in range(L) if good[t]]
    if not frames:
        return ids, 0.0, 0, 0
    stay = np.zeros((L, K), dtype=bool)
    pred = {}
    V, E, jprev = None, None, -1
    total = 0.0
    with np.errstate(invalid='ignore', over='ignore'):
        for t in frames:
            sk = s[t]
            Uv = np.full((K, S), NEG, dtype=np.float32)
            if V is None:
                Uv[:, 0] = sk + lw
            else:
                ent = E + lr
                a = V[:, S - 1] + ls
                below = ent if S == 1 else V[:, S - 2]
                stay[t] = a > below                                    # strict: a tie goes to the advance
                last = sk + np.where(stay[t], a, below)
                for i in range(S - 2, 0, -1):
                    Uv[:, i] = sk + V[:, i - 1]
                if S > 1:
                    Uv[:, 0] = sk + ent
                Uv[:, S - 1] = last
            assert Uv.dtype == np.float32
            N = Uv.max()
            j = int(np.argmax(Uv[:, S - 1]))                           # the first of the maxima: the lowest index (0 if all -inf)
            V = Uv - N
            E = Uv[j, S - 1] - N
            assert V.dtype == np.float32 and E.dtype == np.float32
            total += float(N)
            pred[t] = jprev
            jprev = j
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
        if pred[t] < 0:
            break
        n_switch += int(pred[t] != k)
        k, i = pred[t], S - 1
    return ids, total, n_switch, len(frames)


def viterbi(s, good, off, lens, lw, ls, lr, S, ids=None):
    """The corpus call: (ids [T] int32, log_prob [n_utt] float64, n_switch [n_utt] int32, n_good [n_utt] int32).  Rows
    outside every utterance keep what `ids` held (-7 where none is given)."""
    T = np.asarray(s).shape[0]
    out = np.full(T, -7, dtype=np.int32) if ids is None else np.array(ids, dtype=np.int32)
    lp = np.zeros(len(off), dtype=np.float64)
    nsw = np.zeros(len(off), dtype=np.int32)
    ng = np.zeros(len(off), dtype=np.int32)
    for u, (o, n) in enumerate(zip(off, lens)):
        o, n = int(o), int(n)
        out[o:o + n], lp[u], nsw[u], ng[u] = viterbi_one(s[o:o + n], good[o:o + n], lw, ls, lr, S)
    return out, lp, nsw, ng


def runs(ids):
    """[(unit, length)]: the maximal runs of the ids over the good frames (BAD frames, id -1, are passed over)."""
    a = [int(v) for v in np.asarray(ids) if v >= 0]
    out = []
    for v in a:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return [(k, n) for k, n in out]


def run_lengths_ok(ids, S):
    """Every run of the ids but the utterance's last is at least S good frames long."""
    return all(n >= S for _, n in runs(ids)[:-1])


def segments_score(s64, frames, segs, lw, ls, lr, S):
    """The float64 score of the segments [(k, n)] laid over the good frames `frames`."""
    total, pos = 0.0, 0
    for i, (k, n) in enumerate(segs):
        total += float(lw[k]) if i == 0 else float(lr[k])
        total += max(n - S, 0) * float(ls[k]) if n > S else 0.0
        for t in frames[pos:pos + n]:
            total += float(s64[t, k])
        pos += n
    return total


def J_runs(s64, ids, good, lw, ls, lr, S):
    """The float64 score of a path given by its ids, with the maximal runs of the ids as its segments."""
    s64 = np.asarray(s64, dtype=np.float64)
    lw, ls, lr = (np.asarray(a, dtype=np.float64) for a in (lw, ls, lr))
    frames = [t for t in range(s64.shape[0]) if good[t]]
    if not frames:
        return 0.0
    return segments_score(s64, frames, runs(np.asarray(ids)[frames]), lw, ls, lr, S)


def brute_force(s, good, lw, ls, lr, S):
    """(the largest score, the set of id tuples over the good frames attaining it) over ALL segmentations -- adjacent
    segments of one unit included --: tiny cases only."""
    s64 = np.asarray(s, dtype=np.float64)
    lw, ls, lr = (np.asarray(a, dtype=np.float64) for a in (lw, ls, lr))
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

    with np.errstate(invalid='ignore'):
        for comp in compositions(n):
            for units in itertools.product(range(K), repeat=len(comp)):
                v = segments_score(s64, frames, list(zip(units, comp)), lw, ls, lr, S)
                if np.isnan(v):
                    continue
                path = tuple(k for k, m in zip(units, comp) for _ in range(m))
                if v > best:
                    best, arg = v, {path}
                elif v == best:
                    arg.add(path)
    return float(best), arg


def optimum_f64(s64, good, lw, ls, lr, S):
    """The float64 maximum over one utterance by the textbook DP over the K x S states (no normalisation, no ids)."""
    s64 = np.asarray(s64, dtype=np.float64)
    lw, ls, lr = (np.asarray(a, dtype=np.float64) for a in (lw, ls, lr))
    K = s64.shape[1]
    V = None
    with np.errstate(invalid='ignore'):
        for t in range(s64.shape[0]):
            if not good[t]:
                continue
            Un = np.full((K, S), -np.inf)
            if V is None:
                Un[:, 0] = s64[t] + lw
            else:
                ent = V[:, S - 1].max() + lr
                below = ent if S == 1 else V[:, S - 2]
                last = s64[t] + np.maximum(V[:, S - 1] + ls, below)
                for i in range(S - 2, 0, -1):
                    Un[:, i] = s64[t] + V[:, i - 1]
                if S > 1:
                    Un[:, 0] = s64[t] + ent
                Un[:, S - 1] = last
            V = Un
    return 0.0 if V is None else float(V.max())


def delta(E, smax, lmax, S):
    """The per-cell perturbation of the module docstring."""
    vmax = 4.0 * S * (float(smax) + float(lmax))
    return float(np.max(E)) + U24 * (float(smax) + 3.0 * float(lmax) + 4.0 * vmax)
