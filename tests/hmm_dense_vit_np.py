"""The max-product path of abnet3_amd/hmm.py's full-transition HMM restated in numpy (test infrastructure only): the
reference the tests of abnz_hmm_dense_viterbi compare the kernel with.

The model is tests/hmm_dense_np.py's: states = the K components, init [K], trans [K][K] row-stochastic, emissions
s[t, k] = logN[t, k]; a BAD frame is passed over.  The log tables li = log init32, lt = log trans32 are taken in float64 from
the float32 init / trans and rounded once to float32.  Recurrence over the good frames, every operation one add or a
compare in `dtype`:
    first:  u[k] = s[k] + li[k]
    later:  c[k] = max_j (W[j] + lt[j][k]),  bp[k] = the lowest j that attains it,  u[k] = s[k] + c[k]
    every:  M = max_k u[k],  W = u - M,  log_prob += M (a float64 sum in frame order)
The final state is the lowest k with W[k] == 0 (the lowest index of the maximum of u); backwards ids[t] = cur, then
cur = bp_t[cur]: of all optimal paths the smallest one when read from the last frame to the first.  The loop over the
frames is explicit; the K x K candidates of a frame are numpy element-wise operations, which round each element exactly
as a scalar loop would, and np.argmax returns the first of the maxima.

The allowance of the float comparison (`delta`).  Let s64 be the float64 scores of the fp32 operands, the tables the fp32
tables read as float64, and J64(a) the log joint of a path a evaluated with them in float64.  The kernel's recurrence is
exact dynamic programming for a problem whose cell values (score + incoming log transition) are perturbed by e[t, k].
lmax is the largest |li|, |lt|; the tables are logarithms of probabilities, so they are <= 0 up to check_transitions' 1e-3
slack on a row sum, which the factor 2 below swallows.
  * the score tile: a dot product of depth n = 2D + 1 whose xc^2 operands were rounded once, accumulated in fp32 in some
    order: |fp32 score - s64| <= (n + 2) 2^-24 sum|terms| (1 + 2^-10), sum|terms| = gmm_np.score_scale -- `score_bound`, E;
  * the tables' one rounding from float64: 2^-24 lmax on the one table entry a cell's incoming value uses (nothing against
    J64, which reads the rounded tables; it is the distance to the model's own float64 tables, kept so that one delta
    serves both comparisons);
  * the step's three roundings.  The previous frame's maximum j* has W[j*] = 0, so c[k] >= lt[j*][k] >= -lmax, and c[k] <= lmax.
    a = W[j] + lt[j][k] matters only where it is the maximum or within a rounding of it: there |a| <= lmax and its
    rounding is at most 2^-24 lmax (rounding is monotone, so an error in a candidate far below the maximum cannot lift it
    over).  W[j] = u[j] - M feeds only such an a: where it matters |W[j]| = |a - lt[j][k]| <= 2 lmax, 2^-24 x 2 lmax.
    u = s + c (s + li at the first good frame) is at most smax + lmax in magnitude: 2^-24 (smax + lmax).  An error in
    W[j] at frame t is an error of the cells (t + 1, .)'s incoming values through j.
  So |e| <= delta = max E + 2^-24 (smax + 5 lmax) per good frame, and for every path |J'(a) - J64(a)| <= n_good delta.
  The device path a* maximises J', the float64 path a64 maximises J64:
      J64(a64) >= J64(a*) >= J'(a*) - n delta >= J'(a64) - n delta >= J64(a64) - 2 n delta,
  and the device log_prob is J'(a*) up to the same roundings: within 2 n delta of J64(a64) as well.  The bar is derived,
  not measured.
"""
import itertools

import numpy as np

U = 2.0 ** -24


def log_transitions(init, trans, dtype=np.float32):
    """(li [K], lt [K, K]) in `dtype` from float32(init), float32(trans): float32 is hmm.log_transitions."""
    i32, t32 = np.asarray(init, dtype=np.float32), np.asarray(trans, dtype=np.float32)
    return np.log(i32.astype(np.float64)).astype(dtype), np.log(t32.astype(np.float64)).astype(dtype)


def sticky_log_transitions(ls, lr):
    """lt [K, K] of the sticky model's tables: lt[j][k] = lr[k] off the diagonal and ls[k] on it."""
    ls, lr = np.asarray(ls), np.asarray(lr)
    K = len(ls)
    lt = np.repeat(lr[None, :], K, axis=0).copy()
    lt[np.arange(K), np.arange(K)] = ls
    return lt


def viterbi_one(s, good, li, lt, dtype=np.float32, count_ties=False):
    """(ids int32 [L], log_prob float, n_switch int, n_good int) of one utterance: s [L, K], good [L] bool.  count_ties: a
    fifth element, the number of good frames where the argmax over j of the CHOSEN cell -- or, at the last good frame, the
    final argmax over k -- is not unique."""
    s = np.asarray(s).astype(dtype)
    li, lt = np.asarray(li).astype(dtype), np.asarray(lt).astype(dtype)
    L, K = s.shape
    ids = np.full(L, -1, dtype=np.int32)
    frames = [t for t in range(L) if good[t]]
    if not frames:
        return (ids, 0.0, 0, 0, 0) if count_ties else (ids, 0.0, 0, 0)
    bp, tied = {}, {}
    W, last = None, 0
    log_prob = 0.0
    with np.errstate(invalid='ignore'):
        for t in frames:
            if W is None:
                u = (s[t] + li).astype(dtype)
                bp[t] = np.arange(K)
                tied[t] = np.zeros(K, dtype=bool)
            else:
                cand = (W[:, None] + lt).astype(dtype)             # [j][k]
                bp[t] = np.argmax(cand, axis=0)                    # the first of the maxima: the lowest j
                c = cand[bp[t], np.arange(K)]
                tied[t] = (cand == c[None, :]).sum(axis=0) > 1
                u = (s[t] + c).astype(dtype)
            last = int(np.argmax(u))                               # the lowest index of the maximum
            M = u[last]
            final_tie = int((u == M).sum() > 1)
            W = (u - M).astype(dtype)
            log_prob += float(M)
    cur, n_switch, n_ties = last, 0, final_tie
    for t in reversed(frames):
        ids[t] = cur
        n_ties += int(tied[t][cur])
        prev = int(bp[t][cur])
        n_switch += int(prev != cur)
        cur = prev
    out = (ids, log_prob, n_switch, len(frames))
    return out + (n_ties,) if count_ties else out


def viterbi(s, good, off, lens, li, lt, dtype=np.float32, ids=None):
    """The corpus call: (ids [T] int32, log_prob [n_utt] float64, n_switch [n_utt] int32, n_good [n_utt] int32).  Rows
    outside every utterance keep what `ids` held (-7 where none is given)."""
    T = np.asarray(s).shape[0]
    out = np.full(T, -7, dtype=np.int32) if ids is None else np.array(ids, dtype=np.int32)
    lp = np.zeros(len(off), dtype=np.float64)
    nsw = np.zeros(len(off), dtype=np.int32)
    ng = np.zeros(len(off), dtype=np.int32)
    for u, (o, n) in enumerate(zip(off, lens)):
        o, n = int(o), int(n)
        out[o:o + n], lp[u], nsw[u], ng[u] = viterbi_one(s[o:o + n], good[o:o + n], li, lt, dtype)
    return out, lp, nsw, ng


def ties(s, good, off, lens, li, lt, dtype=np.float32):
    """The corpus' tie count (viterbi_one's count_ties summed over the utterances)."""
    return sum(viterbi_one(s[int(o):int(o) + int(n)], good[int(o):int(o) + int(n)], li, lt, dtype, True)[4] for o, n in zip(off, lens))


def switches(ids):
    a = np.asarray(ids)
    a = a[a >= 0]
    return int((a[1:] != a[:-1]).sum())


def optimum_f64(s64, good, li, lt):
    """The float64 maximum of the log joint over one utterance by the textbook DP (no normalisation, no ids)."""
    li, lt = np.asarray(li, dtype=np.float64), np.asarray(lt, dtype=np.float64)
    s64 = np.asarray(s64, dtype=np.float64)
    V = None
    for t in range(s64.shape[0]):
        if not good[t]:
            continue
        V = s64[t] + li if V is None else s64[t] + (V[:, None] + lt).max(axis=0)
    return 0.0 if V is None else float(V.max())


def J(s64, ids, good, li, lt):
    """The float64 log joint of a given path (ids at the good frames; the BAD frames are skipped)."""
    li, lt = np.asarray(li, dtype=np.float64), np.asarray(lt, dtype=np.float64)
    s64 = np.asarray(s64, dtype=np.float64)
    total, prev = 0.0, None
    for t in range(s64.shape[0]):
        if not good[t]:
            continue
        k = int(ids[t])
        total += s64[t, k] + (li[k] if prev is None else lt[prev, k])
        prev = k
    return float(total)


def brute_force(s, good, li, lt):
    """(the largest log joint, the optimal path that is smallest when read from the last good frame to the first) by
    enumeration of all K^n paths over the good frames, in float64 from the tables as given: tiny cases only."""
    s = np.asarray(s, dtype=np.float64)
    li, lt = np.asarray(li, dtype=np.float64), np.asarray(lt, dtype=np.float64)
    L, K = s.shape
    frames = [t for t in range(L) if good[t]]
    if not frames:
        return 0.0, ()
    best, arg = -np.inf, None
    for z in itertools.product(range(K), repeat=len(frames)):
        v = li[z[0]] + s[frames[0], z[0]]
        for i in range(1, len(frames)):
            v += lt[z[i - 1], z[i]] + s[frames[i], z[i]]
        if v > best or (v == best and z[::-1] < arg[::-1]):
            best, arg = v, z
    return float(best), arg


def score_bound(scale, D):
    """The forward bound of an fp32 dot product of depth 2D + 1 (module docstring) from gmm_np.score_scale's sums."""
    return (2 * D + 3) * U * (1.0 + 2.0 ** -10) * np.asarray(scale, dtype=np.float64)


def table_max(li, lt):
    """The largest magnitude in the two tables."""
    return float(max(np.abs(np.asarray(li, dtype=np.float64)).max(), np.abs(np.asarray(lt, dtype=np.float64)).max()))


def delta(E, smax, lmax):
    """The per-cell perturbation of the module docstring."""
    return float(np.max(E)) + U * (float(smax) + 5.0 * float(lmax))
