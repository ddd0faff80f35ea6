"""The max-product path of abnet3_amd/hmm.py's sticky HMM restated in numpy (test infrastructure only): the reference the
Viterbi tests compare the kernel with.

The model is tests/hmm_np.py's: states = the K components, initial distribution w, transitions
a[j, k] = rho [j == k] + (1 - rho) w[k], emissions s[t, k] = logN[t, k]; a BAD frame is passed over.  The log tables, all
from w32 = float32(w), r = float32(stay), omr = float32(1) - r, in float64 and rounded once to float32:
    lw = log w32,   ls = log(r + omr w32),   lr = log(omr w32)       (lw = lr = -inf where w32 == 0).
Recurrence over the good frames, every operation one add or a compare in `dtype`:
    first:  u[k] = s[k] + lw[k]
    later:  a = W[k] + ls[k],  st[k] = a > lr[k] (strict),  u[k] = s[k] + (st[k] ? a : lr[k])
    every:  M = max_k u[k],  j* its lowest index,  W = u - M,  log_prob += M (a float64 sum)
and the frame records st and the previous good frame's j*.  Traceback from the last good frame's j*: a frame keeps cur
while st[cur], otherwise cur becomes the recorded predecessor.  The loop over the frames is explicit; the K lanes of a
frame are numpy element-wise operations, which round each element exactly as a scalar loop would.

The allowance of the float comparison (`delta`).  Let s64 be the float64 scores of the fp32 operands, the tables the
fp32 tables read as float64, and J64(a) the log joint of a path a evaluated with them in float64.  The kernel's recurrence
is exact dynamic programming for a problem whose cell values (score + incoming log transition) are perturbed by e[t, k]:
  * the score tile: a dot product of depth n = 2D + 1 whose xc^2 operands were rounded once, accumulated in fp32 in some
    order: |fp32 score - s64| <= (n + 2) 2^-24 sum|terms| (1 + 2^-10), sum|terms| = gmm_np.score_scale -- `score_bound`;
  * the tables' one rounding from float64: 2^-24 lmax on the one table entry a cell's incoming value uses, lmax the
    largest finite |lw|, |ls|, |lr| (nothing against J64, which reads the rounded tables; it is the distance to the
    model's own float64 tables, and it is kept in the allowance so that one delta serves both comparisons);
  * the step's three roundings.  a = W + ls matters only where it is used or where the comparison a > lr is within a
    rounding of flipping; there lr < a <= 0 up to that rounding, so |a| <= lmax and the rounding is at most 2^-24 lmax.
    W = u - M feeds only that a: where it matters |W| = |a - ls| <= lmax, 2^-24 lmax again (rounding is monotone, so an
    error in a W far below lr - ls cannot lift it over the threshold).  u = s + (a | lr | lw) is at most smax + lmax in
    magnitude: 2^-24 (smax + lmax).  An error in W[k] at frame t is an error of cell (t + 1, k)'s incoming value.
  So |e| <= delta = max E + 2^-24 (smax + 4 lmax) per good frame, and for every path |J'(a) - J64(a)| <= n_good delta.
  The device path a* maximises J', the float64 path a64 maximises J64:
      J64(a64) >= J64(a*) >= J'(a*) - n delta >= J'(a64) - n delta >= J64(a64) - 2 n delta,
  and the device log_prob is J'(a*) up to the same roundings: within 2 n delta of J64(a64) as well.
"""
import itertools

import numpy as np

U = 2.0 ** -24


def tables(w, stay, dtype=np.float32):
    """(lw, ls, lr) [K] in `dtype`: float32 is hmm.viterbi_tables; float64 keeps the unrounded logarithms."""
    w32 = np.asarray(w, dtype=np.float32).ravel()
    r = np.float32(stay)
    omr = np.float32(1.0) - r
    w64 = w32.astype(np.float64)
    with np.errstate(divide='ignore'):
        lw = np.log(w64)
        ls = np.log(np.float64(r) + np.float64(omr) * w64)
        lr = np.log(np.float64(omr) * w64)
    return lw.astype(dtype), ls.astype(dtype), lr.astype(dtype)


def viterbi_one(s, good, lw, ls, lr, dtype=np.float32):
    """(ids int32 [L], log_prob float, n_switch int, n_good int) of one utterance: s [L, K], good [L] bool."""
    s = np.asarray(s).astype(dtype)
    lw, ls, lr = (np.asarray(a).astype(dtype) for a in (lw, ls, lr))
    L, K = s.shape
    ids = np.full(L, -1, dtype=np.int32)
    frames = [t for t in range(L) if good[t]]
    if not frames:
        return ids, 0.0, 0, 0
    stay = np.zeros((L, K), dtype=bool)
    pred = {}
    W, jprev = None, -1
    log_prob = 0.0
    with np.errstate(invalid='ignore'):
        for t in frames:
            if W is None:
                u = (s[t] + lw).astype(dtype)
            else:
                a = (W + ls).astype(dtype)
                stay[t] = a > lr
                u = (s[t] + np.where(stay[t], a, lr)).astype(dtype)
            j = int(np.argmax(u))                      # the first of the maxima: the lowest index
            M = u[j]
            W = (u - M).astype(dtype)
            log_prob += float(M)
            pred[t] = jprev
            jprev = j
    cur, n_switch = jprev, 0
    for t in reversed(frames):
        ids[t] = cur
        if pred[t] >= 0 and not stay[t, cur]:
            n_switch += int(pred[t] != cur)
            cur = pred[t]
    return ids, log_prob, n_switch, len(frames)


def viterbi(s, good, off, lens, lw, ls, lr, dtype=np.float32, ids=None):
    """The corpus call: (ids [T] int32, log_prob [n_utt] float64, n_switch [n_utt] int32, n_good [n_utt] int32).  Rows
    outside every utterance keep what `ids` held (-7 where none is given)."""
    T = np.asarray(s).shape[0]
    out = np.full(T, -7, dtype=np.int32) if ids is None else np.array(ids, dtype=np.int32)
    lp = np.zeros(len(off), dtype=np.float64)
    nsw = np.zeros(len(off), dtype=np.int32)
    ng = np.zeros(len(off), dtype=np.int32)
    for u, (o, n) in enumerate(zip(off, lens)):
        o, n = int(o), int(n)
        out[o:o + n], lp[u], nsw[u], ng[u] = viterbi_one(s[o:o + n], good[o:o + n], lw, ls, lr, dtype)
    return out, lp, nsw, ng


def switches(ids):
    a = np.asarray(ids)
    a = a[a >= 0]
    return int((a[1:] != a[:-1]).sum())


def optimum_f64(s64, good, lw, ls, lr):
    """The float64 maximum of the log joint over one utterance by the textbook DP (no normalisation, no ids)."""
    lw, ls, lr = (np.asarray(a, dtype=np.float64) for a in (lw, ls, lr))
    V = None
    for t in range(s64.shape[0]):
        if not good[t]:
            continue
        V = s64[t] + lw if V is None else s64[t] + np.maximum(V + ls, V.max() + lr)
    return 0.0 if V is None else float(V.max())


def J(s64, ids, good, lw, ls, lr):
    """The float64 log joint of a given path (ids at the good frames; the BAD frames are skipped)."""
    lw, ls, lr = (np.asarray(a, dtype=np.float64) for a in (lw, ls, lr))
    s64 = np.asarray(s64, dtype=np.float64)
    total, prev = 0.0, None
    for t in range(s64.shape[0]):
        if not good[t]:
            continue
        k = int(ids[t])
        total += s64[t, k] + (lw[k] if prev is None else ls[k] if k == prev else lr[k])
        prev = k
    return float(total)


def brute_force(logn, bad, w32, rho):
    """(the largest log joint, the list of all paths over the good frames attaining it) by enumeration of all K^n paths
    under a[j, k] = rho [j == k] + (1 - rho) w[k] taken directly in float64 (no log tables): tiny cases only."""
    logn = np.asarray(logn, dtype=np.float64)
    L, K = logn.shape
    w = np.asarray(w32, dtype=np.float32).astype(np.float64)
    r = float(np.float32(rho))
    omr = float(np.float32(1.0) - np.float32(rho))
    frames = [t for t in range(L) if not bad[t]]
    if not frames:
        return 0.0, [()]
    best, arg = -np.inf, []
    with np.errstate(divide='ignore'):
        for z in itertools.product(range(K), repeat=len(frames)):
            v = np.log(w[z[0]]) + logn[frames[0], z[0]]
            for i in range(1, len(frames)):
                v += np.log((r if z[i] == z[i - 1] else 0.0) + omr * w[z[i]]) + logn[frames[i], z[i]]
            if v > best:
                best, arg = v, [z]
            elif v == best:
                arg.append(z)
    return float(best), arg


def score_bound(scale, D):
    """The forward bound of an fp32 dot product of depth 2D + 1 (module docstring) from gmm_np.score_scale's sums."""
    return (2 * D + 3) * U * (1.0 + 2.0 ** -10) * np.asarray(scale, dtype=np.float64)


def table_max(lw, ls, lr):
    """The largest finite magnitude in the three tables."""
    a = np.abs(np.concatenate([np.asarray(t, dtype=np.float64).ravel() for t in (lw, ls, lr)]))
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else 0.0


def delta(E, smax, lmax):
    """The per-cell perturbation of the module docstring."""
    return float(np.max(E)) + U * (float(smax) + 4.0 * float(lmax))
