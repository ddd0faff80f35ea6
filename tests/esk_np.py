"""abnet3_amd/eskmeans.py's definition restated with numpy and explicit loops: the reference the ES-KMeans tests compare
the kernels with.

The definition:

* Landmarks lm [n_lm] (rows of the table), utterance u owns lm[lm_off[u] .. lm_off[u + 1]).  Candidate (g, s), 1 <= s <= S,
  runs from landmark g to g + s inside one utterance: rows lm[g] .. lm[g + s] - 1, n = lm[g + s] - lm[g], index g S + s - 1,
  allowed if s == 1 or n <= max_frames.
* Vector (abn_segment_vectors' rule): the `frames` rows row0 + ((2 j + 1) n) // (2 frames), concatenated; the sum of
  squares in float64 with element e added to partial e mod 64 in order of e and the 64 partials folded 32, 16, .. 1
  (p[l] + p[l + o]); inv = fp32(1 / sqrt(ss)) (0 where ss is not > 0); v = fp32(x * inv).  float64 products of fp32
  values are exact, so this is the kernels' value to the bit.  keep = ss > 0.
* Score: s[c, k] = <v_c, m_k> + b_k in float64 over the fp32 operands (tests/kmeans_np.py's `scores`, with its
  allowance E at depth frames D + 1); best = max_k, id = the lowest k attaining it; -1 / NaN for a candidate that
  crosses an utterance, is not allowed, is all zero or has a non-finite sampled value.
* Cost: c = fp32(n) * (1 - 2 best): the product 2 best is exact, the subtraction and the last product round once each in
  fp32; +inf where id = -1.
* DP per utterance with L = landmarks - 1, fp32: gamma[0] = 0, gamma[j] = min_s fl(gamma[j - s] + c(j - s, s)), s
  ascending with a strict <, so equal sums go to the smallest s.  Traceback from L: cut at every chosen boundary (first
  and last included), word / span at every chosen start, -1 elsewhere; objective = gamma[L]; n_seg.  gamma[L] = +inf:
  objective NaN, n_seg -1, nothing marked.

The allowance of the float comparison (`dp_bound`).  Let best64 be the float64 best score of the fp32 operands,
c64 = n (1 - 2 best64), and J64(z) the sum of c64 over a segmentation z in float64.  The kernel's DP is exact dynamic
programming for a problem whose segment costs are c' = c64 + e:
  * |fp32 score - s64| <= E for every k (kmeans_np.scores' allowance: a dot product of depth frames D + 1 in any order),
    so |best32 - best64| <= E whichever k attains either maximum;
  * n < 2^24 and 2 best are exact; fl(1 - 2 best32) and the product round once each: |c32 - n (1 - 2 best32)| <=
    (2 u + u^2) n |1 - 2 best32| <= 3 u n (|1 - 2 best64| + 2 E), u = 2^-24.  Together
    |c32 - c64| <= n (2 E + 3 u (|1 - 2 best64| + 2 E)) =: d_c;
  * each step rounds the addition gamma[j - s] + c once: at most u |gamma[j]|.  A partial path has at most L segments of
    at most cmax = max (|c64| + d_c) each, so |gamma| <= L cmax (1 + u)^L, and the rounding can be charged to the
    segment that ends at j: at most 2 u L cmax for L < 2^20.
  So |e| <= delta = max d_c + 2 u L cmax per segment, and a segmentation has at most L segments: |J'(z) - J64(z)| <= L delta
  for every z.  The device path z* minimises J', the float64 path z64 minimises J64:
      J64(z64) <= J64(z*) <= J'(z*) + L delta <= J'(z64) + L delta <= J64(z64) + 2 L delta,
  and the device objective is J'(z*): within L delta of J64(z*), within 2 L delta of the float64 optimum J64(z64) too.
"""
import itertools

import numpy as np

import kmeans_np

U = 2.0 ** -24


def utterance_of(g, lm_off):
    """The utterance that owns landmark g."""
    return int(np.searchsorted(np.asarray(lm_off), g, side='right') - 1)


def candidates(lm, lm_off, S, max_frames=None, T=None):
    """(row0 int64 [n_lm S], n int64 [n_lm S]) with n = 0 for a candidate that crosses an utterance or is not allowed."""
    lm, lm_off = np.asarray(lm, dtype=np.int64), np.asarray(lm_off, dtype=np.int64)
    row0 = np.zeros(len(lm) * S, dtype=np.int64)
    n = np.zeros(len(lm) * S, dtype=np.int64)
    for u in range(len(lm_off) - 1):
        for g in range(int(lm_off[u]), int(lm_off[u + 1])):
            for s in range(1, S + 1):
                if g + s >= lm_off[u + 1]:
                    continue
                length = int(lm[g + s] - lm[g])
                if s == 1 or max_frames is None or length <= max_frames:
                    row0[g * S + s - 1], n[g * S + s - 1] = lm[g], length
    return row0, n


def sum_of_squares(x):
    """The float64 sum of squares of a row of fp32 values in the kernels' order (module docstring)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    p = np.zeros(64, dtype=np.float64)
    for e0 in range(0, len(x), 64):
        chunk = x[e0:e0 + 64]
        p[:len(chunk)] += chunk * chunk
    o = 32
    while o:
        p = p[:o] + p[o:2 * o]
        o >>= 1
    return float(p[0])


def vector(table, row0, n, frames):
    """(v float32 [frames D], keep bool, bad bool): the segment's unit vector; bad: all zero, or a non-finite value in
    it (the kernels' BAD rule: v^2 not finite)."""
    rows = [int(row0 + ((2 * j + 1) * n) // (2 * frames)) for j in range(frames)]
    x = np.asarray(table, dtype=np.float32)[rows].ravel()
    with np.errstate(all='ignore'):
        ss = sum_of_squares(x)
        inv = np.float32(1.0 / np.sqrt(ss)) if ss > 0.0 else np.float32(0.0)
        v = (x * inv).astype(np.float32)
        bad = not (ss > 0.0) or not np.isfinite(v * v).all()
    return v, bool(ss > 0.0), bool(bad)


def vectors(table, row0, n, frames):
    """(V float32 [C, frames D], bad bool [C]) of candidate arrays (n = 0: a zero row, bad)."""
    D = np.asarray(table).shape[1]
    V = np.zeros((len(n), frames * D), dtype=np.float32)
    bad = np.ones(len(n), dtype=bool)
    for c in range(len(n)):
        if n[c] > 0:
            V[c], _, bad[c] = vector(table, row0[c], n[c], frames)
    V[bad] = 0.0
    return V, bad


def score(V, bad, m, b):
    """(best float64 [C], id int32 [C], gap [C], E [C]): the float64 best score, the lowest index attaining it (-1 / NaN
    where bad), the float64 distance to the second best (inf for K = 1) and the fp32 allowance of a score."""
    s, E = kmeans_np.scores(V, bad, np.asarray(m, dtype=np.float32), np.asarray(b, dtype=np.float32))
    ids = np.argmax(s, axis=1).astype(np.int32)
    best = s[np.arange(len(ids)), ids]
    if s.shape[1] > 1:
        rest = s.copy()
        rest[np.arange(len(ids)), ids] = -np.inf
        gap = best - rest.max(axis=1)
    else:
        gap = np.full(len(ids), np.inf)
    best = np.where(bad, np.nan, best)
    ids[bad] = -1
    return best, ids, gap, E


def cost32(n, best, ids):
    """The fp32 cost of the module docstring for arrays (or scalars)."""
    with np.errstate(all='ignore'):
        c = np.float32(n) * (np.float32(1.0) - np.float32(2.0) * np.asarray(best, dtype=np.float32))
    return np.where(np.asarray(ids) < 0, np.float32(np.inf), c).astype(np.float32)


def dp_one(c, L, S):
    """One utterance: c [L, S] float32 with c[g, s - 1] the cost of the segment from g to g + s (+inf: blocked; entries
    with g + s > L are not read).  Returns (span int32 [L + 1] at the chosen starts / -1, objective, n_seg), or
    (all -1, nan, -1) when L cannot be reached."""
    gamma = [np.float32(0.0)] + [np.float32(np.inf)] * L
    back = [0] * (L + 1)
    for j in range(1, L + 1):
        for s in range(1, S + 1):
            if j - s < 0:
                break
            with np.errstate(all='ignore'):
                v = np.float32(gamma[j - s] + np.float32(c[j - s, s - 1]))
            if v < gamma[j]:
                gamma[j], back[j] = v, s
    span = np.full(L + 1, -1, dtype=np.int32)
    if not gamma[L] < np.inf:
        return span, float('nan'), -1
    j, n_seg = L, 0
    while j > 0:
        s = back[j]
        j -= s
        span[j] = s
        n_seg += 1
    return span, float(gamma[L]), n_seg


def dp(cand_best, cand_id, lm, lm_off, S):
    """The corpus call: (cut uint8 [n_lm], word int32 [n_lm], span int32 [n_lm], objective float64 [n_utt], n_seg int32
    [n_utt]) as abn_esk_segment writes them."""
    lm, lm_off = np.asarray(lm, dtype=np.int64), np.asarray(lm_off, dtype=np.int64)
    n_lm, n_utt = len(lm), len(lm_off) - 1
    cut, word, span = np.zeros(n_lm, dtype=np.uint8), np.full(n_lm, -1, dtype=np.int32), np.full(n_lm, -1, dtype=np.int32)
    obj, n_seg = np.zeros(n_utt, dtype=np.float64), np.zeros(n_utt, dtype=np.int32)
    for u in range(n_utt):
        lo, hi = int(lm_off[u]), int(lm_off[u + 1])
        L = hi - lo - 1
        c = np.full((L, S), np.inf, dtype=np.float32)
        for g in range(L):
            for s in range(1, min(S, L - g) + 1):
                at = (lo + g) * S + s - 1
                c[g, s - 1] = cost32(lm[lo + g + s] - lm[lo + g], cand_best[at], cand_id[at])
        sp, obj[u], n_seg[u] = dp_one(c, L, S)
        if n_seg[u] < 0:
            continue
        span[lo:hi] = sp
        starts = lo + np.flatnonzero(sp >= 1)
        word[starts] = np.asarray(cand_id)[starts * S + sp[sp >= 1] - 1]
        cut[starts] = 1
        cut[hi - 1] = 1
    return cut, word, span, obj, n_seg


def brute_force(c, L, S):
    """(best total, spans of the optimal segmentation the tie rule picks) over all 2^(L - 1) segmentations, totals in
    float64 (exact on half-integer grids); (nan, None) when every segmentation is blocked.  The tie rule: among the
    optimal ones the smallest last span, then the smallest span before it, and so on."""
    best, arg = np.inf, None
    for bits in itertools.product((0, 1), repeat=L - 1):
        bounds = [0] + [j + 1 for j in range(L - 1) if bits[j]] + [L]
        spans = [b - a for a, b in zip(bounds[:-1], bounds[1:])]
        if max(spans) > S:
            continue
        total = sum(float(c[a, s - 1]) for a, s in zip(bounds[:-1], spans))
        if not total < np.inf:
            continue
        key = tuple(reversed(spans))
        if total < best or (total == best and key < tuple(reversed(arg))):
            best, arg = total, spans
    return (float('nan'), None) if arg is None else (best, arg)


def optimum_f64(c64, L, S):
    """The float64 optimum of one utterance by the textbook DP: c64 [L, S] float64 (+inf: blocked)."""
    gamma = np.full(L + 1, np.inf)
    gamma[0] = 0.0
    for j in range(1, L + 1):
        for s in range(1, min(S, j) + 1):
            gamma[j] = min(gamma[j], gamma[j - s] + c64[j - s, s - 1])
    return float(gamma[L])


def dp_bound(n, best64, E, L):
    """2 L delta of the module docstring for one utterance: n, best64, E over its allowed candidates."""
    n, best64, E = (np.asarray(a, dtype=np.float64) for a in (n, best64, E))
    d_c = n * (2.0 * E + 3.0 * U * (np.abs(1.0 - 2.0 * best64) + 2.0 * E))
    cmax = float((np.abs(n * (1.0 - 2.0 * best64)) + d_c).max())
    return 2.0 * L * (float(d_c.max()) + 2.0 * U * L * cmax)
