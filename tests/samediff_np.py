"""abnet3_amd/samediff.py restated with explicit loops and exact fractions (test infrastructure only).

The definition, restated:

* Tokens are sorted by word type, so type c occupies a contiguous index range; row i carries cbeg[i], cend[i] (its
  type's range, half open) and optionally spk[i].
* Pool: all pairs i < j whose similarity is finite.  A pair is positive when j lies in [cbeg[i], cend[i]).
  condition 'all': every same-type pair is a positive, nothing is left out; 'swdp': positives are same word,
  different speaker, same-word same-speaker pairs are left out of the pool; 'swsp': positives are same word, same
  speaker, same-word different-speaker pairs are left out.  Different-word pairs are always in the pool.
* Thresholds v_0 >= ... >= v_{P-1}: the positives' similarities, sorted, NaN removed.
* Bucket of a pool pair of similarity x: b(x) = #{r : v_r > x} in [0, P]; hist[b] counts the pool pairs per bucket,
  positives included.
* A tie group g of equal thresholds, first index f_g, last index + 1 = l_g: A_g = sum_{b <= f_g} hist[b] pool pairs are
  at least that similar, l_g of them positives.  P_g = l_g / A_g, R_g = l_g / P.
* AP = sum_g (l_g - f_g) / P * P_g;  PRB = P_g at the group minimising |P_g - R_g|, the first on a tie;  P = 0: nan.
* For a distance the order is reversed: v ascending, b(x) = #{r : v_r < x}.
"""
import math
from fractions import Fraction

import numpy as np


def buckets_hist(sims, i, j, cbeg, cend, spk=None, condition='all', distance=False):
    """(thr, hist, n_bad) from the similarities (distances with distance=True) `sims` of the pairs (i[p], j[p])."""
    pool, positives, n_bad = [], [], 0
    for x, a, b in zip(np.asarray(sims).tolist(), np.asarray(i).tolist(), np.asarray(j).tolist()):
        assert a < b
        same = cbeg[a] <= b < cend[a]
        if same and condition != 'all':
            same_spk = spk[a] == spk[b]
            if (condition == 'swdp' and same_spk) or (condition == 'swsp' and not same_spk):
                continue
        if not math.isfinite(x):
            n_bad += 1
            continue
        pool.append(x)
        if same:
            positives.append(x)
    thr = np.array(sorted(positives, reverse=not distance), dtype=np.asarray(sims).dtype)
    hist = [0] * (len(thr) + 1)
    for x in pool:
        hist[int((thr < x).sum() if distance else (thr > x).sum())] += 1
    return thr, hist, n_bad


def groups(thr):
    """[(f, l)] of the tie groups of the sorted thresholds."""
    out, f = [], 0
    for r in range(1, len(thr) + 1):
        if r == len(thr) or thr[r] != thr[f]:
            out.append((f, r))
            f = r
    return out


def _from_groups(stats, P):
    """(ap, prb) from [(positives in the group, positives so far, pool pairs so far)] in exact fractions."""
    if P == 0:
        return float('nan'), float('nan')
    ap, best, prb = Fraction(0), None, None
    for k, l, A in stats:
        prec, rec = Fraction(l, A), Fraction(l, P)
        ap += Fraction(k, P) * prec
        if best is None or abs(prec - rec) < best:
            best, prb = abs(prec - rec), prec
    return float(ap), float(prb)


def scores(thr, hist):
    """(ap, prb) of the definition."""
    return _from_groups([(l - f, l, sum(hist[:f + 1])) for f, l in groups(thr)], len(thr))


def brute_ap(sim, is_pos, distance=False):
    """(ap, prb) by sorting the whole pool (finite similarities `sim`, their labels `is_pos`) and walking it group by
    group of equal similarity: a group with positives contributes its share of the positives times the precision
    once the whole group is in."""
    order = sorted(range(len(sim)), key=lambda p: sim[p], reverse=not distance)
    P = int(sum(bool(b) for b in is_pos))
    stats, seen, tp, a = [], 0, 0, 0
    while a < len(order):
        b = a
        while b < len(order) and sim[order[b]] == sim[order[a]]:
            b += 1
        k = sum(1 for p in order[a:b] if is_pos[p])
        seen, tp = seen + (b - a), tp + k
        if k:
            stats.append((k, tp, seen))
        a = b
    return _from_groups(stats, P)
