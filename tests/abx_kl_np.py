"""Numpy restatement of the symmetrised Kullback-Leibler frame distance of the ABX evaluation (distance='kl' in
abnet3_amd/abx.py's module docstring): the tables, the cell as an explicit float32 loop over k, the float64 DTW
recurrence with its tie-break and the carried path length.  Triplets, cell scores and the error are tests/abx_np.py's.
Test infrastructure only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abx_np  # noqa: E402


def tables(x, floor=1e-6):
    """(P, L, bad): P = max(x, floor) in float32, L = float32(log(float64(P))), bad[r] = row r holds a non-finite or
    a negative value (the P / L contents of such a row are unspecified)."""
    x = np.asarray(x, dtype=np.float32)
    f = np.float32(floor)
    assert f > 0
    bad = (~np.isfinite(x) | (x < 0)).any(axis=1)
    with np.errstate(invalid='ignore'):
        P = np.where(x > f, x, f).astype(np.float32)
    L = np.log(P.astype(np.float64)).astype(np.float32)
    return P, L, bad


def frame_distances(P1, L1, P2, L2):
    """[n1, n2] float32: d = 0.5f * sum over ascending k of (P_p[k] - P_q[k]) * (L_p[k] - L_q[k]), the subtraction of
    the P's, that of the L's, the product and the addition each rounded to float32 (float32 arrays: numpy rounds every
    elementwise operation on its own and keeps subnormals)."""
    P1, L1, P2, L2 = (np.asarray(a, dtype=np.float32) for a in (P1, L1, P2, L2))
    acc = np.zeros((P1.shape[0], P2.shape[0]), dtype=np.float32)
    for k in range(P1.shape[1]):
        dp = P1[:, k, None] - P2[None, :, k]
        dl = L1[:, k, None] - L2[None, :, k]
        acc = acc + (dp * dl)
        assert acc.dtype == np.float32
    return np.float32(0.5) * acc


def dtw(d):
    """(total_cost float64, path_len) of the frame-distance matrix d: cost = d + min(diag, up, left) in float64, the
    first minimum in the order diag, up, left, the length carried along the chosen predecessor; the virtual cell
    (-1, -1) costs 0 and has length 0."""
    n, m = d.shape
    if n == 0 or m == 0:
        return 0.0, 0
    d = d.astype(np.float64)
    cost = np.full((n + 1, m + 1), np.inf)
    ln = np.zeros((n + 1, m + 1), dtype=np.int64)
    cost[0, 0] = 0.0
    for s in range(2, n + m + 1):                       # the cells of an anti-diagonal do not depend on each other
        i = np.arange(max(1, s - m), min(n, s - 1) + 1)
        j = s - i
        dg, up, left = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        take_up = up < dg                               # first minimum in the order diag, up, left
        b1 = np.where(take_up, up, dg)
        l1 = np.where(take_up, ln[i - 1, j], ln[i - 1, j - 1])
        take_left = left < b1
        cost[i, j] = d[i - 1, j - 1] + np.where(take_left, left, b1)
        ln[i, j] = np.where(take_left, ln[i, j - 1], l1) + 1
    return float(cost[n, m]), int(ln[n, m])


def dtw_cost_batch(t1, off1, n1, t2, off2, n2, cap=None):
    """(total_cost float64 [P], path_len int32 [P]) of the pair table over the tables t = (P, L, bad) of each side, with
    the kernel's rules: a pair outside the tables, with a negative length or a token 2 beyond `cap` is refused (-1),
    an empty token gives 0 / 0, a BAD row in either token drops the pair (0 / 0)."""
    (P1, L1, b1), (P2, L2, b2) = t1, t2
    cost = np.zeros(len(n1), dtype=np.float64)
    plen = np.zeros(len(n1), dtype=np.int32)
    for p in range(len(n1)):
        a, n, b, m = int(off1[p]), int(n1[p]), int(off2[p]), int(n2[p])
        if n < 0 or m < 0 or a < 0 or b < 0 or a + n > len(P1) or b + m > len(P2) or (cap is not None and m > cap):
            plen[p] = -1
            continue
        if n == 0 or m == 0 or b1[a:a + n].any() or b2[b:b + m].any():
            continue
        cost[p], plen[p] = dtw(frame_distances(P1[a:a + n], L1[a:a + n], P2[b:b + m], L2[b:b + m]))
    return cost, plen


def dtw_distance(ta, tb):
    """d(P, Q) = total_cost / path_len (float64) of two tokens given as (P, L) table slices."""
    c, n = dtw(frame_distances(ta[0], ta[1], tb[0], tb[1]))
    return np.float64(c) / np.float64(n)


def abx_error(items, tokens, mode):
    """The ABX error of `mode` with tokens[i] = (P, L) table slices of item i (abx_np's triplets, cells, error)."""
    trips = abx_np.triplets(items.phones, items.contexts, items.speakers, mode)
    d = {pq: dtw_distance(tokens[pq[0]], tokens[pq[1]]) for pq in abx_np.needed_pairs(trips)}
    return abx_np.error(abx_np.cell_scores(trips, d))
