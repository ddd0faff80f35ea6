"""abnet3_amd/discovery.py restated by brute force (test infrastructure only): segments, segment vectors, float64
similarities, the overlap exclusion, top-k under (similarity descending, index ascending), the mutual filter and the
pair list -- plain loops and dense n x n arrays, written from the module's definition."""
import numpy as np


def delta(d):
    """An fp32 dot product of d terms of unit vectors is within gamma_d ~ d 2^-24 of the exact one whatever the order
    of summation; doubled for the rounding of the two normalisations (and 4 for the products' own roundings)."""
    return 2.0 * (d + 4) * 2.0 ** -24


def segments(n_frames, lengths=(40, 60, 80), shift=5):
    out = []
    for f, n in enumerate(n_frames):
        for L in lengths:
            s = 0
            while s + L <= n:
                out.append((f, s, L))
                s += shift
    return out


def gather(feats, segs, K=10):
    """[n, K D] float32: the frames t_j = s + ((2j + 1) L) // (2K) of every segment, not normalised.
    feats: one [T, D] array per file (in file-number order)."""
    rows = []
    for f, s, L in segs:
        rows.append(np.concatenate([feats[f][s + ((2 * j + 1) * L) // (2 * K)] for j in range(K)]))
    return np.asarray(rows, dtype=np.float32).reshape(len(segs), -1)


def unit64(g):
    g = np.asarray(g, dtype=np.float64)
    n = np.sqrt((g * g).sum(1))
    return g / np.where(n > 0, n, 1.0)[:, None], n > 0


def excluded(q_meta, c_meta):
    """[nq, nc] bool: same file and intersecting half-open intervals."""
    q, c = np.asarray(q_meta), np.asarray(c_meta)
    return (q[:, None, 0] == c[None, :, 0]) & (q[:, None, 1] < c[None, :, 2]) & (c[None, :, 1] < q[:, None, 2])


def topk(S, k, excl=None):
    """idx [nq, k] (-1 for unused), sim [nq, k] (-inf) of float64 similarities S by (sim descending, j ascending)."""
    nq, nc = S.shape
    idx = np.full((nq, k), -1, dtype=np.int64)
    sim = np.full((nq, k), -np.inf)
    for i in range(nq):
        cand = [j for j in range(nc) if excl is None or not excl[i, j]]
        cand.sort(key=lambda j: (-S[i, j], j))
        for p, j in enumerate(cand[:k]):
            idx[i, p], sim[i, p] = j, S[i, j]
    return idx, sim


def pairs_from_lists(idx, sim, min_similarity=0.0, mutual=True, max_pairs=None):
    lists = [{int(j): float(s) for j, s in zip(ri, rs) if j >= 0} for ri, rs in zip(idx, sim)]
    out = []
    for a in range(len(lists)):
        for b in range(a + 1, len(lists)):
            ab, ba = b in lists[a], a in lists[b]
            if (ab and ba) if mutual else (ab or ba):
                s = lists[a][b] if ab else lists[b][a]
                if s >= min_similarity:
                    out.append((a, b, s))
    out.sort(key=lambda t: (-t[2], t[0], t[1]))
    return out[:max_pairs] if max_pairs is not None else out


def check_topk(idx, sim, S, k, excl, dlt, min_exact=0.9):
    """The parity check of abn_knn_topk against float64 similarities S (excl: [nq, nc] bool or None).
    Asserts the float64-side condition first (>= min_exact of the queries have no other candidate within dlt of their
    k-th best), then the kernel's lists; returns the number of exact-kind queries."""
    nq, nc = S.shape
    adm = np.ones_like(S, dtype=bool) if excl is None else ~excl
    # float64 side, before the GPU result is looked at
    exact, taus = np.zeros(nq, dtype=bool), np.full(nq, -np.inf)
    sets = []
    for i in range(nq):
        js = np.flatnonzero(adm[i])
        order = js[np.lexsort((js, -S[i, js]))]
        top = order[:k]
        sets.append(set(top.tolist()))
        if len(order) <= k:
            exact[i] = True                      # every admissible candidate is returned: no cut to sit near
            continue
        taus[i] = S[i, top[-1]]
        near = np.abs(S[i, order] - taus[i]) <= dlt
        exact[i] = near.sum() == 1
    assert exact.mean() >= min_exact, 'only %.1f %% of the queries are free of near ties' % (100 * exact.mean())
    idx, sim = np.asarray(idx), np.asarray(sim)
    assert idx.shape == (nq, k) and sim.shape == (nq, k)
    for i in range(nq):
        n_adm = int(adm[i].sum())
        n_ret = min(k, n_adm)
        got = idx[i, :n_ret]
        assert (got >= 0).all() and (got < nc).all(), (i, got)
        assert (idx[i, n_ret:] == -1).all() and np.isneginf(sim[i, n_ret:]).all(), (i, idx[i], sim[i])
        assert len(set(got.tolist())) == n_ret, (i, got)
        assert adm[i, got].all(), ('excluded candidate returned', i, got)
        assert np.abs(sim[i, :n_ret].astype(np.float64) - S[i, got]).max(initial=0.0) <= dlt, (i, sim[i], S[i, got])
        s_ret = sim[i, :n_ret]
        assert (s_ret[:-1] >= s_ret[1:]).all(), ('not sorted', i, s_ret)
        ties = s_ret[:-1] == s_ret[1:]
        assert (got[:-1][ties] < got[1:][ties]).all(), ('ties not by ascending j', i, got, s_ret)
        if n_adm > k:
            assert (S[i, got] >= taus[i] - dlt).all(), (i, S[i, got], taus[i])
            must = np.flatnonzero(adm[i] & (S[i] > taus[i] + dlt))
            assert set(must.tolist()) <= set(got.tolist()), (i, must, got)
        if exact[i]:
            assert set(got.tolist()) == sets[i], (i, sorted(got.tolist()), sorted(sets[i]))
    return int(exact.sum())
