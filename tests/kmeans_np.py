"""abnet3_amd/kmeans.py's definition restated in float64 numpy: the reference the k-means tests compare the kernels with.

Everything here takes the fp32-ROUNDED inputs of the kernels -- the centred frames xc, the tables m and b -- and
evaluates scores, argmax (lowest k on ties), statistics, update and inertia in float64.  `allowance` is the per-row
error an fp32 evaluation of the score may have, in any summation order."""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    """The standard forward bound of an fp32 sum of n terms (or a dot product of depth n) in any order."""
    return n * U / (1.0 - n * U)


def prepare(x, metric='euclidean'):
    """(xc float32 [T, D], bad bool [T], shift float32 [D]) of a raw float32 table, as the module forms them."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all='ignore'):
        if metric == 'cosine':
            shift = np.zeros(x.shape[1], dtype=np.float32)
            xc = (x / np.sqrt((x * x).sum(axis=1, keepdims=True, dtype=np.float32))).astype(np.float32)
        else:
            fin = np.isfinite(x).all(axis=1)
            shift = x[fin].astype(np.float64).mean(axis=0).astype(np.float32)
            xc = (x - shift).astype(np.float32)
        bad = ~np.isfinite(xc * xc).all(axis=1)
    return xc, bad, shift


def tables(mu, metric='euclidean'):
    """(m float32 [K, D], b float32 [K]) of float64 centred centroids: m rounded once, b from the rounded m."""
    m = np.asarray(mu, dtype=np.float64).astype(np.float32)
    if metric == 'cosine':
        return m, np.zeros(m.shape[0], dtype=np.float32)
    return m, (-0.5 * (m.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)


def scores(xc, bad, m, b):
    """s [T, K] float64 (rows of BAD frames: 0) and the allowance E [T] = gamma(D + 1) max_k (sum_d |xc m| + |b|)."""
    x64 = np.where(bad[:, None], 0.0, xc.astype(np.float64))
    m64, b64 = m.astype(np.float64), b.astype(np.float64)
    s = x64 @ m64.T + b64[None, :]
    E = gamma(xc.shape[1] + 1) * (np.abs(x64) @ np.abs(m64).T + np.abs(b64)[None, :]).max(axis=1)
    return s, E


def assign(xc, bad, m, b):
    """(ids int32 [T], s, E): argmax over k, the lowest k on equal scores, -1 for a BAD frame."""
    s, E = scores(xc, bad, m, b)
    ids = np.argmax(s, axis=1).astype(np.int32)        # (numpy's argmax returns the first maximum)
    ids[bad] = -1
    return ids, s, E


def statistics(xc, ids, m, K):
    """(N [K], S [K, D], d2 [T]) in float64 for the given ids: counts, sums of xc, and the frames' distortions
    sum_d (xc - m[id])^2 (0 for id = -1)."""
    x64, m64 = xc.astype(np.float64), m.astype(np.float64)
    good = ids >= 0
    N = np.bincount(ids[good], minlength=K).astype(np.float64)
    S = np.zeros((K, xc.shape[1]))
    np.add.at(S, ids[good], x64[good])
    d2 = np.zeros(len(ids))
    d2[good] = ((x64[good] - m64[ids[good]]) ** 2).sum(axis=1)
    return N, S, d2


def sum_bound(xc, ids, K):
    """[K, D]: gamma(N[k]) sum_{t: ids[t] = k} |xc[t, d]|, what an fp32 sum of a cluster's rows may be off by."""
    good = ids >= 0
    N = np.bincount(ids[good], minlength=K).astype(np.float64)
    A = np.zeros((K, xc.shape[1]))
    np.add.at(A, ids[good], np.abs(xc[good].astype(np.float64)))
    return gamma(N)[:, None] * A


def update(N, S, mu_prev, metric='euclidean'):
    """(mu [K, D] float64, number of empty clusters): S / N, an empty cluster keeps its centroid; the cosine metric
    renormalises each new mean to unit length."""
    mu = np.array(mu_prev, dtype=np.float64)
    live = N > 0
    new = S[live] / N[live][:, None]
    if metric == 'cosine':
        nrm = np.sqrt((new * new).sum(axis=1, keepdims=True))
        new = np.where(nrm > 0, new / np.where(nrm > 0, nrm, 1.0), mu[live])
    mu[live] = new
    return mu, int((~live).sum())


def inertia(d2, ids):
    return d2.sum() / max(1, int((ids >= 0).sum()))


def iteration(xc, bad, mu, metric='euclidean'):
    """One Lloyd iteration: (ids, inertia, new mu, empty count)."""
    m, b = tables(mu, metric)
    ids, _, _ = assign(xc, bad, m, b)
    N, S, d2 = statistics(xc, ids, m, len(mu))
    mu2, empty = update(N, S, mu, metric)
    return ids, inertia(d2, ids), mu2, empty
