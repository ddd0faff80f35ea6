"""The mixture of abnet3_amd/gmm.py restated in numpy (test infrastructure only).

Every function takes a `dtype`: float64 is the reference, float32 the yardstick -- the same formulas with every
product and sum rounded to fp32 in numpy's order, which is neither the kernel's order nor a bound on it; its own
error against float64, scaled by the sum of the absolute values of the terms, is what the kernel's is compared with.
Both start from the same fp32 xc, A, B, c."""
import numpy as np


def centre(x, shift):
    """xc = float32(x - shift) and the BAD rows (a non-finite xc^2)."""
    with np.errstate(all='ignore'):
        xc = (np.asarray(x, dtype=np.float32) - np.asarray(shift, dtype=np.float32)).astype(np.float32)
        bad = ~np.isfinite(xc * xc).all(axis=1)
    return xc, bad


def moments(x):
    """(shift float32 [D], gv float64 [D]) of a training table: the mean of the frames without a non-finite value,
    and the variance of xc over the good frames."""
    x = np.asarray(x, dtype=np.float32)
    fin = np.isfinite(x).all(axis=1)
    shift = x[fin].astype(np.float64).mean(axis=0).astype(np.float32)
    xc, bad = centre(x, shift)
    x64 = xc[~bad].astype(np.float64)
    return shift, (x64 * x64).mean(axis=0) - x64.mean(axis=0) ** 2


def tables(w, m, v):
    """(A, B, c) float32 from float64 weights, centred means and variances."""
    w, m, v = (np.asarray(a, dtype=np.float64) for a in (w, m, v))
    with np.errstate(divide='ignore'):
        c = np.log(w) - 0.5 * (np.log(2.0 * np.pi * v) + m * m / v).sum(axis=1)
    return (m / v).astype(np.float32), (-0.5 / v).astype(np.float32), c.astype(np.float32)


def augment(xc, bad, dtype):
    """[xc | xc^2 | 1] in `dtype` (float32: the square is rounded to fp32, as on the device); BAD rows are zero."""
    xc = np.where(bad[:, None], np.float32(0), xc).astype(dtype)
    return np.concatenate([xc, xc * xc, np.ones((xc.shape[0], 1), dtype=dtype)], axis=1)


def weights_matrix(A, B, c, dtype):
    return np.concatenate([A, B, c[:, None]], axis=1).astype(dtype)


def scores(xc, bad, A, B, c, dtype=np.float64):
    return augment(xc, bad, dtype) @ weights_matrix(A, B, c, dtype).T


def score_scale(xc, bad, A, B, c):
    """sum_d |xc A| + xc^2 |B| + |c| per (frame, component), float64."""
    return np.abs(augment(xc, bad, np.float64)) @ np.abs(weights_matrix(A, B, c, np.float64)).T


def lse_post(s, bad):
    """(lse [T], g [T, K]) in s's dtype; BAD rows: NaN and zeros."""
    with np.errstate(all='ignore'):
        mx = s.max(axis=1, keepdims=True)
        e = np.exp(s - mx)
        lse = (mx[:, 0] + np.log(e.sum(axis=1, dtype=s.dtype))).astype(s.dtype)
        g = np.exp(s - lse[:, None]).astype(s.dtype)
    lse[bad] = np.nan
    g[bad] = 0
    return lse, g


def statistics(g, xc, bad, dtype=np.float64):
    """(N [K], S1 [K, D], S2 [K, D]) in `dtype`."""
    aug = augment(xc, bad, dtype)
    D = xc.shape[1]
    S = g.astype(dtype).T @ aug
    return S[:, 2 * D], S[:, :D], S[:, D:2 * D]


def mstep(N, S1, S2, Tg, gv, m_prev, v_prev, var_floor=0.01, min_count=1.0):
    """(w, m, v, starved count), float64."""
    N, S1, S2 = (np.asarray(a, dtype=np.float64) for a in (N, S1, S2))
    keep = N < min_count
    with np.errstate(all='ignore'):
        m = S1 / N[:, None]
        v = np.maximum(S2 / N[:, None] - m * m, var_floor * np.asarray(gv, dtype=np.float64)[None, :])
    m = np.where(keep[:, None], m_prev, m)
    v = np.where(keep[:, None], v_prev, v)
    w = N / float(Tg)
    return w / w.sum(), m, v, int(keep.sum())


def initial(xc, bad, gv, K, seed=0):
    """(w, m, v) of the documented initialisation."""
    rows = np.flatnonzero(~bad)
    if len(rows) < K:
        raise ValueError('T < K')
    pick = np.sort(np.random.default_rng(seed).choice(len(rows), K, replace=False))
    return np.full(K, 1.0 / K), xc[rows[pick]].astype(np.float64), np.tile(np.asarray(gv, dtype=np.float64), (K, 1))


def em_iteration(xc, bad, w, m, v, gv, var_floor=0.01, min_count=1.0, dtype=np.float64):
    """One iteration: (mean log-likelihood under (w, m, v), then the M-step's w, m, v, starved)."""
    A, B, c = tables(w, m, v)
    lse, g = lse_post(scores(xc, bad, A, B, c, dtype), bad)
    Tg = int((~bad).sum())
    ll = float(lse[~bad].astype(np.float64).sum() / Tg)
    N, S1, S2 = statistics(g, xc, bad, dtype)
    return (ll,) + mstep(N, S1, S2, Tg, gv, m, v, var_floor, min_count)


def fit(x, K, n_iter=20, tol=1e-4, var_floor=0.01, min_count=1.0, seed=0, dtype=np.float64, shift=None, gv=None):
    """dict(w, m, v, shift, gv, log_likelihoods, starved); m is centred (mean - shift)."""
    if shift is None:
        shift, gv = moments(x)
    xc, bad = centre(x, shift)
    w, m, v = initial(xc, bad, gv, K, seed)
    lls, starved = [], 0
    for it in range(n_iter):
        ll, w, m, v, starved = em_iteration(xc, bad, w, m, v, gv, var_floor, min_count, dtype)
        lls.append(ll)
        if it > 0 and lls[-1] - lls[-2] < tol:
            break
    return dict(w=w, m=m, v=v, shift=shift, gv=gv, log_likelihoods=lls, starved=starved)
