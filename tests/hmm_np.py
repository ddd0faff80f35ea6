"""The sticky HMM of abnet3_amd/hmm.py restated in numpy with explicit loops (test infrastructure only).

States: the K components of a mixture with weights w; initial distribution w; transitions
a[j, k] = rho [j == k] + (1 - rho) w[k]; emissions logN[t, k].  A BAD frame is passed over: its row is zero, its
predecessor is its successor's predecessor, it counts neither as a frame nor as a transition.

`dtype` float64 is the reference; float32 is the yardstick: the same formulas with every product and sum rounded to
fp32 in this file's order, which is not the kernel's (gmm_np.py's convention).  Both start from the same float32 w and
rho (1 - rho is taken in float32) and the same logN."""
import itertools

import numpy as np


def emission_offsets(m, v):
    """c0 [K] float32: gmm_np.tables' c without log w."""
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return (-0.5 * (np.log(2.0 * np.pi * v) + m * m / v).sum(axis=1)).astype(np.float32)


def forward_backward(logn, bad, w32, rho, dtype=np.float64, smooth=True):
    """One utterance.  logn [L, K], bad [L] bool, w32 [K] float32, rho: a float32 value.
    dict(gamma [L, K], ahat [L, K], c [L], m [L], loglik (float64), stays (float64), n_good)."""
    dt = np.dtype(dtype).type
    logn = np.asarray(logn).astype(dtype)
    L, K = logn.shape
    w32 = np.asarray(w32, dtype=np.float32)
    w = w32.astype(dtype)
    rho32 = np.float32(rho)
    r, omr = dt(rho32), dt(np.float32(1.0) - rho32)
    live = w32 > 0
    bt = np.zeros((L, K), dtype=dtype)
    ahat = np.zeros((L, K), dtype=dtype)
    gamma = np.zeros((L, K), dtype=dtype)
    c = np.zeros(L, dtype=dtype)
    m = np.zeros(L, dtype=dtype)
    good = [t for t in range(L) if not bad[t]]
    loglik = 0.0
    prev = None
    with np.errstate(all='ignore'):
        for t in good:
            mt = dt(-np.inf)
            for k in range(K):
                if live[k] and logn[t, k] > mt:
                    mt = logn[t, k]
            m[t] = mt
            s = dt(0)
            u = np.zeros(K, dtype=dtype)
            for k in range(K):
                bt[t, k] = np.exp(dt(logn[t, k] - mt)) if live[k] else dt(0)    # (the kernel's rule: no inf x 0 at a far emission)
                pred = w[k] if prev is None else dt(dt(r * ahat[prev, k]) + dt(omr * w[k]))
                u[k] = dt(bt[t, k] * pred)
                s = dt(s + u[k])
            c[t] = s
            for k in range(K):
                ahat[t, k] = dt(u[k] / s)
            loglik += float(np.log(np.float64(s))) + float(mt)
            prev = t
        stays = 0.0
        if smooth:
            bhat = np.ones(K, dtype=dtype)
            for i in range(len(good) - 1, -1, -1):
                t = good[i]
                for k in range(K):
                    gamma[t, k] = dt(ahat[t, k] * bhat[k])
                if i == 0:
                    break
                p = good[i - 1]
                e = np.zeros(K, dtype=dtype)
                sw = dt(0)
                for k in range(K):
                    e[k] = dt(dt(bt[t, k] * bhat[k]) / c[t])
                    stays += float(r) * float(ahat[p, k]) * float(e[k])
                    sw = dt(sw + dt(w[k] * e[k]))
                for k in range(K):
                    bhat[k] = dt(dt(r * e[k]) + dt(omr * sw))
    return dict(gamma=gamma if smooth else ahat, ahat=ahat, c=c, m=m, loglik=loglik, stays=stays, n_good=len(good))


def brute_force(logn, bad, w32, rho):
    """The same quantities by enumeration of all K^n paths over the good frames, float64: (gamma, loglik, stays)."""
    logn = np.asarray(logn, dtype=np.float64)
    L, K = logn.shape
    w = np.asarray(w32, dtype=np.float32).astype(np.float64)
    r = float(np.float32(rho))
    omr = float(np.float32(1.0) - np.float32(rho))
    good = [t for t in range(L) if not bad[t]]
    gamma = np.zeros((L, K))
    if not good:
        return gamma, 0.0, 0.0
    shift = sum(logn[t][w > 0].max() for t in good)
    b = {t: np.exp(logn[t] - logn[t][w > 0].max()) for t in good}
    total, stays = 0.0, 0.0
    for z in itertools.product(range(K), repeat=len(good)):
        p = w[z[0]] * b[good[0]][z[0]]
        st = 0.0
        for i in range(1, len(good)):
            same = z[i] == z[i - 1]
            a = (r if same else 0.0) + omr * w[z[i]]
            p *= a * b[good[i]][z[i]]
            if same and a > 0:
                st += r / a                                   # the share of "stayed" in the transition j -> j
        total += p
        stays += p * st
        for i, t in enumerate(good):
            gamma[t, z[i]] += p
    return gamma / total, float(np.log(total) + shift), stays / total


def corpus(logn, bad, off, lens, w32, rho, dtype=np.float64, smooth=True):
    """Every utterance of a table: dict(post [T, K], loglik [n], stays [n], n_good [n], ahat [T, K], c [T], m [T])."""
    T, K = np.asarray(logn).shape
    post, ahat = np.zeros((T, K), dtype=dtype), np.zeros((T, K), dtype=dtype)
    c, m = np.zeros(T, dtype=dtype), np.zeros(T, dtype=dtype)
    ll, st, ng = [], [], []
    for o, n in zip(off, lens):
        r = forward_backward(logn[o:o + n], bad[o:o + n], w32, rho, dtype, smooth)
        post[o:o + n], ahat[o:o + n], c[o:o + n], m[o:o + n] = r['gamma'], r['ahat'], r['c'], r['m']
        ll.append(r['loglik'])
        st.append(r['stays'])
        ng.append(r['n_good'])
    return dict(post=post, ahat=ahat, c=c, m=m, loglik=np.array(ll), stays=np.array(st), n_good=np.array(ng, dtype=np.int64))


def forward_backward_fast(logn, bad, w32, rho, smooth=True, dtype=np.float64):
    """forward_backward with the loops over k vectorised (the sums over k then run in numpy's pairwise order; the
    large shapes of the GPU tests and the EM tests use it): (loglik, stays, n_good, gamma, ahat [L, K], m [L])."""
    dt = np.dtype(dtype).type
    logn = np.asarray(logn).astype(dtype)
    w32 = np.asarray(w32, dtype=np.float32)
    w = w32.astype(dtype)
    rho32 = np.float32(rho)
    r, omr = dt(rho32), dt(np.float32(1.0) - rho32)
    good = np.flatnonzero(~np.asarray(bad))
    L, K = logn.shape
    gamma, ahat_all, m_all = np.zeros((L, K), dtype=dtype), np.zeros((L, K), dtype=dtype), np.zeros(L, dtype=dtype)
    if not len(good):
        return 0.0, 0.0, 0, gamma, ahat_all, m_all
    with np.errstate(all='ignore'):
        lg = logn[good]
        m = np.where(w32 > 0, lg, dt(-np.inf)).max(axis=1)
        bt = np.where(w32 > 0, np.exp(lg - m[:, None]), dt(0))    # (0 at weight 0, as in the kernel: no inf x 0 at a far emission)
        n = len(good)
        ahat, c = np.zeros((n, K), dtype=dtype), np.zeros(n, dtype=dtype)
        for i in range(n):
            u = bt[i] * (w if i == 0 else r * ahat[i - 1] + omr * w)
            c[i] = u.sum(dtype=dtype)
            ahat[i] = u / c[i]
        ll = float((np.log(c.astype(np.float64)) + m.astype(np.float64)).sum())
        stays = 0.0
        ahat_all[good], m_all[good] = ahat, m
        if smooth:
            bhat = np.ones(K, dtype=dtype)
            for i in range(n - 1, -1, -1):
                gamma[good[i]] = ahat[i] * bhat
                if i == 0:
                    break
                e = bt[i] * bhat / c[i]
                stays += float(r) * float((ahat[i - 1].astype(np.float64) * e.astype(np.float64)).sum())
                bhat = r * e + omr * (w * e).sum(dtype=dtype)
        else:
            gamma[good] = ahat
    return ll, stays, n, gamma, ahat_all, m_all


def corpus_fast(logn, bad, off, lens, w32, rho, dtype=np.float64, smooth=True):
    """corpus() through forward_backward_fast: dict(post, ahat, m, loglik, stays, n_good)."""
    T, K = np.asarray(logn).shape
    post, ahat, m = np.zeros((T, K), dtype=dtype), np.zeros((T, K), dtype=dtype), np.zeros(T, dtype=dtype)
    ll, st, ng = [], [], []
    for o, n in zip(off, lens):
        r = forward_backward_fast(logn[o:o + n], bad[o:o + n], w32, rho, smooth, dtype)
        post[o:o + n], ahat[o:o + n], m[o:o + n] = r[3], r[4], r[5]
        ll.append(r[0])
        st.append(r[1])
        ng.append(r[2])
    return dict(post=post, ahat=ahat, m=m, loglik=np.array(ll), stays=np.array(st), n_good=np.array(ng, dtype=np.int64))


def em_stay(utterances, w32, rho0, n_iter=10):
    """EM on rho in float64 over [(logn, bad), ...]: (rhos [n_iter + 1], total log-likelihoods [n_iter])."""
    rhos, lls = [float(np.float32(rho0))], []
    for _ in range(n_iter):
        S = LL = 0.0
        trans = 0
        for logn, bad in utterances:
            ll, st, n = forward_backward_fast(logn, bad, w32, rhos[-1])[:3]
            S += st
            LL += ll
            trans += max(n - 1, 0)
        lls.append(LL)
        rhos.append(float(np.float32(min(max(S / trans, 0.0), 0.9999))))
    return rhos, lls


def planted(seed, K=4, D=3, n_utt=200, L=50, rho=0.9, scale=4.0):
    """The planted corpus of the EM tests: (x [n_utt L, D] float32, lens, w, means [K, D]); unit variances."""
    rng = np.random.default_rng(seed)
    w = np.array([0.4, 0.3, 0.2, 0.1])[:K]
    w = w / w.sum()
    mu = rng.normal(size=(K, D)) * scale
    rows = []
    for _ in range(n_utt):
        z = rng.choice(K, p=w)
        for t in range(L):
            if t > 0 and rng.random() > rho:
                z = rng.choice(K, p=w)
            rows.append(mu[z] + rng.normal(size=D))
    return np.asarray(rows, dtype=np.float32), np.full(n_utt, L, dtype=np.int64), w, mu
