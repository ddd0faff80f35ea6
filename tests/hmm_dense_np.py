"""The HMM with a full transition matrix of abnet3_amd/hmm.py restated in numpy (test infrastructure only).

States: the K components of a mixture; init [K]; trans [K][K] row-stochastic, trans[j][k] = P(k at t | j at the previous
good frame); emissions logN[t, k].  A BAD frame is passed over: its row is zero, its predecessor is its successor's
predecessor, it counts neither as a frame nor as a transition.

`dtype` float64 is the reference; float32 is the yardstick: the same formulas with every product and sum rounded to fp32
in this file's order, which is not the kernel's (gmm_np.py's convention).  Both start from the same float32 init and
trans and the same logN.  `forward_backward` has explicit loops over k and j; `forward_backward_fast` has them vectorised
(the sums over k then run in numpy's order) for the shapes of the GPU tests."""
import itertools

import numpy as np

TINY = 2.0 ** -100
TRANS_MIN = 2.0 ** -80


def sticky_matrix(w, stay):
    """(init, trans) float32 of the sticky model: trans[j][k] = r [j == k] + (1 - r) w32[k], formed in float64 from
    w32 = float32(w), r = float32(stay), 1 - r taken in float32, and rounded once."""
    w32 = np.asarray(w, dtype=np.float32)
    r = np.float32(stay)
    omr = np.float32(1.0) - r
    t = np.float64(omr) * w32.astype(np.float64)[None, :] + np.float64(r) * np.eye(len(w32))
    return w32.copy(), t.astype(np.float32)


def forward_backward(logn, bad, init, trans, dtype=np.float64, smooth=True):
    """One utterance, explicit loops.  logn [L, K], bad [L] bool, init [K] and trans [K, K] float32.
    dict(gamma [L, K], ahat [L, K], c [L], m [L], loglik (float64), G [K, K], xi [K, K], first [K] (float64), n_good)."""
    dt = np.dtype(dtype).type
    logn = np.asarray(logn).astype(dtype)
    L, K = logn.shape
    pi = np.asarray(init, dtype=np.float32).astype(dtype)
    a = np.asarray(trans, dtype=np.float32).astype(dtype)
    bt = np.zeros((L, K), dtype=dtype)
    ahat = np.zeros((L, K), dtype=dtype)
    gamma = np.zeros((L, K), dtype=dtype)
    c = np.zeros(L, dtype=dtype)
    m = np.zeros(L, dtype=dtype)
    G = np.zeros((K, K))
    first = np.zeros(K)
    good = [t for t in range(L) if not bad[t]]
    loglik = 0.0
    prev = None
    with np.errstate(all='ignore'):
        for t in good:
            mt = dt(-np.inf)
            for k in range(K):
                if logn[t, k] > mt:
                    mt = logn[t, k]
            m[t] = mt
            s = dt(0)
            u = np.zeros(K, dtype=dtype)
            for k in range(K):
                bt[t, k] = np.exp(dt(logn[t, k] - mt))
                if prev is None:
                    pred = pi[k]
                else:
                    pred = dt(0)
                    for j in range(K):
                        pred = dt(pred + dt(ahat[prev, j] * a[j, k]))
                u[k] = dt(bt[t, k] * pred)
                s = dt(s + u[k])
            c[t] = s
            for k in range(K):
                ahat[t, k] = dt(u[k] / s)
            loglik += float(np.log(np.float64(s))) + float(mt)
            prev = t
        if smooth and good:
            bhat = np.ones(K, dtype=dtype)
            for i in range(len(good) - 1, -1, -1):
                t = good[i]
                for k in range(K):
                    gamma[t, k] = dt(ahat[t, k] * bhat[k])
                if i == 0:
                    first += gamma[t].astype(np.float64)
                    break
                p = good[i - 1]
                e = np.zeros(K, dtype=dtype)
                for k in range(K):
                    e[k] = dt(dt(bt[t, k] * bhat[k]) / c[t])
                for j in range(K):
                    acc = dt(0)
                    for k in range(K):
                        G[j, k] += float(ahat[p, j]) * float(e[k])
                        acc = dt(acc + dt(a[j, k] * e[k]))
                    bhat[j] = acc
    xi = a.astype(np.float64) * G
    return dict(gamma=gamma if smooth else ahat, ahat=ahat, c=c, m=m, loglik=loglik, G=G, xi=xi, first=first, n_good=len(good))


def forward_backward_fast(logn, bad, init, trans, dtype=np.float64, smooth=True):
    """forward_backward with the loops over k and j vectorised: the same dict without c."""
    logn = np.asarray(logn).astype(dtype)
    L, K = logn.shape
    pi = np.asarray(init, dtype=np.float32).astype(dtype)
    a = np.asarray(trans, dtype=np.float32).astype(dtype)
    good = np.flatnonzero(~np.asarray(bad))
    gamma, ahat_all, m_all = np.zeros((L, K), dtype=dtype), np.zeros((L, K), dtype=dtype), np.zeros(L, dtype=dtype)
    G, first = np.zeros((K, K)), np.zeros(K)
    n = len(good)
    if not n:
        return dict(gamma=gamma, ahat=ahat_all, m=m_all, loglik=0.0, G=G, xi=G.copy(), first=first, n_good=0)
    with np.errstate(all='ignore'):
        lg = logn[good]
        m = lg.max(axis=1)
        bt = np.exp(lg - m[:, None])
        ahat, c = np.zeros((n, K), dtype=dtype), np.zeros(n, dtype=dtype)
        for i in range(n):
            u = bt[i] * (pi if i == 0 else (ahat[i - 1][:, None] * a).sum(axis=0, dtype=dtype))
            c[i] = u.sum(dtype=dtype)
            ahat[i] = u / c[i]
        ll = float((np.log(c.astype(np.float64)) + m.astype(np.float64)).sum())
        ahat_all[good], m_all[good] = ahat, m
        if smooth:
            bhat = np.ones(K, dtype=dtype)
            for i in range(n - 1, -1, -1):
                gamma[good[i]] = ahat[i] * bhat
                if i == 0:
                    first += gamma[good[i]].astype(np.float64)
                    break
                e = bt[i] * bhat / c[i]
                G += np.outer(ahat[i - 1].astype(np.float64), e.astype(np.float64))
                bhat = (a * e[None, :]).sum(axis=1, dtype=dtype)
        else:
            gamma[good] = ahat
    return dict(gamma=gamma, ahat=ahat_all, m=m_all, loglik=ll, G=G, xi=a.astype(np.float64) * G, first=first, n_good=n)


def brute_force(logn, bad, init, trans):
    """The same quantities by enumeration of all K^n paths over the good frames, float64: (gamma, loglik, xi, first)."""
    logn = np.asarray(logn, dtype=np.float64)
    L, K = logn.shape
    pi = np.asarray(init, dtype=np.float32).astype(np.float64)
    a = np.asarray(trans, dtype=np.float32).astype(np.float64)
    good = [t for t in range(L) if not bad[t]]
    gamma, xi, first = np.zeros((L, K)), np.zeros((K, K)), np.zeros(K)
    if not good:
        return gamma, 0.0, xi, first
    shift = sum(logn[t].max() for t in good)
    b = {t: np.exp(logn[t] - logn[t].max()) for t in good}
    total = 0.0
    for z in itertools.product(range(K), repeat=len(good)):
        p = pi[z[0]] * b[good[0]][z[0]]
        for i in range(1, len(good)):
            p *= a[z[i - 1], z[i]] * b[good[i]][z[i]]
        total += p
        first[z[0]] += p
        for i, t in enumerate(good):
            gamma[t, z[i]] += p
            if i:
                xi[z[i - 1], z[i]] += p
    return gamma / total, float(np.log(total) + shift), xi / total, first / total


def corpus(logn, bad, off, lens, init, trans, dtype=np.float64, smooth=True, fast=True):
    """Every utterance of a table: dict(post, ahat [T, K], m [T], loglik [n], n_good [n], xi [K, K], first [K],
    xi_utt [n, K, K], first_utt [n, K])."""
    T, K = np.asarray(logn).shape
    fb = forward_backward_fast if fast else forward_backward
    post, ahat, m = np.zeros((T, K), dtype=dtype), np.zeros((T, K), dtype=dtype), np.zeros(T, dtype=dtype)
    ll, ng, xis, firsts = [], [], [], []
    for o, n in zip(off, lens):
        r = fb(logn[o:o + n], bad[o:o + n], init, trans, dtype, smooth)
        post[o:o + n], ahat[o:o + n], m[o:o + n] = r['gamma'], r['ahat'], r['m']
        ll.append(r['loglik'])
        ng.append(r['n_good'])
        xis.append(r['xi'])
        firsts.append(r['first'])
    xis, firsts = np.array(xis).reshape(len(ll), K, K), np.array(firsts).reshape(len(ll), K)
    return dict(post=post, ahat=ahat, m=m, loglik=np.array(ll), n_good=np.array(ng, dtype=np.int64), xi=xis.sum(axis=0),
                first=firsts.sum(axis=0), xi_utt=xis, first_utt=firsts)


def floor_rows(p):
    """Every entry below TRANS_MIN raised to it and each row renormalised once (a vector is one row)."""
    p = np.array(p, dtype=np.float64)
    p[p < TRANS_MIN] = TRANS_MIN
    return p / p.sum(axis=-1, keepdims=True)


def mstep(xi, first, trans, init, alpha):
    """The M-step in float64: (trans, init).  trans[j][k] = (xi[j][k] + alpha) / (sum_k xi[j][k] + K alpha), init likewise
    from `first`; a row without mass at alpha = 0 keeps its old values; then the floor."""
    xi, first = np.asarray(xi, dtype=np.float64), np.asarray(first, dtype=np.float64)
    old_t, old_i = np.asarray(trans, dtype=np.float64), np.asarray(init, dtype=np.float64)
    K = len(first)
    new_t = np.zeros((K, K))
    for j in range(K):
        den = xi[j].sum() + K * alpha
        new_t[j] = (xi[j] + alpha) / den if den > 0 else old_t[j]
    den = first.sum() + K * alpha
    new_i = (first + alpha) / den if den > 0 else old_i
    return floor_rows(new_t), floor_rows(new_i)


def bigram_counts(ids_by_name, K):
    """int64 [K][K]: the unit bigrams of decoded id sequences, BAD frames (-1) passed over."""
    counts = np.zeros((K, K), dtype=np.int64)
    for ids in ids_by_name.values():
        prev = None
        for v in np.asarray(ids).tolist():
            if v < 0:
                continue
            if prev is not None:
                counts[prev, v] += 1
            prev = v
    return counts


def em(utterances, init, trans, alpha, n_iter=10):
    """Float64 EM on init and trans over [(logn, bad), ...], the emissions fixed: (inits, transs [n_iter + 1], total
    log-likelihoods [n_iter]).  The parameters stay float64 between the iterations (forward_backward_fast is given them
    as they are: float32 rounding would break the monotonicity the test is about)."""
    inits, transs, lls = [np.asarray(init, dtype=np.float64)], [np.asarray(trans, dtype=np.float64)], []
    K = len(inits[0])
    for _ in range(n_iter):
        xi, first, LL = np.zeros((K, K)), np.zeros(K), 0.0
        for logn, bad in utterances:
            r = _fb64(logn, bad, inits[-1], transs[-1])
            xi += r[0]
            first += r[1]
            LL += r[2]
        lls.append(LL)
        t, i = mstep(xi, first, transs[-1], inits[-1], alpha)
        transs.append(t)
        inits.append(i)
    return inits, transs, lls


def _fb64(logn, bad, pi, a):
    """(xi, first, loglik) of one utterance with float64 parameters."""
    lg = np.asarray(logn, dtype=np.float64)[~np.asarray(bad)]
    n, K = lg.shape
    if not n:
        return np.zeros((K, K)), np.zeros(K), 0.0
    m = lg.max(axis=1)
    bt = np.exp(lg - m[:, None])
    ahat, c = np.zeros((n, K)), np.zeros(n)
    for i in range(n):
        u = bt[i] * (pi if i == 0 else ahat[i - 1] @ a)
        c[i] = u.sum()
        ahat[i] = u / c[i]
    G, bhat = np.zeros((K, K)), np.ones(K)
    for i in range(n - 1, 0, -1):
        e = bt[i] * bhat / c[i]
        G += np.outer(ahat[i - 1], e)
        bhat = a @ e
    return a * G, ahat[0] * bhat, float((np.log(c) + m).sum())


def planted_cycle(seed, K=3, D=3, n_utt=120, L=40, stay=0.8, scale=4.0):
    """A corpus from K units with a cyclic transition structure (k stays with probability `stay`, otherwise goes to
    k + 1 mod K): (x [n_utt L, D] float32, lens, means [K, D], labels); unit variances."""
    rng = np.random.default_rng(seed)
    mu = rng.normal(size=(K, D)) * scale
    rows, labels = [], []
    for _ in range(n_utt):
        z = int(rng.integers(0, K))
        for t in range(L):
            if t > 0 and rng.random() > stay:
                z = (z + 1) % K
            rows.append(mu[z] + rng.normal(size=D))
            labels.append(z)
    return np.asarray(rows, dtype=np.float32), np.full(n_utt, L, dtype=np.int64), mu, np.asarray(labels)
