"""Baum-Welch training of the sticky HMM of abnet3_amd/hmm.py restated in numpy (test infrastructure only); tests/hmm_np.py
holds the recursion itself and is imported, not changed.

The model as a generative story: z_first ~ w; at every later good frame the unit stays with probability rho, otherwise
it is redrawn from w (and may come back the same); emissions are diagonal Gaussians.  The complete data hold the switch
variable.  E-step, per component k over all good frames, gamma the smoothed posteriors:
    N[k] = sum_t gamma_t(k),  S1[k][d] = sum_t gamma_t(k) xc,  S2[k][d] = sum_t gamma_t(k) xc^2     (xc, xc^2 in fp32)
    stay_k[k] = sum over the transitions (p -> t) of rho ahat_p[k] e_t[k],  e_t = bt[t] bhat / c_t  (hmm_np's names)
M-step, float64:
    m = S1 / N,  v = max(S2 / N - m^2, var_floor gv[d]);  a component with N < min_count keeps its mean and variance;
      with the means held fixed v = max(S2 / N - 2 m S1 / N + m^2, var_floor gv[d]);
    draws[k] = max(N[k] - stay_k[k], 0): the expected number of times k was drawn from w, as a first frame or as a redraw;
      w = draws / sum draws;  a weight below WEIGHT_MIN = 2^-80 becomes exactly 0 and the rest are renormalised;
    rho = sum_k stay_k / sum_u max(n_good_u - 1, 0), clipped to [0, 0.9999] and rounded to float32.

`dtype` float64 is the reference; float32 is the yardstick in hmm_np's convention: the scores, the recursion and the
statistics' products and sums rounded to fp32 in this file's order, the M-step in float64 either way."""
import itertools

import numpy as np

import gmm_np
import hmm_np

STAY_MAX = 0.9999
WEIGHT_MIN = 2.0 ** -80


def forward_backward(logn, bad, w32, rho, dtype=np.float64):
    """One utterance, hmm_np.forward_backward_fast's recursion line for line, and the per-component stays:
    dict(gamma [L, K], loglik, stays, n_good, stay_k [K] float64, draws [K] float64 = sum_t gamma - stay_k)."""
    dt = np.dtype(dtype).type
    logn = np.asarray(logn).astype(dtype)
    w32 = np.asarray(w32, dtype=np.float32)
    w = w32.astype(dtype)
    rho32 = np.float32(rho)
    r, omr = dt(rho32), dt(np.float32(1.0) - rho32)
    good = np.flatnonzero(~np.asarray(bad))
    L, K = logn.shape
    gamma = np.zeros((L, K), dtype=dtype)
    sk = np.zeros(K)
    if not len(good):
        return dict(gamma=gamma, loglik=0.0, stays=0.0, n_good=0, stay_k=sk, draws=np.zeros(K))
    with np.errstate(all='ignore'):
        lg = logn[good]
        m = np.where(w32 > 0, lg, dt(-np.inf)).max(axis=1)
        bt = np.where(w32 > 0, np.exp(lg - m[:, None]), dt(0))
        n = len(good)
        ahat, c = np.zeros((n, K), dtype=dtype), np.zeros(n, dtype=dtype)
        for i in range(n):
            u = bt[i] * (w if i == 0 else r * ahat[i - 1] + omr * w)
            c[i] = u.sum(dtype=dtype)
            ahat[i] = u / c[i]
        ll = float((np.log(c.astype(np.float64)) + m.astype(np.float64)).sum())
        stays = 0.0
        bhat = np.ones(K, dtype=dtype)
        for i in range(n - 1, -1, -1):
            gamma[good[i]] = ahat[i] * bhat
            if i == 0:
                break
            e = bt[i] * bhat / c[i]
            terms = ahat[i - 1].astype(np.float64) * e.astype(np.float64)
            stays += float(r) * float(terms.sum())
            sk += float(r) * terms
            bhat = r * e + omr * (w * e).sum(dtype=dtype)
    return dict(gamma=gamma, loglik=ll, stays=stays, n_good=n, stay_k=sk,
                draws=gamma.astype(np.float64).sum(axis=0) - sk)


def brute_force(logn, bad, w32, rho):
    """(stay_k [K], draws [K]) by enumeration of all K^n paths over the good frames TOGETHER WITH all 2^(n - 1) switch
    sequences (stay / redraw at every transition), float64: a stay keeps the unit with probability rho, a redraw draws
    the next unit from w with probability 1 - rho; the first frame is a draw."""
    logn = np.asarray(logn, dtype=np.float64)
    L, K = logn.shape
    w = np.asarray(w32, dtype=np.float32).astype(np.float64)
    r = float(np.float32(rho))
    omr = float(np.float32(1.0) - np.float32(rho))
    good = [t for t in range(L) if not bad[t]]
    sk, dr = np.zeros(K), np.zeros(K)
    if not good:
        return sk, dr
    b = [np.exp(logn[t] - logn[t][w > 0].max()) for t in good]
    n, total = len(good), 0.0
    for z in itertools.product(range(K), repeat=n):
        for s in itertools.product((False, True), repeat=n - 1):          # True: the unit stayed into frame i + 1
            p = w[z[0]] * b[0][z[0]]
            for i in range(1, n):
                p *= (r if z[i] == z[i - 1] else 0.0) if s[i - 1] else omr * w[z[i]]
                p *= b[i][z[i]]
            if p == 0.0:
                continue
            total += p
            dr[z[0]] += p
            for i in range(1, n):
                (sk if s[i - 1] else dr)[z[i]] += p
    return sk / total, dr / total


def e_step(xc, bad, off, lens, w, m, v, rho, dtype=np.float64):
    """The corpus under (w, centred means m, variances v, rho): dict(gamma [T, K], sums [K, 2D + 1] = [S1 | S2 | N] float64,
    stay_k [n_utt, K], loglik, stays, n_good [n_utt], scores [T, K])."""
    A, B, _ = gmm_np.tables(w, m, v)
    s = gmm_np.scores(xc, bad, A, B, hmm_np.emission_offsets(m, v), dtype)
    w32 = np.asarray(w, dtype=np.float64).astype(np.float32)
    gamma = np.zeros(s.shape, dtype=dtype)
    sk, ll, st, ng = [], [], [], []
    for o, n in zip(off, lens):
        r = forward_backward(s[o:o + n], bad[o:o + n], w32, rho, dtype)
        gamma[o:o + n] = r['gamma']
        sk.append(r['stay_k'])
        ll.append(r['loglik'])
        st.append(r['stays'])
        ng.append(r['n_good'])
    N, S1, S2 = gmm_np.statistics(gamma, xc, bad, dtype)
    sums = np.concatenate([S1, S2, N[:, None]], axis=1).astype(np.float64)
    return dict(gamma=gamma, sums=sums, stay_k=np.array(sk).reshape(len(lens), -1), loglik=np.array(ll), stays=np.array(st),
                n_good=np.array(ng, dtype=np.int64), scores=s)


def m_step(sums, stay_k_total, n_trans, w, m, v, rho, gv, var_floor=0.01, min_count=1.0, params='mvws', stays_total=None):
    """(w, m, v, rho, n_retired) of the M-step above, float64; a letter missing from params holds its parameter."""
    sums = np.asarray(sums, dtype=np.float64)
    K, D = np.shape(m)
    N, S1, S2 = sums[:, 2 * D], sums[:, :D], sums[:, D:2 * D]
    w, m, v = (np.array(a, dtype=np.float64) for a in (w, m, v))
    floor = var_floor * np.asarray(gv, dtype=np.float64)
    for k in range(K):
        if N[k] < min_count:
            continue
        m1 = S1[k] / N[k]
        if 'v' in params:
            second = S2[k] / N[k] - m1 * m1 if 'm' in params else S2[k] / N[k] - 2.0 * m[k] * m1 + m[k] * m[k]
            v[k] = np.maximum(second, floor)
        if 'm' in params:
            m[k] = m1
    if 'w' in params:
        draws = np.maximum(N - np.asarray(stay_k_total, dtype=np.float64), 0.0)
        w = draws / draws.sum()
        w[w < WEIGHT_MIN] = 0.0
        w = w / w.sum()
    if 's' in params:
        num = float(np.sum(stay_k_total)) if stays_total is None else float(stays_total)
        rho = float(np.float32(min(max(num / n_trans, 0.0), STAY_MAX)))
    return w, m, v, rho, int((w == 0).sum())


def em(xc, bad, off, lens, w, m, v, rho, gv, n_iter=10, tol=-np.inf, params='mvws', var_floor=0.01, min_count=1.0,
       dtype=np.float64, stay_from_stays=False):
    """StickyHmmPosteriorgram.fit restated: dict(w, m, v, rho, log_likelihoods (per good frame), rhos, totals (the
    total log-likelihoods)).  stay_from_stays: the stay update from the utterances' scalar stays (hmm_np.em_stay's
    number) instead of sum_k stay_k."""
    rho = float(np.float32(rho))
    lls, rhos, totals = [], [rho], []
    for it in range(n_iter):
        r = e_step(xc, bad, off, lens, w, m, v, rho, dtype)
        S = 0.0
        for s in r['stays']:
            S += s
        n, ntr = int(r['n_good'].sum()), int(np.maximum(r['n_good'] - 1, 0).sum())
        total = 0.0
        for l in r['loglik']:
            total += l
        totals.append(total)
        lls.append(total / n)
        if it > 0 and lls[-1] - lls[-2] < tol:
            break
        w, m, v, rho, _ = m_step(r['sums'], r['stay_k'].sum(axis=0), ntr, w, m, v, rho, gv, var_floor, min_count, params,
                                 stays_total=S if stay_from_stays else None)
        rhos.append(rho)
    return dict(w=w, m=m, v=v, rho=rho, log_likelihoods=lls, rhos=rhos, totals=totals)


def perturbed_start(seed, n_utt=60, L=50):
    """hmm_np.planted(seed, n_utt, L) and a start away from the truth: (x, lens, shift float32, gv, w, centred m, v)."""
    x, lens, w_true, mu = hmm_np.planted(seed, n_utt=n_utt, L=L)
    shift, gv = gmm_np.moments(x)
    rng = np.random.default_rng(100 + seed)
    m = mu - shift.astype(np.float64) + 0.7 * rng.normal(size=mu.shape)
    v = np.full(mu.shape, 2.0)
    w = np.full(len(w_true), 1.0 / len(w_true))
    return x, lens, shift, gv, w, m, v
