"""abnet3_amd/kmeans.py's penalised segmentation and abnet3_amd/tde.py's boundary scores restated with explicit loops: the
reference the unit tests compare the kernel with.

The definition (inputs: the fp32 scores s[t, k] of tests/kmeans_np.py's `scores`, rounded to fp32):

* An utterance is the len[u] rows from off[u].  The chain runs over its good frames in order; a BAD frame keeps id -1,
  neither breaks the chain nor pays: the state passes through unchanged.
* penalty >= 0 is in the units of the distortion d2 = |xc - m|^2 = |xc|^2 - 2 s, so in score units p = fp32(penalty / 2).
* Objective: choose a[t] to maximise  J(a) = sum_t s[t, a_t] - p #{consecutive good frames with different ids}.
* Recurrence, all fp32, normalised so that nothing grows with T:
    first good frame:  U[k] = s[t, k]
    later good frames: stay[t, k] = (W[k] > -p)  (strict),  U[k] = s[t, k] + (stay[t, k] ? W[k] : -p)
    every good frame:  M_t = max_k U[k],  j*[t] = the lowest k attaining it,  W[k] = U[k] - M_t
  objective[u] = the sum of the M_t in frame order, in float64.
* Traceback: the last good frame's id is its j*; going backwards the previous good frame's id is the same id if
  stay[t, a_t], otherwise j* of the previous good frame.  n_switch[u] = the switches on the path.
* With penalty = 0 nothing stays: every id is j*[t] = the frame-wise argmax, lowest k on ties.
* No good frame: all ids -1, objective 0, 0 switches.  len[u] = 0 is allowed.

The allowance of the float comparison (test 7).  Let s64 be the float64 scores of the fp32 operands and J64(a) the
objective evaluated with them in float64.  The kernel's recurrence is exact dynamic programming for a problem whose
cell scores are s'[t, k] = s64[t, k] + e[t, k]:
  * |fp32 score - s64| <= E[t]  (kmeans_np.scores' allowance: a dot product of depth D + 1 in any order);
  * each step rounds twice, the addition U = s + (W or -p) and the subtraction W = U - M.  Either result is at most
    max|U| <= max|s| + p in magnitude (W <= 0 and W > -p where it is used, else -p is used), so each rounding is at
    most 2^-24 (max|s| + p); an error in W[k] at step t is an error in the cell (t + 1, k)'s incoming value, i.e. it
    can be charged to a cell score.
  So |e| <= delta = max_t E[t] + 2 * 2^-24 (max|s| + p) per good frame, and for every labelling a,
  |J'(a) - J64(a)| <= n_good delta.  The device path a* maximises J', the float64 path a64 maximises J64:
      J64(a64) >= J64(a*) >= J'(a*) - n delta >= J'(a64) - n delta >= J64(a64) - 2 n delta.
  The device objective is J'(a*) up to the same roundings, within n delta of J64(a*): within 2 n delta of J64(a64) too.
"""
import itertools

import numpy as np

U = 2.0 ** -24


def score_penalty(penalty):
    return np.float32(np.float64(penalty) / 2.0)


def viterbi_one(s, good, p):
    """(ids int32 [L], objective float, n_switch int) of one utterance: s [L, K] float32, good [L] bool, p fp32."""
    L, K = s.shape
    p = np.float32(p)
    ids = np.full(L, -1, dtype=np.int32)
    frames = [t for t in range(L) if good[t]]
    if not frames:
        return ids, 0.0, 0
    stay = np.zeros((L, K), dtype=bool)
    jstar = {}
    W = None
    objective = 0.0
    for t in frames:
        Uv = np.empty(K, dtype=np.float32)
        for k in range(K):
            if W is None:
                Uv[k] = s[t, k]
            else:
                stay[t, k] = W[k] > -p
                Uv[k] = np.float32(s[t, k] + (W[k] if stay[t, k] else -p))
        M = Uv[0]
        j = 0
        for k in range(1, K):
            if Uv[k] > M:
                M, j = Uv[k], k
        jstar[t] = j
        W = (Uv - M).astype(np.float32)
        objective += float(M)
    a = jstar[frames[-1]]
    n_switch = 0
    for i in range(len(frames) - 1, -1, -1):
        t = frames[i]
        ids[t] = a
        if i > 0 and not stay[t, a]:
            b = jstar[frames[i - 1]]
            n_switch += int(b != a)          # (b == a only with p = 0, where nothing stays: W[j*] = 0 > -p otherwise)
            a = b
    return ids, objective, n_switch


def viterbi(s, good, off, lens, p, ids=None):
    """The corpus call: (ids [T] int32, objective [n_utt] float64, n_switch [n_utt] int32).  Rows outside every
    utterance keep what `ids` held (-7 where none is given)."""
    T = s.shape[0]
    out = np.full(T, -7, dtype=np.int32) if ids is None else np.array(ids, dtype=np.int32)
    obj = np.zeros(len(off), dtype=np.float64)
    nsw = np.zeros(len(off), dtype=np.int32)
    for u, (o, n) in enumerate(zip(off, lens)):
        o, n = int(o), int(n)
        out[o:o + n], obj[u], nsw[u] = viterbi_one(np.asarray(s[o:o + n], dtype=np.float32), good[o:o + n], p)
    return out, obj, nsw


def switches(ids):
    a = np.asarray(ids)
    a = a[a >= 0]
    return int((a[1:] != a[:-1]).sum())


def J(s, ids, p):
    """The objective of a labelling, in float64 from the given scores (BAD frames: id -1, skipped)."""
    ids = np.asarray(ids)
    t = np.nonzero(ids >= 0)[0]
    return float(np.asarray(s, dtype=np.float64)[t, ids[t]].sum() - float(p) * switches(ids))


def brute_force(s, good, p):
    """(best J, the set of all labellings of the good frames attaining it) over every labelling: tiny cases only."""
    L, K = s.shape
    frames = [t for t in range(L) if good[t]]
    best, arg = -np.inf, []
    for lab in itertools.product(range(K), repeat=len(frames)):
        ids = np.full(L, -1, dtype=np.int64)
        ids[frames] = lab
        v = J(s, ids, p)
        if v > best:
            best, arg = v, [tuple(lab)]
        elif v == best:
            arg.append(tuple(lab))
    return (best if frames else 0.0), arg


def optimum_f64(s64, good, p):
    """The float64 optimum of J over one utterance by the textbook DP (no normalisation, no ids)."""
    V = None
    for t in range(s64.shape[0]):
        if not good[t]:
            continue
        V = s64[t].copy() if V is None else s64[t] + np.maximum(V, V.max() - float(p))
    return 0.0 if V is None else float(V.max())


def delta(E, smax, p):
    """The per-cell perturbation of the module docstring."""
    return float(np.max(E)) + 2.0 * U * (float(smax) + float(p))


def runs(ids):
    """(start, end, unit) int arrays: the runs of equal ids, frames start .. end - 1, BAD frames left out (a BAD frame
    ends a run)."""
    ids = np.asarray(ids)
    out = []
    t = 0
    while t < len(ids):
        e = t + 1
        while e < len(ids) and ids[e] == ids[t]:
            e += 1
        if ids[t] >= 0:
            out.append((t, e, int(ids[t])))
        t = e
    return tuple(np.array([r[i] for r in out], dtype=np.int64) for i in range(3))


def boundary_scores(found, gold, tolerance=0.02):
    """{file: sorted found times}, {file: sorted gold boundary times} -> precision, recall, F, OS, R-value, in float64.
    Two pointers over the sorted lists: |f - g| <= tolerance is a hit and both advance, otherwise the smaller does."""
    hits = n_found = n_gold = 0
    for name in gold:
        f = sorted(float(v) for v in found.get(name, ()))
        g = sorted(float(v) for v in gold[name])
        n_found += len(f)
        n_gold += len(g)
        i = j = 0
        while i < len(f) and j < len(g):
            if abs(f[i] - g[j]) <= tolerance:
                hits += 1
                i += 1
                j += 1
            elif f[i] < g[j]:
                i += 1
            else:
                j += 1
    prec = hits / n_found if n_found else 0.0
    rec = hits / n_gold if n_gold else 0.0
    F = 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0
    OS = rec / prec - 1.0 if prec > 0 else 0.0
    r1 = np.sqrt((1.0 - rec) ** 2 + OS ** 2)
    r2 = abs((-OS + rec - 1.0) / np.sqrt(2.0))
    return {'precision': prec, 'recall': rec, 'f': F, 'os': OS, 'r_value': 1.0 - (r1 + r2) / 2.0,
            'n_found': n_found, 'n_gold': n_gold, 'n_hit': hits}


def exact_case(T, K, D, seed):
    """Exact inputs for the kernel's tests: integer frames in runs around integer centroids,
    (x [T, D], m [K, D], b [K], s [T, K] float32), every fp32 operation of the score GEMM exact."""
    rng = np.random.default_rng(seed)
    m = rng.integers(-2, 3, size=(K, D)).astype(np.float32)
    lab = np.repeat(rng.integers(0, K, size=T // 3 + 1), 3)[:T]
    x = (m[lab] + rng.integers(-1, 2, size=(T, D))).astype(np.float32)
    b = (-0.5 * (m.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    s = (x.astype(np.float64) @ m.astype(np.float64).T + b.astype(np.float64)).astype(np.float32)
    assert np.array_equal(s.astype(np.float64), x.astype(np.float64) @ m.astype(np.float64).T + b.astype(np.float64))
    return x, m, b, s
