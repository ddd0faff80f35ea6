"""Numpy restatement of the term-discovery prefilter (abnet3_amd/prefilter.py's module docstring): the signatures in
float64 with the forward error bound of a float32 dot product, `live`, the diagonal runs of the dot plot with explicit
loops over diagonals, the tie order and the refusals, and TermPrefilter.keep.  Test infrastructure only."""
import numpy as np

CAP = 512           # abn_dtw_local_max_n2()
U24 = 2.0 ** -24    # the unit roundoff of float32


def planes(D, bits=64, seed=0):
    return np.random.default_rng(seed).standard_normal((bits, D)).astype(np.float32)


def live(table):
    """uint8 [rows]: every element finite and at least one non-zero."""
    t = np.asarray(table)
    return (np.isfinite(t).all(axis=1) & (t != 0).any(axis=1)).astype(np.uint8)


def dots(table, pl):
    """(dot, bound) float64 [rows, bits]: the exact-to-float64 dot products and the forward error bound of ANY float32
    summation order, fused or not: 2 D 2^-24 sum_k |x_k p_k| (gamma_D = D u / (1 - D u) <= 2 D u for D <= 4096)."""
    x, p = np.asarray(table, dtype=np.float64), np.asarray(pl, dtype=np.float64)
    with np.errstate(all='ignore'):
        return x @ p.T, 2.0 * x.shape[1] * U24 * (np.abs(x) @ np.abs(p).T)


def pack(bits01):
    """uint32 [rows, bits // 32] of a 0 / 1 array [rows, bits]: bit b is bit b % 32 of word b // 32."""
    rows, bits = bits01.shape
    w = np.zeros((rows, bits // 32), dtype=np.uint32)
    for b in range(bits):
        w[:, b // 32] |= (bits01[:, b].astype(np.uint32) << np.uint32(b % 32))
    return w


def unpack(sig, bits):
    sig = np.asarray(sig).view(np.uint32) if np.asarray(sig).dtype == np.int32 else np.asarray(sig, dtype=np.uint32)
    return np.stack([(sig[:, b // 32] >> np.uint32(b % 32)) & np.uint32(1) for b in range(bits)], axis=1).astype(np.uint8)


def signatures(table, pl):
    """(sig uint32 [rows, words], live uint8 [rows], decided bool [rows, bits]): the float64 signs, dead rows' words 0;
    `decided` marks the (row, bit) entries whose |dot| exceeds the bound -- a float32 sum cannot get those wrong."""
    lv = live(table)
    safe = np.where(lv[:, None] != 0, np.asarray(table, dtype=np.float64), 0.0)
    d, bound = dots(safe, pl)
    return pack(((d > 0) & (lv[:, None] != 0)).astype(np.uint8)), lv, np.abs(d) > bound


POP16 = np.array([bin(v).count('1') for v in range(1 << 16)], dtype=np.uint8)


def popcount(a):
    """The set bits of every uint32 of a (a table of the 16-bit halves)."""
    a = np.asarray(a, dtype=np.uint32)
    return POP16[a & np.uint32(0xffff)].astype(np.int64) + POP16[a >> np.uint32(16)]


def hit_matrix(sig1, live1, o1, n, sig2, live2, o2, m, max_hamming, exclude=0):
    """bool [n, m]: hit(i, j)."""
    a, b = np.asarray(sig1[o1:o1 + n], dtype=np.uint32), np.asarray(sig2[o2:o2 + m], dtype=np.uint32)
    ham = popcount(a[:, None, :] ^ b[None, :, :]).sum(axis=-1)
    hit = (ham <= max_hamming) & (np.asarray(live1[o1:o1 + n]) != 0)[:, None] & (np.asarray(live2[o2:o2 + m]) != 0)[None, :]
    if exclude > 0:
        gap = (o1 + np.arange(n, dtype=np.int64))[:, None] - (o2 + np.arange(m, dtype=np.int64))[None, :]
        hit &= np.abs(gap) >= exclude
    return hit


def runs(hit, span, dilate=0):
    """(best, diag, end1) of a hit matrix [n, m]: hd = the hits spread over |t| <= dilate columns inside the matrix;
    run(i, j) = the hd along the diagonal in the `span` cells ending at (i, j); the largest run, ties to the smallest
    i - j, then the smallest i; nothing: (0, 0, -1).  One loop per diagonal, one step per cell."""
    n, m = hit.shape
    if n == 0 or m == 0:
        return 0, 0, -1
    hd = np.zeros((n, m), dtype=bool)
    for t in range(-dilate, dilate + 1):
        lo, hi = max(0, -t), min(m, m - t)              # columns j with 0 <= j + t < m
        if lo < hi:
            hd[:, lo:hi] |= hit[:, lo + t:hi + t]
    best, diag, end1 = 0, 0, -1
    for k in range(-(m - 1), n):                        # ascending diagonals: a strict > keeps the smallest i - j
        c = np.cumsum(np.diagonal(hd, -k), dtype=np.int64)      # hd(i, i - k) for i = max(0, k) ...: the cells inside the matrix
        run = c.copy()
        run[span:] -= c[:-span]                         # the last `span` cells up to each one
        e = int(np.argmax(run))                         # the first of equal maxima: the smallest i
        if run[e] > best:
            best, diag, end1 = int(run[e]), k, max(0, k) + e
    return best, diag, end1


def runs_slow(hit, span, dilate=0):
    """runs() once more, cell by cell from the definition (small matrices: the hand-made cases check runs against it)."""
    n, m = hit.shape
    best, diag, end1 = 0, 0, -1
    key = None
    for i in range(n):
        for j in range(m):
            run = 0
            for s in range(span):
                if i - s >= 0 and j - s >= 0:
                    run += int(any(hit[i - s, j - s + t] for t in range(-dilate, dilate + 1) if 0 <= j - s + t < m))
            if run > 0 and (key is None or (-run, i - j, i) < key):
                key, best, diag, end1 = (-run, i - j, i), run, i - j, i
    return best, diag, end1


def diag_hits(sig1, live1, off1, n1, sig2, live2, off2, n2, max_hamming, span=32, dilate=0, exclude=0, cap=CAP):
    """The kernel's outputs for a pair table: (best, diag, end1) int32 [P].  A pair outside its tables, with a negative
    length or a side 2 beyond `cap` is refused: (-1, 0, -1)."""
    P = len(n1)
    best, diag, end1 = np.zeros(P, np.int32), np.zeros(P, np.int32), np.full(P, -1, np.int32)
    rows1, rows2 = len(sig1), len(sig2)
    for p in range(P):
        o1, n, o2, m = int(off1[p]), int(n1[p]), int(off2[p]), int(n2[p])
        if n < 0 or m < 0 or o1 < 0 or o2 < 0 or o1 + n > rows1 or o2 + m > rows2 or m > cap:
            best[p] = -1
            continue
        if n and m:
            best[p], diag[p], end1[p] = runs(hit_matrix(sig1, live1, o1, n, sig2, live2, o2, m, max_hamming, exclude), span, dilate)
    return best, diag, end1


def best_runs(sig, live_, base, lengths, kp, exclude, max_hamming, span, dilate):
    """best [len(kp)] over TermDiscoverer's kernel pairs (u, v, first frame of the window, frames) of utterances at
    table rows base[u] .. base[u] + lengths[u]: the pairs of an utterance with itself under `exclude`, the others 0."""
    out = np.zeros(len(kp), dtype=np.int32)
    for p, (u, v, w0, wn) in enumerate(kp):
        b, _, _ = diag_hits(sig, live_, [base[u]], [lengths[u]], sig, live_, [base[v] + w0], [wn], max_hamming, span, dilate,
                            exclude if u == v else 0)
        out[p] = b[0]
    return out


def keep(best, min_hits):
    return np.asarray(best) >= min_hits
