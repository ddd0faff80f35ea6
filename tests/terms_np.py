"""Numpy restatement of term discovery (abnet3_amd/terms.py's module docstring): the search's cells with the exclusion
band, the float64 Smith-Waterman recurrence one anti-diagonal at a time with its first-maximum rule and the carried
length and start cell, the best cell with its tie rule, the kernel's refusal rules; then TermDiscoverer's windowing,
filtering, clustering and file texts, and a corpus with planted repeats.  Test infrastructure only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qbe_np  # noqa: E402

CAP = 512           # abn_dtw_local_max_n2()


def cosine_cells(X, Y):
    """[N, M] float64 holding the float32 cells of side-1 frames X against side-2 frames Y (+inf: blocked)."""
    return qbe_np.cosine_cells(X, Y)


def kl_cells(tx, ty):
    return qbe_np.kl_cells(tx, ty)


def exclude_cells(d, o1, o2, exclude):
    """d with the cells |(o1 + i) - (o2 + j)| < exclude blocked (exclude = 0: none)."""
    d = np.array(d, dtype=np.float64)
    if exclude > 0 and d.size:
        gap = (o1 + np.arange(d.shape[0], dtype=np.int64))[:, None] - (o2 + np.arange(d.shape[1], dtype=np.int64))[None, :]
        d[np.abs(gap) < exclude] = np.inf
    return d


def local_align(d, theta):
    """(score, path_len, start1, start2, end1, end2) of the cell matrix d [N, M] (float32 values or +inf) under
    s = float64(float32(theta)) - float64(d).  H(i, j): best = the first maximum of diag, up, left in that order (outside
    the matrix: dead, H = 0, length 0); best > 0: H = best + s, length and start carried; else H = s, length 1, start
    (i, j); not H > 0: dead.  The result is the cell of largest H > 0, ties to the smallest i, then the smallest j."""
    n, m = d.shape
    if n == 0 or m == 0:
        return 0.0, 0, -1, -1, -1, -1
    sim = np.float64(np.float32(theta)) - d.astype(np.float64)
    H = np.zeros((n + 1, m + 1))                        # cell (i, j) lives at [i + 1, j + 1]
    L = np.zeros((n + 1, m + 1), dtype=np.int64)
    SI = np.full((n + 1, m + 1), -1, dtype=np.int64)
    SJ = np.full((n + 1, m + 1), -1, dtype=np.int64)
    for s in range(2, n + m + 1):                       # the cells of an anti-diagonal do not depend on each other
        i = np.arange(max(1, s - m), min(n, s - 1) + 1)
        j = s - i
        dg, up, left = H[i - 1, j - 1], H[i - 1, j], H[i, j - 1]
        take_up = up > dg                               # first maximum in the order diag, up, left
        b1 = np.where(take_up, up, dg)
        take_left = left > b1
        best = np.where(take_left, left, b1)
        pick = lambda A: np.where(take_left, A[i, j - 1], np.where(take_up, A[i - 1, j], A[i - 1, j - 1]))
        ext = best > 0
        h = np.where(ext, best + sim[i - 1, j - 1], sim[i - 1, j - 1])
        live = h > 0
        H[i, j] = np.where(live, h, 0.0)
        L[i, j] = np.where(live, np.where(ext, pick(L) + 1, 1), 0)
        SI[i, j] = np.where(live, np.where(ext, pick(SI), i - 1), -1)
        SJ[i, j] = np.where(live, np.where(ext, pick(SJ), j - 1), -1)
    k = int(np.argmax(H[1:, 1:]))                       # the first of equal maxima in row-major order: smallest i, then j
    e1, e2 = divmod(k, m)
    if not H[e1 + 1, e2 + 1] > 0:
        return 0.0, 0, -1, -1, -1, -1
    return (float(H[e1 + 1, e2 + 1]), int(L[e1 + 1, e2 + 1]), int(SI[e1 + 1, e2 + 1]), int(SJ[e1 + 1, e2 + 1]), e1, e2)


def local_batch(cells, rows1, off1, n1, rows2, off2, n2, theta, exclude=0, cap=CAP):
    """The kernel's outputs for a pair table: (score f64, path_len, start1, start2, end1, end2 int32 [P]).
    cells(o1, n, o2, m) -> [n, m] cell matrix.  A pair outside the tables, with a negative length or a side 2 beyond
    `cap` is refused (path_len -1)."""
    P = len(n1)
    score = np.zeros(P)
    out = [np.zeros(P, dtype=np.int32)] + [np.full(P, -1, dtype=np.int32) for _ in range(4)]
    for p in range(P):
        o1, n, o2, m = int(off1[p]), int(n1[p]), int(off2[p]), int(n2[p])
        if n < 0 or m < 0 or o1 < 0 or o2 < 0 or o1 + n > rows1 or o2 + m > rows2 or m > cap:
            out[0][p] = -1
            continue
        d = exclude_cells(cells(o1, n, o2, m), o1, o2, exclude) if n and m else np.zeros((n, m))
        r = local_align(d, theta)
        score[p] = r[0]
        for a, v in zip(out, r[1:]):
            a[p] = v
    return (score,) + tuple(out)


def local_cosine_batch(f1, off1, n1, f2, off2, n2, theta, exclude=0, cap=CAP):
    return local_batch(lambda o1, n, o2, m: cosine_cells(f1[o1:o1 + n], f2[o2:o2 + m]), len(f1), off1, n1, len(f2), off2, n2,
                       theta, exclude, cap)


def local_kl_batch(t1, off1, n1, t2, off2, n2, theta, exclude=0, cap=CAP):
    return local_batch(lambda o1, n, o2, m: kl_cells([a[o1:o1 + n] for a in t1], [a[o2:o2 + m] for a in t2]),
                       len(t1[0]), off1, n1, len(t2[0]), off2, n2, theta, exclude, cap)


# ---------------------------------------------------------------------------------------------------------------
# TermDiscoverer: windows, matches, clusters, files

def windows(n, window):
    """[(first frame, frames)] of the side-2 windows of an utterance of n frames: `window` frames, hop window // 2,
    the last one flush with the end; one window when the utterance fits; none when it is empty."""
    if n <= 0:
        return []
    if n <= window:
        return [(0, n)]
    hop = max(1, window // 2)
    return [(s, window) for s in range(0, n - window, hop)] + [(n - window, window)]


def kernel_pairs(lengths, pairs, window):
    """[(u, v, first frame of the window in v, frames)] in the module's order: the utterance pairs in the order given,
    each pair's windows by ascending first frame.  Utterances without frames produce nothing."""
    return [(u, v, w0, wn) for u, v in pairs if lengths[u] > 0 for w0, wn in windows(lengths[v], window)]


def all_pairs(n):
    return [(u, v) for u in range(n) for v in range(u, n)]


def keep_matches(kp, result, theta, min_frames, max_distance=None):
    """The kept matches [(file1, first1, last1, file2, first2, last2, score, path_len, distance)] from the kernel pairs
    and their results, in kernel-pair order, a repeat of the same six bounds (two windows that see one match) left out."""
    theta = np.float64(np.float32(theta))
    out, seen = [], set()
    for (u, v, w0, _wn), sc, ln, s1, s2, e1, e2 in zip(kp, *result):
        if ln <= 0 or e1 - s1 + 1 < min_frames or e2 - s2 + 1 < min_frames:
            continue
        dist = float(theta - np.float64(sc) / np.float64(ln))
        if max_distance is not None and dist > max_distance:
            continue
        key = (u, int(s1), int(e1), v, int(w0 + s2), int(w0 + e2))
        if key not in seen:
            seen.add(key)
            out.append(key + (float(sc), int(ln), dist))
    return out


def cluster(matches, merge_overlap=0.5):
    """The clusters [[(file, first, last)]] of the matches: fragment 2k / 2k + 1 are the two stretches of match k; the
    two fragments of a match are joined, and two fragments of one file whose intersection is at least merge_overlap of
    the shorter one; within a cluster the fragments of a file are taken by descending score (then first frame, last
    frame, fragment number) and one that shares a frame with one already taken is dropped; tokens by (file, first
    frame); clusters of fewer than two tokens dropped; clusters by their first token."""
    frag = []
    for m in matches:
        frag.append((m[0], m[1], m[2], m[6]))
        frag.append((m[3], m[4], m[5], m[6]))
    parent = list(range(len(frag)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    for k in range(len(matches)):
        union(2 * k, 2 * k + 1)
    for a in range(len(frag)):
        for b in range(a + 1, len(frag)):
            fa, fb = frag[a], frag[b]
            if fa[0] != fb[0]:
                continue
            inter = min(fa[2], fb[2]) - max(fa[1], fb[1]) + 1
            if inter >= 1 and inter >= merge_overlap * min(fa[2] - fa[1] + 1, fb[2] - fb[1] + 1):
                union(a, b)
    groups = {}
    for x in range(len(frag)):
        groups.setdefault(find(x), []).append(x)
    clusters = []
    for root, members in groups.items():
        tokens = []
        for x in sorted(members, key=lambda x: (-frag[x][3], frag[x][1], frag[x][2], x)):
            f, lo, hi, _ = frag[x]
            if not any(g == f and min(hi, h2) >= max(lo, l2) for g, l2, h2 in tokens):
                tokens.append((f, lo, hi))
        tokens.sort()
        if len(tokens) >= 2:
            clusters.append((tokens[0], root, tokens))
    return [t for _, _, t in sorted(clusters)]


def discover(names, feats, theta, cells='cosine', tables=None, min_frames=50, max_distance=None, exclude=None, window=CAP,
             merge_overlap=0.5, pairs=None):
    """(matches, clusters) of the restatement over the utterances `names` (already in the module's sorted order) of the
    features dict; cells='kl': `tables` {name: (P, L, bad)} host slices.  Files are indices into names.  The exclusion
    (default min_frames) applies to the pairs of an utterance with itself, in frames of that utterance."""
    exclude = min_frames if exclude is None else exclude
    lengths = [len(feats[k]) for k in names]
    kp = kernel_pairs(lengths, all_pairs(len(names)) if pairs is None else pairs, window)
    res = [[] for _ in range(6)]
    for u, v, w0, wn in kp:
        if cells == 'kl':
            d = kl_cells(tables[names[u]], [a[w0:w0 + wn] for a in tables[names[v]]])
        else:
            d = cosine_cells(feats[names[u]], feats[names[v]][w0:w0 + wn])
        if u == v:
            d = exclude_cells(d, 0, w0, exclude)
        for a, x in zip(res, local_align(d, theta)):
            a.append(x)
    matches = keep_matches(kp, res, theta, min_frames, max_distance)
    return matches, cluster(matches, merge_overlap)


def text(name):
    return name.decode('UTF-8') if isinstance(name, bytes) else str(name)


def classes_text(names, times, clusters):
    out = []
    for k, tokens in enumerate(clusters):
        out.append('Class %d\n' % k)
        for f, lo, hi in tokens:
            t = times[names[f]]
            out.append('%s %r %r\n' % (text(names[f]), float(t[lo]), float(t[hi])))
        out.append('\n')
    return ''.join(out)


def pairs_text(matches):
    return ''.join('%d %d %d %d %d %d %.11f\n' % (m[0], m[3], m[1], m[2] + 1, m[4], m[5] + 1, m[8]) for m in matches)


def map_text(names):
    return ''.join('%d %s\n' % (f, text(k)) for f, k in enumerate(names))


# ---------------------------------------------------------------------------------------------------------------
# the end-to-end fixture: utterances of unrelated Gaussian frames with exact copies of a few "words" planted in them

def planted_corpus(seed=11, D=40, lengths=(150, 230, 700, 310, 180), word_lengths=(60, 75, 90)):
    """(feats {name: [T, D]}, times {name: [T]}, planted {word: [(name, first, last)]}).  Unrelated Gaussian frames sit
    near angular distance 0.5, a word's copies at 0 (or the cell's smallest values, 1e-4): under theta = 0.05 nothing
    but a copy pays.  Word w is planted in utterances w, w + 1 and w + 2 (utterance 2 holds all three and needs two windows); the copies of
    different words do not touch."""
    rng = np.random.default_rng(seed)
    words = [rng.standard_normal((n, D)).astype(np.float32) for n in word_lengths]
    names = ['utt%d' % u for u in range(len(lengths))]
    feats = {k: rng.standard_normal((n, D)).astype(np.float32) for k, n in zip(names, lengths)}
    planted = {w: [] for w in range(len(words))}
    at = {0: [(0, 20)], 1: [(0, 30), (1, 120)], 2: [(0, 10), (1, 130), (2, 480)], 3: [(1, 40), (2, 150)], 4: [(2, 70)]}
    for u, spots in at.items():
        for w, lo in spots:
            feats[names[u]][lo:lo + len(words[w])] = words[w]
            planted[w].append((names[u], lo, lo + len(words[w]) - 1))
    times = {k: (np.arange(len(v)) + 0.5) * 0.01 for k, v in feats.items()}
    return feats, times, planted
