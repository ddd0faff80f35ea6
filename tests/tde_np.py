"""The definition abnet3_amd/tde.py computes, restated with explicit loops: the plain two-row Levenshtein DP, the
inclusion rule phone by phone, pair enumeration, NED and coverage.  Standard library and numpy only: nothing of the
package is imported.  Also the synthetic alignment and clusters the host and the GPU tests share."""
import numpy as np


def levenshtein(a, b):
    """Unit-cost edit distance of two sequences, two rows of the DP matrix."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if x == y else 1))
        prev = cur
    return prev[len(b)]


def levenshtein_rows(a, b):
    """The same distance one numpy row at a time, for the long cases of the GPU tests: substitution and deletion are
    elementwise; the insertion chain cur[j] = min(cur[j], cur[j - 1] + 1) is a running minimum of cur[j] - j.
    tests/test_tde_host.py holds it against levenshtein()."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    ramp = np.arange(len(b) + 1, dtype=np.int64)
    prev = ramp.copy()
    for i, x in enumerate(a, 1):
        cur = np.empty_like(prev)
        cur[0] = i
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != x))
        prev = np.minimum.accumulate(cur - ramp) + ramp
    return int(prev[len(b)])


def edit_batch(sym1, off1, n1, sym2, off2, n2, max_short, distance=levenshtein):
    """abn_edit_distance_batched's contract on host arrays: int32 distances, -1 for a refused pair."""
    out = np.empty(len(n1), dtype=np.int32)
    for p, (o1, l1, o2, l2) in enumerate(zip(off1, n1, off2, n2)):
        o1, l1, o2, l2 = int(o1), int(l1), int(o2), int(l2)
        if l1 < 0 or l2 < 0 or o1 < 0 or o2 < 0 or o1 + l1 > len(sym1) or o2 + l2 > len(sym2) or min(l1, l2) > max_short:
            out[p] = -1
        else:
            out[p] = distance(sym1[o1:o1 + l1].tolist(), sym2[o2:o2 + l2].tolist())
    return out


def parse_alignment(lines):
    """{file: [(onset, offset, symbol)] sorted} and {symbol: id} of alignment lines `file onset offset symbol`."""
    files = {}
    for line in lines:
        if line.strip():
            f, on, off, s = line.split()
            files.setdefault(f, []).append((float(on), float(off), s))
    for v in files.values():
        v.sort()
    symbols = sorted({s for v in files.values() for _, _, s in v})
    return files, {s: k for k, s in enumerate(symbols)}


def belongs(tok_on, tok_off, ph_on, ph_off):
    ov = min(tok_off, ph_off) - max(tok_on, ph_on)
    return ov > 0 and (ov >= 0.03 or ov >= 0.5 * (ph_off - ph_on))


def transcribe(tokens, files, symbols, ignore=()):
    """[[phone id]] per token (file, onset, offset), and the set of (file, phone number) that belong to some token."""
    out, covered = [], set()
    for f, on, off in tokens:
        seq = []
        for k, (p_on, p_off, s) in enumerate(files[f]):
            if belongs(on, off, p_on, p_off) and s not in ignore:
                seq.append(symbols[s])
                covered.add((f, k))
        out.append(seq)
    return out, covered


def pairs(clusters):
    """[(token1, token2)], tokens numbered flat in cluster order: (cluster, first member, second member), without the
    pairs of one file that overlap in time."""
    out, base = [], 0
    for c in clusters:
        for a in range(len(c)):
            for b in range(a + 1, len(c)):
                (f1, on1, off1), (f2, on2, off2) = c[a], c[b]
                if not (f1 == f2 and min(off1, off2) > max(on1, on2)):
                    out.append((base + a, base + b))
        base += len(c)
    return out


def evaluate(clusters, files, symbols, ignore=()):
    """dict(ned, coverage, n_clusters, n_tokens, n_pairs, n_skipped, dist, max_len, token1, token2)."""
    flat = [t for c in clusters for t in c]
    trans, covered = transcribe(flat, files, symbols, ignore)
    dist, max_len, t1, t2, skipped = [], [], [], [], 0
    all_pairs = pairs(clusters)
    for a, b in all_pairs:
        if not trans[a] and not trans[b]:
            skipped += 1
            continue
        dist.append(levenshtein(trans[a], trans[b]))
        max_len.append(max(len(trans[a]), len(trans[b])))
        t1.append(a), t2.append(b)
    dist, max_len = np.array(dist, dtype=np.int32), np.array(max_len, dtype=np.int32)
    total = sum(1 for v in files.values() for _, _, s in v if s not in ignore)
    return dict(ned=float(np.mean(dist.astype(np.float64) / max_len.astype(np.float64))) if len(dist) else float('nan'),
                coverage=len(covered) / total if total else float('nan'), n_clusters=len(clusters), n_tokens=len(flat),
                n_pairs=len(all_pairs), n_skipped=skipped, dist=dist, max_len=max_len,
                token1=np.array(t1, dtype=np.int64), token2=np.array(t2, dtype=np.int64))


def synthetic(seed=0, n_files=20, alphabet=40, n_clusters=60):
    """(alignment lines, clusters, ignore): 20 files of 50-200 phones of 30-150 ms over 40 symbols (two of them
    'SIL' / 'NSN', ignored); clusters of 2-6 tokens of 0.1-0.9 s, some sharing a file and overlapping, about one in
    seven so short that it holds no phone."""
    rng = np.random.default_rng(seed)
    names = ['s%02d_utt%d' % (k % 7, k) for k in range(n_files)]
    symbols = ['SIL', 'NSN'] + ['p%02d' % k for k in range(alphabet - 2)]
    lines, ends = [], {}
    for f in names:
        t = round(float(rng.uniform(0, 0.2)), 3)
        for _ in range(int(rng.integers(50, 201))):
            d = round(float(rng.uniform(0.03, 0.15)), 3)
            lines.append('%s %r %r %s' % (f, t, round(t + d, 3), symbols[int(rng.integers(0, alphabet))]))
            t = round(t + d, 3)
        ends[f] = t
    rng.shuffle(lines)
    clusters = []
    for _ in range(n_clusters):
        c = []
        for k in range(int(rng.integers(2, 7))):
            if c and rng.random() < 0.25:                   # in the file of the previous token, overlapping it or not
                f = c[-1][0]
                on = max(0.0, c[-1][1] + float(rng.uniform(-0.3, 0.5)))
            else:
                f = names[int(rng.integers(0, n_files))]
                on = float(rng.uniform(0, ends[f] - 1.0))
            length = 0.01 if rng.random() < 0.15 else float(rng.uniform(0.1, 0.9))
            c.append((f, round(on, 4), round(on + length, 4)))
        clusters.append(c)
    return lines, clusters, ('SIL', 'NSN')
