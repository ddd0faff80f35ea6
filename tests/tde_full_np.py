"""The full term scores abnet3_amd/tde.py computes (evaluate_full), restated with explicit loops over tests/tde_np.py: snapping
phone by phone, the gold words, the sets F and G with their types and edges, the pair histogram pair by pair from
tde_np.pairs and tde_np.levenshtein, |S| by a double loop over all token pairs, NED as an exact Fraction.  Standard library,
numpy and tde_np only: nothing of the package is imported.  Also the word alignment and the extra clusters that extend
tde_np.synthetic, and the token tables the GPU tests feed to the kernel."""
from fractions import Fraction

import numpy as np

import tde_np


def snap(token, files, symbols, ignore=()):
    """((file, lo, hi), [phone id]) of a (file, onset, offset) token: the file-local rows of its first and last phone that
    belongs to it and is not ignored, and its transcription; (None, []) for an empty token."""
    f, on, off = token
    rows = [k for k, (p_on, p_off, s) in enumerate(files[f]) if tde_np.belongs(on, off, p_on, p_off) and s not in ignore]
    if not rows:
        return None, []
    return (f, rows[0], rows[-1]), [symbols[files[f][k][2]] for k in rows]


def edges(spans):
    out = set()
    for f, lo, hi in spans:
        out.add((f, lo))
        out.add((f, hi + 1))
    return out


def prf(hit, found, gold):
    p = hit / found if found else 0.0
    r = hit / gold if gold else 0.0
    return p, r, (2.0 * p * r / (p + r) if p + r > 0 else 0.0)


def gold(word_files, files, symbols, ignore=(), ignore_words=None):
    """dict(spans, lexicon, boundaries, n_gold, n_gold_empty) of a parsed word alignment ({file: [(onset, offset, word)]})."""
    ignore_words = ignore if ignore_words is None else ignore_words
    spans, lexicon, n, n_empty = set(), set(), 0, 0
    for f in sorted(word_files):
        for on, off, w in word_files[f]:
            if w in ignore_words:
                continue
            n += 1
            span, seq = snap((f, on, off), files, symbols, ignore)
            if span is None:
                n_empty += 1
            else:
                spans.add(span)
                lexicon.add(tuple(seq))
    return dict(spans=spans, lexicon=lexicon, boundaries=edges(spans), n_gold=n, n_gold_empty=n_empty)


def overlap(a, b):
    return a[0] == b[0] and min(a[2], b[2]) > max(a[1], b[1])


def histogram(clusters, trans, groups=None):
    """(hist [2][M + 1][M + 1] int64, n_pairs, n_skipped) pair by pair; trans: the flat tokens' transcriptions."""
    M = max([1] + [len(t) for t in trans])
    hist = np.zeros((2, M + 1, M + 1), dtype=np.int64)
    all_pairs = tde_np.pairs(clusters)
    skipped = 0
    for a, b in all_pairs:
        if not trans[a] and not trans[b]:
            skipped += 1
            continue
        g = 0 if groups is None or groups[a] == groups[b] else 1
        hist[g][tde_np.levenshtein(trans[a], trans[b])][max(len(trans[a]), len(trans[b]))] += 1
    return hist, len(all_pairs), skipped


def same_type_pairs(flat, trans):
    """|S| by the double loop: admissible pairs of any clusters with identical non-empty transcriptions."""
    n = 0
    for i in range(len(flat)):
        for j in range(i + 1, len(flat)):
            if trans[i] and trans[i] == trans[j] and not overlap(flat[i], flat[j]):
                n += 1
    return n


def ned_of(hist):
    total, num = 0, Fraction(0)
    for g in range(hist.shape[0]):
        for d in range(hist.shape[1]):
            for L in range(hist.shape[2]):
                if hist[g][d][L]:
                    total += int(hist[g][d][L])
                    num += Fraction(int(hist[g][d][L]) * d, L)
    return float(num / total) if total else float('nan')


def evaluate_full(clusters, files, symbols, ignore=(), word_files=None, ignore_words=None, speakers=None):
    """dict with FullTermScores' fields; speakers: {file: speaker} or None."""
    flat = [t for c in clusters for t in c]
    snapped = [snap(t, files, symbols, ignore) for t in flat]
    trans = [seq for _, seq in snapped]
    groups = None if speakers is None else [speakers[t[0]] for t in flat]
    hist, n_pairs, n_skipped = histogram(clusters, trans, groups)
    n_same = same_type_pairs(flat, trans)
    covered = tde_np.transcribe(flat, files, symbols, ignore)[1]
    total = sum(1 for v in files.values() for _, _, s in v if s not in ignore)
    F = {span for span, _ in snapped if span is not None}
    types = {tuple(seq) for _, seq in snapped if seq}
    out = dict(ned=ned_of(hist), ned_within=ned_of(hist[0:1]), ned_across=ned_of(hist[1:2]),
               coverage=len(covered) / total if total else float('nan'), token=None, type=None, boundary=None,
               grouping=prf(int(hist[:, 0, :].sum()), int(hist.sum()), n_same), n_clusters=len(clusters), n_tokens=len(flat),
               n_empty=sum(1 for span, _ in snapped if span is None), n_gold=0, n_gold_empty=0, n_pairs=n_pairs, n_skipped=n_skipped,
               n_same=n_same, hist=hist)
    if word_files is not None:
        g = gold(word_files, files, symbols, ignore, ignore_words)
        out.update(token=prf(len(F & g['spans']), len(F), len(g['spans'])), type=prf(len(types & g['lexicon']), len(types), len(g['lexicon'])),
                   boundary=prf(len(edges(F) & g['boundaries']), len(edges(F)), len(g['boundaries'])), n_gold=g['n_gold'],
                   n_gold_empty=g['n_gold_empty'])
    return out


# ----------------------------------------------------------------------------------------------------------------------
# corpora
# ----------------------------------------------------------------------------------------------------------------------
def synthetic_words(lines, clusters, seed=0):
    """(word alignment lines, clusters): tde_np.synthetic's phones grouped into words of 1 - 4 phones (about one in eight an
    ignored 'SIL' word, one in twenty so short that it holds no phone), and its clusters extended by clusters of gold word
    intervals grouped by their first phone -- so that the token, type, boundary and grouping scores are not all zero."""
    rng = np.random.default_rng(seed + 1000)
    files, _ = tde_np.parse_alignment(lines)
    word_lines, by_first = [], {}
    for f in sorted(files):
        k, phones = 0, files[f]
        while k < len(phones):
            n = int(rng.integers(1, 5))
            on, off = phones[k][0], phones[min(k + n, len(phones)) - 1][1]
            u = rng.random()
            if u < 0.05:
                off = round(on + 0.001, 4)
            word = 'SIL' if u > 0.875 else 'w%d' % int(rng.integers(0, 30))
            word_lines.append('%s %r %r %s' % (f, on, off, word))
            if 0.05 <= u <= 0.875:
                by_first.setdefault(phones[k][2], []).append((f, on, off))
            k += n
    rng.shuffle(word_lines)
    extra = [v[:6] for _, v in sorted(by_first.items()) if len(v) >= 2][:15]
    return word_lines, list(clusters) + extra


def speakers_of(files):
    """tde_np.synthetic names its files sNN_uttK: the speaker is the part before the underscore."""
    return {f: f.split('_')[0] for f in files}


def token_table(rng, sizes, lengths, alphabet, n_files=3, n_groups=2, p_overlap=0.2, p_copy=0.3):
    """A table of tokens for the kernel: clusters of the given sizes; every token draws its length from `lengths` and is,
    with probability p_copy, a copy of the previous token with one symbol changed (small distances), otherwise random;
    with probability p_overlap it lies in the previous token's file and overlaps it in time.  Returns dict(table, tok_off,
    tok_n, tok_file, tok_on, tok_end, groups, cl_first) of numpy arrays in the kernel's dtypes."""
    seqs, tf, on, end, grp = [], [], [], [], []
    for s in sizes:
        for k in range(s):
            n = int(lengths[int(rng.integers(0, len(lengths)))])
            if k and rng.random() < p_copy and len(seqs[-1]) == n and n:
                seq = list(seqs[-1])
                seq[int(rng.integers(0, n))] = int(rng.integers(0, alphabet))
            else:
                seq = rng.integers(0, alphabet, n).tolist()
            seqs.append(seq)
            if k and rng.random() < p_overlap:
                tf.append(tf[-1])
                on.append(on[-1] + 0.1)
            else:
                tf.append(int(rng.integers(0, n_files)))
                on.append(float(rng.uniform(0, 100)))
            end.append(on[-1] + (0.0 if rng.random() < 0.05 else 0.3))
            grp.append(int(rng.integers(0, n_groups)))
    tok_n = np.array([len(q) for q in seqs], dtype=np.int32)
    return dict(table=np.array([x for q in seqs for x in q], dtype=np.int32), tok_off=(np.cumsum(tok_n, dtype=np.int64) - tok_n),
                tok_n=tok_n, tok_file=np.array(tf, dtype=np.int32), tok_on=np.array(on, dtype=np.float64),
                tok_end=np.array(end, dtype=np.float64), groups=np.array(grp, dtype=np.int32),
                cl_first=np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64))


def levenshtein_many(A, B):
    """tde_np.levenshtein_rows for P pairs at once: A [P, la], B [P, lb] -> [P] distances (tests/test_tde_full_host.py holds
    it against tde_np.levenshtein)."""
    A, B = np.asarray(A, dtype=np.int64), np.asarray(B, dtype=np.int64)
    ramp = np.arange(B.shape[1] + 1, dtype=np.int64)
    prev = np.tile(ramp, (A.shape[0], 1))
    for i in range(1, A.shape[1] + 1):
        cur = np.empty_like(prev)
        cur[:, 0] = i
        cur[:, 1:] = np.minimum(prev[:, 1:] + 1, prev[:, :-1] + (B != A[:, i - 1:i]))
        prev = np.minimum.accumulate(cur - ramp, axis=1) + ramp
    return prev[:, -1]


def table_histogram(t, use_groups=True):
    """(hist, n_pairs, n_skipped) of a token_table: the pairs listed by the loops above, then the distances of all pairs of
    one pair of lengths in one levenshtein_many."""
    seqs = [t['table'][o:o + n].astype(np.int64) for o, n in zip(t['tok_off'], t['tok_n'])]
    M = max([1] + [len(q) for q in seqs])
    hist = np.zeros((2, M + 1, M + 1), dtype=np.int64)
    n_pairs = n_skipped = 0
    by_lengths = {}
    first, tf, on, end = t['cl_first'].tolist(), t['tok_file'].tolist(), t['tok_on'].tolist(), t['tok_end'].tolist()
    for c in range(len(first) - 1):
        for a in range(first[c], first[c + 1]):
            for b in range(a + 1, first[c + 1]):
                if tf[a] == tf[b] and min(end[a], end[b]) > max(on[a], on[b]):
                    continue
                n_pairs += 1
                if not len(seqs[a]) and not len(seqs[b]):
                    n_skipped += 1
                    continue
                by_lengths.setdefault((len(seqs[a]), len(seqs[b])), []).append((a, b))
    for (la, lb), ab in by_lengths.items():
        d = levenshtein_many(np.stack([seqs[a] for a, _ in ab]), np.stack([seqs[b] for _, b in ab]))
        g = np.array([1 if use_groups and t['groups'][a] != t['groups'][b] else 0 for a, b in ab])
        np.add.at(hist, (g, d, max(la, lb)), 1)
    return hist, n_pairs, n_skipped
