"""Scoring discovered terms against a phone alignment: NED and coverage (ZeroSpeech track 2 / the TDE toolkit's first two
scores), the edit distances of all within-cluster pairs in one launch of the batched Levenshtein kernel
(csrc/edit.hip, abn_edit_distance_batched).

    python -m abnet3_amd.tde CLASSES ALIGNMENT [--ignore SIL ...]
    python -m abnet3_amd.tde ALIGNMENT --boundaries FILE.npz [--tolerance 0.02] [--ignore SIL ...]

The definition this module computes (tests/tde_np.py restates it with explicit loops; the two agree with ==):

* Alignment file: one ``file onset offset symbol`` line per phone, times in seconds, any line order.  The phones of a
  file are sorted by (onset, offset); their offsets must then be non-decreasing (phones that do not contain one another)
  -- ``read_alignment`` raises ValueError otherwise.  The symbols are numbered in sorted order.
* Classes file: ``Class k``, then one ``file onset offset`` line per token, then a blank line -- what
  terms.write_classes writes and SamplerCluster.parse_input_file reads.
* Inclusion rule (TDE's): with ov = min(token offset, phone offset) - max(token onset, phone onset) in float64, a phone
  belongs to a token when ov > 0 and (ov >= 0.03 or ov >= 0.5 * (phone offset - phone onset)): the token covers at least
  30 ms of the phone or at least half of it.  A token's transcription is the ids of its phones in time order, the
  symbols in `ignore` (silence, noise) left out.
* Pairs: every unordered pair of tokens inside a cluster, in the order (cluster, first member, second member); a pair
  whose two tokens lie in the same file and overlap in time (min of the offsets > max of the onsets) is left out.
  ``n_pairs`` counts the pairs that remain.  Of these, the pairs whose transcriptions are BOTH empty are skipped and
  counted in ``n_skipped``; the per-pair arrays hold the other n_pairs - n_skipped.
* NED of a pair: dist / max(len1, len2), dist the Levenshtein distance of the two transcriptions (unit costs).  ``ned``
  is np.mean over the pairs in that order of int32 distances divided as float64 -- nan when no pair is left.
* Coverage: the phones not in `ignore` that belong to at least one token, over all phones not in `ignore` (nan without
  any).  SIMPLIFICATION: TDE restricts the denominator to the "discoverable" phones (those inside some repeated n-gram
  of the gold transcription); this one counts every phone, so it reads lower than TDE's on the same clusters.
  TDE's matching, grouping, type and token scores are not computed.
* Boundary scores (``boundary_scores``, host only, float64): the standard phone-segmentation scores of a set of found
  boundaries -- ``unit_boundaries`` puts one midway between the two frames of each switch of unit, so a segmentation
  penalty (abnet3_amd/kmeans.py) can be judged against an alignment.  Gold boundaries are the phone onsets of a file
  except its first (an onset between two phones of `ignore` is none).  Both lists sorted, two pointers: |f - g| <=
  tolerance is a hit and both advance, otherwise the smaller advances.  precision = hits / found, recall = hits / gold,
  F their harmonic mean, OS = recall / precision - 1, R-value = 1 - (sqrt((1 - recall)^2 + OS^2) +
  |(-OS + recall - 1) / sqrt 2|) / 2; a ratio with an empty denominator is 0.
"""
import argparse
import sys
from collections import namedtuple

import numpy as np

MIN_OVERLAP = 0.03          # seconds of a phone a token must cover ...
MIN_SHARE = 0.5             # ... or this share of its duration


class Alignment(namedtuple('Alignment', ['names', 'first', 'onset', 'offset', 'ids', 'symbols'])):
    """names: the files, sorted; the phones of file f are rows first[f] .. first[f + 1] of onset / offset (float64) / ids
    (int32), sorted by (onset, offset); symbols: {symbol: id}, ids in sorted symbol order."""
    __slots__ = ()

    def file(self, name):
        """(onset, offset, ids) of one file's phones."""
        f = self.names.index(_text(name))
        return tuple(a[self.first[f]:self.first[f + 1]] for a in (self.onset, self.offset, self.ids))


TermScores = namedtuple('TermScores', ['ned', 'coverage', 'n_clusters', 'n_tokens', 'n_pairs', 'n_skipped', 'dist', 'max_len',
                                       'token1', 'token2'])
TermScores.__doc__ = """evaluate()'s result: ned, coverage, the counts, and per scored pair dist (int32), max_len (int32)
and the token numbers of its two sides (tokens numbered in cluster order) -- for within- / across-speaker splits."""


def _text(name):
    return name.decode('UTF-8') if isinstance(name, bytes) else str(name)


def edit_distance_batch(sym1, off1, n1, sym2, off2, n2, max_short=None):
    """int32 device tensor: the Levenshtein distance of sym1[off1[p] .. off1[p]+n1[p]) and sym2[off2[p] .. +n2[p]) per
    pair p (abn_edit_distance_batched).  sym*: int32 symbol tables, off*: int64, n*: int32 -- device tensors, or host
    arrays, which are uploaded.  The pairs are sorted by (shorter length, longer length) for the launch -- the lanes of a
    wavefront run as long as their longest pair -- and the result is put back in the caller's order.
    max_short (1 .. abn_edit_max_short()): the longest SHORTER side; None derives it from the lengths when they are host
    arrays, and takes the cap otherwise.  A pair beyond it, with a negative length or outside its table comes back as -1:
    nothing is raised here (TermEvaluator, which builds its own table, does raise)."""
    import torch
    from . import _lib
    lib = _lib.load()
    cap = int(lib.abn_edit_max_short())
    host_n = None if any(isinstance(a, torch.Tensor) for a in (n1, n2)) else (np.asarray(n1), np.asarray(n2))

    def up(a, dt):
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype={torch.int32: np.int32, torch.int64: np.int64}[dt])).cuda()
        if a.dtype != dt or a.dim() != 1:
            raise ValueError('edit_distance_batch: a 1-d %s tensor is needed, not %s %s' % (dt, a.dtype, tuple(a.shape)))
        a = a.contiguous()
        _lib.require_device(a)
        return a
    same = sym2 is sym1
    sym1 = up(sym1, torch.int32)
    sym2 = sym1 if same else up(sym2, torch.int32)
    off1, n1, off2, n2 = up(off1, torch.int64), up(n1, torch.int32), up(off2, torch.int64), up(n2, torch.int32)
    P = n1.numel()
    if not (off1.numel() == off2.numel() == n2.numel() == P):
        raise ValueError('edit_distance_batch: the pair table\'s columns differ in length')
    if max_short is None:
        max_short = cap
        if host_n is not None and P:
            max_short = int(min(cap, max(1, np.minimum(host_n[0], host_n[1]).max())))
    max_short = int(max_short)
    if not 1 <= max_short <= cap:
        raise ValueError('edit_distance_batch: max_short must lie in 1 .. %d, not %d' % (cap, max_short))
    dist = torch.empty(P, dtype=torch.int32, device=n1.device)
    if P:
        lo, hi = torch.minimum(n1, n2).to(torch.int64), torch.maximum(n1, n2).to(torch.int64)
        order = torch.argsort((lo << 32) + hi.clamp_(min=0))
        cols = [c[order].contiguous() for c in (off1, n1, off2, n2)]
        out = torch.empty_like(dist)
        _lib.check(lib.abn_edit_distance_batched(_lib.ptr(sym1), sym1.numel(), _lib.ptr(sym2), sym2.numel(),
                                                 *[_lib.ptr(c) for c in cols], P, max_short, _lib.ptr(out), _lib.stream()),
                   'abn_edit_distance_batched')
        dist[order] = out
    return dist


# ---------------------------------------------------------------------------------------------------------------
# host side: the file formats, transcription, pair table, scores (numpy; tests/test_tde_host.py runs it without a GPU)

def read_alignment(path):
    """The Alignment of a ``file onset offset symbol`` file (module docstring)."""
    files, on, off, sym = [], [], [], []
    with open(path, 'r', encoding='utf-8') as fh:
        for ln, line in enumerate(fh, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 4:
                raise ValueError('%s:%d: expected "file onset offset symbol", got %r' % (path, ln, line.rstrip('\n')))
            files.append(parts[0]), on.append(float(parts[1])), off.append(float(parts[2])), sym.append(parts[3])
    return make_alignment(files, on, off, sym)


def make_alignment(files, onset, offset, symbol):
    """The Alignment of parallel per-phone sequences (file name, onset, offset, symbol), in any order."""
    files, symbol = np.asarray([_text(f) for f in files], dtype=object), np.asarray(symbol, dtype=object)
    onset, offset = np.asarray(onset, dtype=np.float64), np.asarray(offset, dtype=np.float64)
    names, fnum = np.unique(files.astype(str), return_inverse=True)
    vocab, ids = np.unique(symbol.astype(str), return_inverse=True)
    if (offset < onset).any():
        k = int(np.flatnonzero(offset < onset)[0])
        raise ValueError('alignment: phone %s %r %r ends before it starts' % (files[k], onset[k], offset[k]))
    order = np.lexsort((offset, onset, fnum))
    fnum, onset, offset, ids = fnum[order], onset[order], offset[order], ids[order].astype(np.int32)
    first = np.searchsorted(fnum, np.arange(len(names) + 1)).astype(np.int64)
    back = np.flatnonzero((fnum[1:] == fnum[:-1]) & (offset[1:] < offset[:-1]))
    if len(back):
        k = int(back[0])
        raise ValueError('alignment: in %s the phone at %r lies inside the phone at %r' % (names[fnum[k]], onset[k + 1], onset[k]))
    return Alignment([str(n) for n in names], first, onset, offset, ids, {str(s): k for k, s in enumerate(vocab)})


def read_classes(path):
    """[[(file, onset, offset)]]: the clusters of a .classes file (module docstring)."""
    clusters, cur = [], None
    with open(path, 'r', encoding='utf-8') as fh:
        for ln, line in enumerate(fh, 1):
            parts = line.split()
            if not parts:
                cur = None
            elif len(parts) == 2 and parts[0] == 'Class':
                cur = []
                clusters.append(cur)
            elif len(parts) == 3 and cur is not None:
                cur.append((parts[0], float(parts[1]), float(parts[2])))
            else:
                raise ValueError('%s:%d: expected "Class k", "file onset offset" or a blank line, got %r' % (path, ln, line.rstrip('\n')))
    return clusters


def _ignored(alignment, ignore):
    """bool per symbol id: it is in `ignore`."""
    out = np.zeros(len(alignment.symbols), dtype=bool)
    for s in ignore:
        if _text(s) in alignment.symbols:
            out[alignment.symbols[_text(s)]] = True
    return out


def _belongs(tokens, alignment):
    """(token number, phone row) of every phone that belongs to a token by the inclusion rule, by token then time."""
    number = {n: f for f, n in enumerate(alignment.names)}
    T = len(tokens)
    tf = np.empty(T, dtype=np.int64)
    for k, tok in enumerate(tokens):
        f = number.get(_text(tok[0]))
        if f is None:
            raise ValueError('token %d lies in file %r, which the alignment does not hold' % (k, _text(tok[0])))
        tf[k] = f
    t_on = np.array([tok[1] for tok in tokens], dtype=np.float64)
    t_off = np.array([tok[2] for tok in tokens], dtype=np.float64)
    lo, hi = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    for f in np.unique(tf):                                # per FILE: phones that end after the onset and start before the offset
        sel, a, b = np.flatnonzero(tf == f), alignment.first[f], alignment.first[f + 1]
        lo[sel] = a + np.searchsorted(alignment.offset[a:b], t_on[sel], side='right')
        hi[sel] = a + np.searchsorted(alignment.onset[a:b], t_off[sel], side='left')
    cnt = np.maximum(hi - lo, 0)
    tok = np.repeat(np.arange(T), cnt)
    ph = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    ov = np.minimum(t_off[tok], alignment.offset[ph]) - np.maximum(t_on[tok], alignment.onset[ph])
    keep = (ov > 0) & ((ov >= MIN_OVERLAP) | (ov >= MIN_SHARE * (alignment.offset[ph] - alignment.onset[ph])))
    return tok[keep], ph[keep]


def transcribe(tokens, alignment, ignore=()):
    """(table int32, tok_off int64, tok_n int32): the phone-id sequence of token k = (file, onset, offset) is
    table[tok_off[k] .. tok_off[k] + tok_n[k]) (module docstring: the inclusion rule, `ignore`)."""
    tok, ph = _belongs(tokens, alignment)
    keep = ~_ignored(alignment, ignore)[alignment.ids[ph]]
    return _table(len(tokens), tok[keep], alignment.ids[ph[keep]])


def _table(T, tok, ids):
    tok_n = np.bincount(tok, minlength=T).astype(np.int32)
    return ids.astype(np.int32), (np.cumsum(tok_n, dtype=np.int64) - tok_n), tok_n


def cluster_pairs(clusters):
    """(token1, token2) int64: every unordered pair inside a cluster, tokens numbered flat in cluster order, pairs in
    the order (cluster, first member, second member); the same-file overlap rule is pair_table's."""
    size = np.array([len(c) for c in clusters], dtype=np.int64)
    start = np.cumsum(size) - size
    pos = np.arange(size.sum()) - np.repeat(start, size)            # a token's place inside its cluster
    later = np.repeat(size, size) - 1 - pos                         # how many tokens of its cluster follow it
    t1 = np.repeat(np.arange(size.sum()), later)
    t2 = np.arange(later.sum()) - np.repeat(np.cumsum(later) - later, later) + t1 + 1
    return t1, t2


def pair_table(clusters):
    """cluster_pairs without the pairs whose two tokens lie in the same file and overlap in time; clusters of
    (file, onset, offset) tokens."""
    t1, t2 = cluster_pairs(clusters)
    flat = [tok for c in clusters for tok in c]
    _, fnum = np.unique(np.array([_text(t[0]) for t in flat], dtype=str), return_inverse=True)
    on, off = np.array([t[1] for t in flat], dtype=np.float64), np.array([t[2] for t in flat], dtype=np.float64)
    overlap = (fnum[t1] == fnum[t2]) & (np.minimum(off[t1], off[t2]) > np.maximum(on[t1], on[t2]))
    return t1[~overlap], t2[~overlap]


def tokens_of(clusters, names, times):
    """TermDiscoverer.clusters ((file number, first frame, last frame) tokens) as (file, onset, offset) clusters: the times
    of the first and the last frame, as terms.write_classes prints them."""
    return [[(_text(names[f]), float(times[names[f]][lo]), float(times[names[f]][hi])) for f, lo, hi in c] for c in clusters]


class TermEvaluator(object):
    """NED and coverage of term clusters against `alignment` (an Alignment or the path of an alignment file); `ignore`:
    symbols left out of transcriptions and of the coverage denominator (module docstring)."""

    def __init__(self, alignment, ignore=()):
        self.alignment = read_alignment(alignment) if isinstance(alignment, str) else alignment
        self.ignore = tuple(_text(s) for s in ignore)

    def prepare(self, classes, names=None, times=None):
        """The host half of evaluate(): (flat tokens, (table, tok_off, tok_n), (token1, token2) of the scored pairs,
        n_pairs, n_skipped, coverage)."""
        if isinstance(classes, str):
            classes = read_classes(classes)
        elif names is not None:
            if times is None:
                raise ValueError('TermEvaluator: clusters of frame tokens need `names` and `times`')
            classes = tokens_of(classes, names, times)
        a = self.alignment
        flat = [tok for c in classes for tok in c]
        tok, ph = _belongs(flat, a)
        real = ~_ignored(a, self.ignore)
        keep = real[a.ids[ph]]
        total = int(real[a.ids].sum())
        coverage = len(np.unique(ph[keep])) / total if total else float('nan')
        trans = _table(len(flat), tok[keep], a.ids[ph[keep]])
        t1, t2 = pair_table(classes)
        scored = (trans[2][t1] > 0) | (trans[2][t2] > 0)
        return classes, flat, trans, (t1[scored], t2[scored]), len(t1), int((~scored).sum()), coverage

    def evaluate(self, classes, names=None, times=None):
        """TermScores of `classes`: the path of a .classes file, clusters of (file, onset, offset) tokens, or
        TermDiscoverer.clusters together with its `names` and `corpus.times`."""
        classes, flat, (table, tok_off, tok_n), (t1, t2), n_pairs, n_skipped, coverage = self.prepare(classes, names, times)
        if len(t1):
            dist = edit_distance_batch(table, tok_off[t1], tok_n[t1], table, tok_off[t2], tok_n[t2]).cpu().numpy()
            if (dist < 0).any():
                from . import _lib
                raise RuntimeError('the edit-distance kernel refused %d pairs of a table this module built (both transcriptions '
                                   'longer than %d phones?)' % (int((dist < 0).sum()), _lib.EDIT_MAX_SHORT))
        else:
            dist = np.zeros(0, dtype=np.int32)
        max_len = np.maximum(tok_n[t1], tok_n[t2])
        return TermScores(ned(dist, max_len), coverage, len(classes), len(flat), n_pairs, n_skipped, dist, max_len, t1, t2)


def ned(dist, max_len):
    """np.mean of dist / max_len in float64 (nan for no pair)."""
    if not len(dist):
        return float('nan')
    return float(np.mean(np.asarray(dist).astype(np.float64) / np.asarray(max_len).astype(np.float64)))


BoundaryScores = namedtuple('BoundaryScores', ['precision', 'recall', 'f', 'os', 'r_value', 'n_found', 'n_gold', 'n_hit'])
BoundaryScores.__doc__ = """boundary_scores()'s result: precision, recall, F, the over-segmentation OS = recall / precision - 1
and the R-value 1 - (sqrt((1 - recall)^2 + OS^2) + |(-OS + recall - 1) / sqrt 2|) / 2, with the three counts."""


def unit_boundaries(ids_by_name, times):
    """{file: float64 boundary times}: one boundary midway between the two frames of each switch of unit, the BAD
    frames (id < 0) left out first.  times: {file: [T] frame times in seconds}."""
    out = {}
    for k, ids in ids_by_name.items():
        a = np.asarray(ids).astype(np.int64).ravel()
        t = np.asarray(times[k], dtype=np.float64).ravel()
        if len(t) != len(a):
            raise ValueError('unit_boundaries: %r has %d ids and %d times' % (k, len(a), len(t)))
        t, a = t[a >= 0], a[a >= 0]
        sw = np.flatnonzero(a[1:] != a[:-1])
        out[_text(k)] = 0.5 * (t[sw] + t[sw + 1])
    return out


def gold_boundaries(alignment, ignore=()):
    """{file: float64 times}: the phone onsets of each file except its first; an onset between two phones that are both in
    `ignore` (silence, noise) is no boundary."""
    if isinstance(alignment, str):
        alignment = read_alignment(alignment)
    ign = _ignored(alignment, ignore)[alignment.ids] if len(alignment.ids) else np.zeros(0, dtype=bool)
    out = {}
    for f, name in enumerate(alignment.names):
        a, b = int(alignment.first[f]), int(alignment.first[f + 1])
        keep = ~(ign[a + 1:b] & ign[a:b - 1]) if b - a > 1 else np.zeros(0, dtype=bool)
        out[name] = alignment.onset[a + 1:b][keep]
    return out


def boundary_scores(found, alignment, tolerance=0.02, ignore=()):
    """The standard phone-segmentation scores of `found` = {file: boundary times} against an Alignment (or the path of
    one), host only, float64.  Per file of the alignment both lists are sorted and walked with two pointers:
    |f - g| <= tolerance counts a hit and advances both, otherwise the smaller advances.  A file that `found` lacks has
    no found boundary; a file the alignment lacks is a ValueError.  Empty sides give 0 for the ratios they define."""
    gold = gold_boundaries(alignment, ignore)
    found = {_text(k): v for k, v in found.items()}
    for k in found:
        if k not in gold:
            raise ValueError('boundary_scores: file %r is not in the alignment' % k)
    tolerance = float(tolerance)
    hits = n_found = n_gold = 0
    for name, g in gold.items():
        f = np.sort(np.asarray(found.get(name, ()), dtype=np.float64).ravel())
        g = np.sort(g)
        n_found, n_gold = n_found + len(f), n_gold + len(g)
        i = j = 0
        while i < len(f) and j < len(g):
            if abs(f[i] - g[j]) <= tolerance:
                hits, i, j = hits + 1, i + 1, j + 1
            elif f[i] < g[j]:
                i += 1
            else:
                j += 1
    prec = hits / n_found if n_found else 0.0
    rec = hits / n_gold if n_gold else 0.0
    fsc = 2.0 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0
    osg = rec / prec - 1.0 if prec > 0 else 0.0
    r1 = float(np.sqrt((1.0 - rec) ** 2 + osg ** 2))
    r2 = abs((-osg + rec - 1.0) / float(np.sqrt(2.0)))
    return BoundaryScores(prec, rec, fsc, osg, 1.0 - (r1 + r2) / 2.0, n_found, n_gold, hits)


def summary(s):
    """The one line the command line and examples/zero_resource.py print."""
    return 'NED %.4f coverage %.4f (%d clusters, %d tokens, %d pairs, %d skipped)' % (s.ned, s.coverage, s.n_clusters, s.n_tokens,
                                                                                     s.n_pairs, s.n_skipped)


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m abnet3_amd.tde', description='NED and coverage of a .classes file against a phone alignment')
    ap.add_argument('classes', nargs='?', default=None, help='.classes file (terms.write_classes)')
    ap.add_argument('alignment', help='phone alignment: "file onset offset symbol" lines')
    ap.add_argument('--ignore', nargs='*', default=[], metavar='SYMBOL', help='symbols that are no phones (silence, noise)')
    ap.add_argument('--boundaries', default=None, metavar='FILE.npz', help='an .npz of file -> boundary times: the boundary scores')
    ap.add_argument('--tolerance', type=float, default=0.02, help='seconds within which a found boundary hits a gold one')
    args = ap.parse_args(argv)
    if args.classes is None and args.boundaries is None:
        ap.error('a .classes file or --boundaries is needed')
    if args.classes is not None:
        print(summary(TermEvaluator(args.alignment, ignore=args.ignore).evaluate(args.classes)))
    if args.boundaries is not None:
        with np.load(args.boundaries) as z:
            found = {k: z[k] for k in z.files}
        b = boundary_scores(found, read_alignment(args.alignment), args.tolerance, args.ignore)
        print('boundaries: precision %.4f recall %.4f F %.4f OS %.4f R-value %.4f (%d found, %d gold, %d hits, tolerance %g s)'
              % (b.precision, b.recall, b.f, b.os, b.r_value, b.n_found, b.n_gold, b.n_hit, args.tolerance))
    return 0


if __name__ == '__main__':
    sys.exit(main())
