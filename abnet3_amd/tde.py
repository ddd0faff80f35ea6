"""Scoring discovered terms against a phone alignment: NED and coverage (ZeroSpeech track 2 / the TDE toolkit's first two
scores), the edit distances of all within-cluster pairs in one launch of the batched Levenshtein kernel
(csrc/edit.hip, abn_edit_distance_batched); and the rest of the tdev2 score set -- token, type, boundary, grouping, NED
within / across speaker -- from one launch of a kernel that enumerates the pairs itself and returns a histogram
(csrc/edit_hist.hip, abns_edit_cluster_hist).

    python -m abnet3_amd.tde CLASSES ALIGNMENT [--ignore SIL ...]
    python -m abnet3_amd.tde CLASSES ALIGNMENT --full [--words WORD_ALIGNMENT] [--speakers FILE] [--ignore SIL ...]
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
  The token, type, boundary and grouping scores and NED within / across speaker are ``evaluate_full``'s (below); TDE's
  matching score is left out (tdev2 dropped it too).
* The full score set (``TermEvaluator.evaluate_full``; tests/tde_full_np.py restates it with explicit loops, the counts
  agree with ==).  Everything is decided in phone-row index space.  snap(file, onset, offset): the phones that belong to
  the interval by the inclusion rule and are not in `ignore`; none: the token is EMPTY; otherwise its span is
  (file, lo, hi), the file-local rows of the first and the last such phone, and its transcription is ``transcribe``'s.
  Gold: every row of the word alignment (the same file format, the symbols are words) whose symbol is not in
  `ignore_words` is snapped -- ``n_gold`` rows, ``n_gold_empty`` of them empty; G = the distinct gold spans, lexicon =
  the distinct transcriptions of the non-empty gold rows, B_G = {(file, lo), (file, hi + 1)} over G (edge k of a file
  lies in front of its phone row k).  Found: the flat tokens of all clusters snapped likewise (``n_empty``), F, types(F),
  B_F.  token = |F n G| over |F| and over |G|; type (Ludusan et al. 2014, string level) = |types(F) n lexicon| over
  |types(F)| and over |lexicon|; boundary = |B_F n B_G| over |B_F| and over |B_G| (an exact match after snapping; the
  tolerance-based ``boundary_scores`` below is another score).  Each is (precision, recall, F = harmonic mean); a ratio
  with an empty denominator is 0.
  A pair of flat tokens i < j is ADMISSIBLE unless the two lie in the same file and overlap in time (the rule above, on
  the float64 times) or both transcriptions are empty.  C = the admissible pairs inside one cluster (the pairs
  ``evaluate`` scores), S = the admissible pairs in any clusters with identical non-empty transcriptions.
  ``hist[g][d][L]`` (int64, [2][M + 1][M + 1], M the longest transcription, at most 256 on this route) counts the pairs
  of C with Levenshtein distance d and L = max(len1, len2); g = 0 when the two tokens' speakers are equal (all equal
  when none are given), else 1.  It comes from ONE launch that enumerates the pairs itself (csrc/edit_hist.hip,
  abns_edit_cluster_hist): no per-pair array exists on the host or on the device.  NED = sum hist d / L over sum hist as
  an exact Fraction rounded once (nan for no pair); ``ned_within`` from hist[0], ``ned_across`` from hist[1].
  grouping (pair counting) = |C n S| / |C| and |C n S| / |S| with |C| = sum hist, |C n S| = sum_L hist[.][0][L] and
  ``n_same`` = |S| counted on the host per transcription type: C(m, 2) minus the same-file overlapping pairs of the type.
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
from fractions import Fraction

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

FullTermScores = namedtuple('FullTermScores', ['ned', 'ned_within', 'ned_across', 'coverage', 'token', 'type', 'boundary', 'grouping',
                                               'n_clusters', 'n_tokens', 'n_empty', 'n_gold', 'n_gold_empty', 'n_pairs', 'n_skipped',
                                               'n_same', 'hist'])
FullTermScores.__doc__ = """evaluate_full()'s result (module docstring): the three NEDs and coverage; token, type, boundary and
grouping, each (precision, recall, F) -- the first three None without a word alignment; the counts (n_gold: the gold rows
snapped, n_same: |S|) and hist, the int64 [2][M + 1][M + 1] pair histogram everything pair-wise is derived from."""

GoldWords = namedtuple('GoldWords', ['spans', 'lexicon', 'boundaries', 'n_gold', 'n_gold_empty'])
GoldWords.__doc__ = """gold_words()'s result: the sets G of (file number, lo, hi) spans, of transcriptions (tuples of phone ids)
and of (file number, edge) boundaries, the number of gold rows snapped and how many of them were empty."""

Snapped = namedtuple('Snapped', ['table', 'tok_off', 'tok_n', 'file', 'lo', 'hi'])
Snapped.__doc__ = """snap_tokens()'s result: transcribe()'s three arrays, and per token the alignment's file number and the
file-local rows of its first and last phone (all three -1 for an empty token)."""


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


def cluster_histogram(table, tok_off, tok_n, tok_file, tok_on, tok_end, cl_first, groups=None):
    """(hist, n_pairs, n_skipped): the pair histogram of the module docstring from ONE launch that enumerates the pairs itself
    (abns_edit_cluster_hist) -- hist int64 numpy [2][M + 1][M + 1] with M = max(1, the longest tok_n), n_pairs the
    same-cluster pairs that pass the overlap rule, n_skipped those of them with two empty sides.
    table: int32 symbol table; token t, flat in cluster order, is table[tok_off[t] .. tok_off[t] + tok_n[t]) (tok_off int64,
    tok_n int32) in file tok_file[t] (int32) from tok_on[t] to tok_end[t] (float64 seconds) with speaker groups[t] (int32;
    None: one speaker); cluster c holds the tokens cl_first[c] .. cl_first[c + 1] (int64, [n_clusters + 1], read on the HOST:
    a tensor is copied down).  The other arguments are device tensors of exactly these dtypes, taken as they are (a strided
    view is made contiguous), or host arrays / lists, which are converted and uploaded; a wider device dtype, a rank other
    than 1, columns of unequal length, a cl_first that does not run from 0 to the number of tokens or decreases, and M
    beyond abns_edit_hist_max_len() are ValueErrors before anything is launched.  A token that leaves the table makes the
    call fail (HipLibraryError).  The tokens of a cluster are reordered by length for the launch, so that the lanes of a
    wavefront meet pairs of similar length; the histogram does not depend on any order."""
    import torch
    from . import _lib
    who = 'cluster_histogram'
    lib = _lib.load()
    cap = int(lib.abns_edit_hist_max_len())
    host_dtype = {torch.int32: np.int32, torch.int64: np.int64, torch.float64: np.float64}

    def host(what, a, dt):
        arr = np.asarray(a)
        kinds = 'fiu' if dt == torch.float64 else 'iu'
        if arr.ndim != 1 or (arr.size and arr.dtype.kind not in kinds):
            raise ValueError('%s: %s must be a 1-d array of %s, not %s %s' % (who, what, str(dt).replace('torch.', ''), arr.shape, arr.dtype))
        conv = np.ascontiguousarray(arr, dtype=host_dtype[dt])
        if arr.size and not np.array_equal(conv, arr):
            raise ValueError('%s: %s does not fit %s' % (who, what, str(dt).replace('torch.', '')))
        return conv

    def column(what, a, dt):
        if not isinstance(a, torch.Tensor):
            return torch.from_numpy(host(what, a, dt)).cuda()
        if a.dim() == 1 and a.dtype == dt:
            a = a.contiguous()
        _lib.require_tensor(who, what, a, dt, 1)
        return a
    n_host = None if isinstance(tok_n, torch.Tensor) else host('tok_n', tok_n, torch.int32)
    table = column('table', table, torch.int32)
    cols = [column(what, a, dt) for what, a, dt in (('tok_off', tok_off, torch.int64), ('tok_n', tok_n if n_host is None else n_host, torch.int32),
                                                    ('tok_file', tok_file, torch.int32), ('tok_on', tok_on, torch.float64),
                                                    ('tok_end', tok_end, torch.float64))]
    if groups is not None:
        cols.append(column('groups', groups, torch.int32))
    T = cols[1].numel()
    if any(c.numel() != T for c in cols):
        raise ValueError('%s: the token columns differ in length: %s' % (who, [c.numel() for c in cols]))
    first = host('cl_first', cl_first.cpu().numpy() if isinstance(cl_first, torch.Tensor) else cl_first, torch.int64)
    if len(first) < 1 or first[0] != 0 or first[-1] != T or (np.diff(first) < 0).any():
        raise ValueError('%s: cl_first must run from 0 to the %d tokens without decreasing' % (who, T))
    longest = (int(n_host.max()) if n_host is not None else int(cols[1].max())) if T else 0
    if longest > cap:
        raise ValueError('%s: a transcription of %d symbols; this route takes up to %d (abns_edit_hist_max_len)' % (who, longest, cap))
    M, n_cl = max(1, longest), len(first) - 1
    size = np.diff(first)
    if T:
        dev = cols[1].device
        cid = torch.repeat_interleave(torch.arange(n_cl, device=dev), torch.from_numpy(size).to(dev))
        order = torch.argsort(cid * (cap + 2) + cols[1].clamp(0, cap + 1).to(torch.int64))
        cols = [c[order].contiguous() for c in cols]
    n_all = int((size * (size - 1) // 2).sum())
    ws_bytes = int(lib.abns_edit_cluster_hist_ws_bytes(T, n_cl, n_all))
    if ws_bytes < 0:
        _lib.check(-1, 'abns_edit_cluster_hist_ws_bytes')
    hist = torch.empty((2, M + 1, M + 1), dtype=torch.int64, device='cuda')
    counts = torch.empty(2, dtype=torch.int64, device='cuda')
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    _lib.check(lib.abns_edit_cluster_hist(_lib.ptr(table), table.numel(), *[_lib.ptr(c) for c in cols[:5]],
                                          _lib.ptr(cols[5] if groups is not None else None), T, first.ctypes.data_as(_lib.C.c_void_p), n_cl, M,
                                          _lib.ptr(hist), _lib.ptr(counts), _lib.ptr(ws), ws_bytes, _lib.stream()), 'abns_edit_cluster_hist')
    counts = counts.cpu()
    return hist.cpu().numpy(), int(counts[0]), int(counts[1])


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

    def prepare_full(self, classes, names=None, times=None, speakers=None):
        """The host half of evaluate_full() in front of the launch: (clusters, Snapped of the flat tokens, cluster_histogram's
        host columns tok_file, tok_on, tok_end, cl_first, groups (None without speakers), coverage)."""
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
        snapped = _snap(len(flat), tok[keep], ph[keep], a)
        number = {n: f for f, n in enumerate(a.names)}
        tok_file = np.array([number[_text(t[0])] for t in flat], dtype=np.int32)
        tok_on, tok_end = np.array([t[1] for t in flat], dtype=np.float64), np.array([t[2] for t in flat], dtype=np.float64)
        size = np.array([len(c) for c in classes], dtype=np.int64)
        cl_first = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(size)])
        groups = None if speakers is None else speaker_groups([t[0] for t in flat], speakers)
        return classes, snapped, tok_file, tok_on, tok_end, cl_first, groups, coverage

    def evaluate_full(self, classes, names=None, times=None, words=None, speakers=None, ignore_words=None):
        """FullTermScores of `classes` (as for evaluate): NED, NED within / across speaker, coverage (evaluate's definition
        and its note) and grouping always; token, type and boundary against `words`, a word Alignment or the path of one
        (None: the three are None).  speakers: a {file: speaker} mapping or a callable file -> speaker (None: one speaker,
        everything is "within").  ignore_words: word symbols that are no words (default: `ignore`).  The pairs are never
        listed: one launch of cluster_histogram, the rest is counting on the host (module docstring).  A transcription
        longer than 256 phones is cluster_histogram's ValueError."""
        prepared = self.prepare_full(classes, names, times, speakers)
        _, snapped, tok_file, tok_on, tok_end, cl_first, groups, _ = prepared
        hist, n_pairs, n_skipped = cluster_histogram(snapped.table, snapped.tok_off, snapped.tok_n, tok_file, tok_on, tok_end, cl_first, groups)
        return self.finish_full(prepared, hist, n_pairs, n_skipped, words, ignore_words)

    def finish_full(self, prepared, hist, n_pairs, n_skipped, words=None, ignore_words=None):
        """The host half of evaluate_full() behind the launch: FullTermScores from prepare_full()'s tuple and
        cluster_histogram()'s three results (tests/test_tde_full_host.py runs the two halves without a GPU)."""
        classes, snapped, tok_file, tok_on, tok_end, cl_first, groups, coverage = prepared
        n_same = same_type_pairs(snapped, tok_file, tok_on, tok_end)
        token = typ = boundary = None
        n_gold = n_gold_empty = 0
        if words is not None:
            gold = gold_words(words, self.alignment, self.ignore, ignore_words)
            token, typ, boundary = token_scores(snapped, gold), type_scores(snapped, gold), word_boundary_scores(snapped, gold)
            n_gold, n_gold_empty = gold.n_gold, gold.n_gold_empty
        return FullTermScores(ned_from_hist(hist), ned_from_hist(hist[0:1]), ned_from_hist(hist[1:2]), coverage, token, typ, boundary,
                              grouping_scores(hist, n_same), len(classes), len(snapped.tok_n), int((snapped.tok_n == 0).sum()), n_gold,
                              n_gold_empty, n_pairs, n_skipped, n_same, hist)


# ---------------------------------------------------------------------------------------------------------------
# the full score set's host side: snapping, the gold words, counting (module docstring)

def _snap(T, tok, ph, alignment):
    """Snapped of T tokens from the (token number, phone row) list of their kept phones, by token then time."""
    table, tok_off, tok_n = _table(T, tok, alignment.ids[ph])
    fnum, lo, hi = (np.full(T, -1, dtype=np.int64) for _ in range(3))
    has = tok_n > 0
    row_lo, row_hi = ph[tok_off[has]], ph[tok_off[has] + tok_n[has] - 1]
    f = np.searchsorted(alignment.first, row_lo, side='right') - 1
    fnum[has], lo[has], hi[has] = f, row_lo - alignment.first[f], row_hi - alignment.first[f]
    return Snapped(table, tok_off, tok_n, fnum, lo, hi)


def snap_tokens(tokens, alignment, ignore=()):
    """Snapped of (file, onset, offset) tokens (module docstring: snap)."""
    tok, ph = _belongs(tokens, alignment)
    keep = ~_ignored(alignment, ignore)[alignment.ids[ph]]
    return _snap(len(tokens), tok[keep], ph[keep], alignment)


def _spans(s):
    return {(int(f), int(a), int(b)) for f, a, b in zip(s.file[s.tok_n > 0], s.lo[s.tok_n > 0], s.hi[s.tok_n > 0])}


def _types(s):
    return {tuple(s.table[o:o + n].tolist()) for o, n in zip(s.tok_off.tolist(), s.tok_n.tolist()) if n}


def _edges(spans):
    return {(f, a) for f, a, _ in spans} | {(f, b + 1) for f, _, b in spans}


def gold_words(words, alignment, ignore=(), ignore_words=None):
    """GoldWords of a word alignment (an Alignment whose symbols are words, or the path of one) against the phone
    `alignment`: every row whose symbol is not in ignore_words (default: `ignore`) snapped with `ignore`."""
    if isinstance(words, str):
        words = read_alignment(words)
    if isinstance(alignment, str):
        alignment = read_alignment(alignment)
    skip = _ignored(words, ignore if ignore_words is None else ignore_words)
    fnum = np.repeat(np.arange(len(words.names)), np.diff(words.first))
    rows = np.flatnonzero(~skip[words.ids]) if len(words.ids) else np.zeros(0, dtype=np.int64)
    s = snap_tokens([(words.names[fnum[r]], words.onset[r], words.offset[r]) for r in rows], alignment, ignore)
    spans = _spans(s)
    return GoldWords(spans, _types(s), _edges(spans), len(rows), int((s.tok_n == 0).sum()))


def prf(n_hit, n_found, n_gold):
    """(precision, recall, F) of counts; a ratio with an empty denominator is 0, as in boundary_scores."""
    p = n_hit / n_found if n_found else 0.0
    r = n_hit / n_gold if n_gold else 0.0
    return p, r, (2.0 * p * r / (p + r) if p + r > 0 else 0.0)


def token_scores(found, gold):
    """(precision, recall, F) of the distinct found spans against the distinct gold spans."""
    F = _spans(found)
    return prf(len(F & gold.spans), len(F), len(gold.spans))


def type_scores(found, gold):
    """(precision, recall, F) of the distinct found transcriptions against the gold lexicon (Ludusan et al. 2014, at the
    level of phone strings)."""
    types = _types(found)
    return prf(len(types & gold.lexicon), len(types), len(gold.lexicon))


def word_boundary_scores(found, gold):
    """(precision, recall, F) of the found spans' edges against the gold spans' edges: an exact match after snapping."""
    edges = _edges(_spans(found))
    return prf(len(edges & gold.boundaries), len(edges), len(gold.boundaries))


def same_type_pairs(snapped, tok_file, tok_on, tok_end):
    """|S|: the pairs of tokens with identical non-empty transcriptions that do not lie in one file overlapping in time, from
    counts alone: per type C(m, 2); per (type, file) the overlapping pairs are subtracted -- the tokens sorted by
    (onset, end), token j with end > onset overlaps the earlier ones that end after its onset, j minus the number of ALL
    ends of the group <= its onset (a later token that ends there has no length and sorts before j)."""
    n = snapped.tok_n
    sel = np.flatnonzero(n > 0)
    if not len(sel):
        return 0
    key, tid = {}, np.empty(len(sel), dtype=np.int64)
    for k, t in enumerate(sel):
        o = snapped.tok_off[t]
        tid[k] = key.setdefault(snapped.table[o:o + n[t]].tobytes(), len(key))
    m = np.bincount(tid)
    total = int((m * (m - 1) // 2).sum())
    f, on, end = np.asarray(tok_file, dtype=np.int64)[sel], np.asarray(tok_on, dtype=np.float64)[sel], np.asarray(tok_end, dtype=np.float64)[sel]
    order = np.lexsort((end, on, f, tid))
    tid, f, on, end = tid[order], f[order], on[order], end[order]
    new = np.concatenate([[True], (tid[1:] != tid[:-1]) | (f[1:] != f[:-1])])
    group = np.cumsum(new) - 1
    start = np.flatnonzero(new)[group]
    j = np.arange(len(sel)) - start                                 # a token's place in its (type, file) group
    # times as ranks, so that (group, time) becomes one integer key
    ticks = np.unique(np.concatenate([on, end]))
    R = len(ticks) + 1
    on_key, end_key = group * R + np.searchsorted(ticks, on), group * R + np.searchsorted(ticks, end)
    ended = np.searchsorted(np.sort(end_key), on_key, side='right') - start
    return total - int((j - ended)[end > on].sum())


def ned_from_hist(hist):
    """sum hist[g][d][L] d / L over sum hist as an exact Fraction, rounded once to float64; nan for an empty histogram."""
    hist = np.asarray(hist)
    n = int(hist.sum())
    if not n:
        return float('nan')
    g, d, L = np.nonzero(hist)
    return float(sum((Fraction(int(hist[a, b, c]) * int(b), int(c)) for a, b, c in zip(g, d, L)), Fraction(0)) / n)


def grouping_scores(hist, n_same):
    """(precision, recall, F) by pair counting: |C n S| / |C| and |C n S| / |S| with |C| = sum hist and |C n S| = the pairs
    at distance 0."""
    hist = np.asarray(hist)
    return prf(int(hist[:, 0, :].sum()), int(hist.sum()), int(n_same))


def speaker_groups(files, speakers):
    """int32 speaker number per file name of `files`; speakers: a {file: speaker} mapping or a callable file -> speaker."""
    ids, out = {}, np.empty(len(files), dtype=np.int32)
    for k, f in enumerate(files):
        f = _text(f)
        if callable(speakers):
            s = speakers(f)
        elif f in speakers:
            s = speakers[f]
        else:
            raise ValueError('speakers: no speaker for file %r' % f)
        out[k] = ids.setdefault(s, len(ids))
    return out


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


def full_summary(s):
    """The one line `python -m abnet3_amd.tde --full` and examples/zero_resource.py print for a FullTermScores."""
    triple = lambda name, t: '' if t is None else ' %s P %.4f R %.4f F %.4f' % ((name,) + tuple(t))
    return ('NED %.4f (within %.4f, across %.4f) coverage %.4f%s%s%s%s (%d clusters, %d tokens, %d empty, %d gold words, %d empty, '
            '%d pairs, %d skipped, %d same-type pairs)'
            % (s.ned, s.ned_within, s.ned_across, s.coverage, triple('token', s.token), triple('type', s.type), triple('boundary', s.boundary),
               triple('grouping', s.grouping), s.n_clusters, s.n_tokens, s.n_empty, s.n_gold, s.n_gold_empty, s.n_pairs, s.n_skipped, s.n_same))


def read_speakers(path):
    """{file: speaker} of a file of ``file speaker`` lines."""
    out = {}
    with open(path, 'r', encoding='utf-8') as fh:
        for ln, line in enumerate(fh, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 2:
                raise ValueError('%s:%d: expected "file speaker", got %r' % (path, ln, line.rstrip('\n')))
            out[parts[0]] = parts[1]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m abnet3_amd.tde', description='NED and coverage of a .classes file against a phone alignment')
    ap.add_argument('--full', action='store_true', help='the full score set: NED within / across speaker, token, type, boundary, grouping')
    ap.add_argument('--words', default=None, metavar='WORD_ALIGNMENT', help='with --full: "file onset offset word" lines, the gold words')
    ap.add_argument('--speakers', default=None, metavar='FILE', help='with --full: "file speaker" lines')
    ap.add_argument('classes', nargs='?', default=None, help='.classes file (terms.write_classes)')
    ap.add_argument('alignment', help='phone alignment: "file onset offset symbol" lines')
    ap.add_argument('--ignore', nargs='*', default=[], metavar='SYMBOL', help='symbols that are no phones (silence, noise)')
    ap.add_argument('--boundaries', default=None, metavar='FILE.npz', help='an .npz of file -> boundary times: the boundary scores')
    ap.add_argument('--tolerance', type=float, default=0.02, help='seconds within which a found boundary hits a gold one')
    args = ap.parse_args(argv)
    if args.classes is None and args.boundaries is None:
        ap.error('a .classes file or --boundaries is needed')
    if (args.words is not None or args.speakers is not None) and not args.full:
        ap.error('--words and --speakers belong to --full')
    if args.full:
        if args.classes is None:
            ap.error('--full needs a .classes file')
        speakers = None if args.speakers is None else read_speakers(args.speakers)
        print(full_summary(TermEvaluator(args.alignment, ignore=args.ignore).evaluate_full(args.classes, words=args.words, speakers=speakers)))
    elif args.classes is not None:
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
