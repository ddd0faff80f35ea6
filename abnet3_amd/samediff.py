"""Same-different word discrimination (Carlin et al. 2011) on the MI355X: rank all pairs of gold word tokens by
distance and report the average precision of "same word".  It scores the two objects the unsupervised stages are
built on: frame features (DTW between the tokens, the distance ABX uses) and the fixed-size segment vectors that
KnnPairMiner searches and ESKMeans clusters (the cosine of `abn_segment_vectors`' rows).

    python -m abnet3_amd.samediff CLASSES FEATURES [--distance vectors|dtw|dtw-kl] [--frames K]
                                  [--condition all|swdp|swsp] [--spk FILE]

The definition this module computes:

* Tokens are sorted by word type on the host, so type c occupies a contiguous index range.  Row i carries cbeg[i],
  cend[i] (its type's range, half open) and optionally spk[i].
* Pool: all pairs i < j whose similarity is finite.  A pair is POSITIVE when j lies in [cbeg[i], cend[i]).
  `condition` selects the positives and the pool:
      'all'   positives: every same-type pair;               left out of the pool: nothing
      'swdp'  positives: same word, different speaker;        left out: same-word same-speaker pairs
      'swsp'  positives: same word, same speaker;             left out: same-word different-speaker pairs
  Different-word pairs are always in the pool as negatives.
* Thresholds: v_0 >= v_1 >= ... >= v_{P-1}, the positives' similarities sorted by float comparison, NaN removed
  (a positive is a pool pair, so +-inf is removed with it).
* Bucket: for a pool pair of similarity x, b(x) = #{r : v_r > x}, in [0, P].  hist[b] (length P + 1) counts the pool
  pairs per bucket, positives included.
* Tie groups: for a group g of equal thresholds with first index f_g and last index + 1 = l_g, the pool pairs at
  least that similar number A_g = sum_{b <= f_g} hist[b] (x >= v  <=>  b(x) <= #{v_r > v}), the positives among them
  l_g.
* Scores: precision P_g = l_g / A_g, recall R_g = l_g / P;
      AP  = sum_g (l_g - f_g) / P * P_g      (scikit-learn's average_precision_score with ties grouped),
      PRB = P_g at the group that minimises |P_g - R_g|, the first such group on a tie
  (the precision-recall breakeven).  Both follow from integers; they are returned as float64 (AP: the exact sum
  rounded once; PRB: the minimising group chosen by exact comparison).  P = 0 gives nan for both.
* For a distance (the DTW route) the order is reversed: v ascending, b(x) = #{r : v_r < x}.

`distance='vectors'`: the n x n similarities are never stored.  `abn_sd_collect` writes the same-type pairs'
similarities, they are masked by `condition` and sorted on the device, and `abn_sd_count` forms every tile again and
counts each pair into its bucket behind the tile -- the same bits in both passes.
`distance='dtw'` / `'dtw-kl'`: the i < j pairs go through `abx.dtw_cost_batch` in chunks (the distance is
total_cost / path_len in float64, as ABX normalises); buckets by torch.searchsorted, counts by torch.bincount.
"""
import argparse
import sys
from fractions import Fraction

import numpy as np
import torch

from . import _lib

CONDITIONS = ('all', 'swdp', 'swsp')
DISTANCES = ('vectors', 'dtw', 'dtw-kl')
DTW_CHUNK = 1 << 20                   # most pairs in one dtw_cost_batch call (a single row's pairs may exceed it)
_AP_BITS = 256                        # fixed-point bits of the exact AP sum


# ---------------------------------------------------------------------------------------------------------------
# host tables

def sort_by_type(types):
    """(order, cbeg, cend): `order` sorts the tokens by type (stable); cbeg / cend [n] int32 are the half-open range of
    each SORTED row's type.  types: one hashable label per token."""
    labels = {}
    ids = np.array([labels.setdefault(t, len(labels)) for t in types], dtype=np.int64)
    order = np.argsort(ids, kind='stable')
    s = ids[order]
    n = len(s)
    first = np.ones(n, dtype=bool)
    first[1:] = s[1:] != s[:-1]
    beg = np.flatnonzero(first)
    size = np.diff(np.append(beg, n))
    return order, np.repeat(beg, size).astype(np.int32), np.repeat(beg + size, size).astype(np.int32)


def check_ranges(cbeg, cend):
    """ValueError unless cbeg / cend describe contiguous types: cbeg[i] <= i < cend[i] <= n, one range per type."""
    cbeg, cend = np.asarray(cbeg), np.asarray(cend)
    n = len(cbeg)
    if cbeg.shape != (n,) or cend.shape != (n,):
        raise ValueError('samediff: cbeg and cend must be two arrays of one length')
    i = np.arange(n)
    ok = n == 0 or (cbeg[0] == 0 and (cbeg <= i).all() and (i < cend).all() and (cend <= n).all())
    if ok and n > 1:
        inside = i[1:] < cend[:-1]                       # row i + 1 belongs to row i's type
        ok = (np.where(inside, (cbeg[1:] == cbeg[:-1]) & (cend[1:] == cend[:-1]), cbeg[1:] == i[1:])).all()
    if not ok:
        raise ValueError('samediff: cbeg / cend are not the ranges of tokens sorted by type')
    return cbeg.astype(np.int32), cend.astype(np.int32)


def positive_offsets(cbeg, cend):
    """(pos_off int64 [n], total): row i's same-type pairs (i, i + 1) .. (i, cend[i] - 1) start at pos_off[i]."""
    m = np.asarray(cend, dtype=np.int64) - np.arange(len(cend), dtype=np.int64) - 1
    return np.cumsum(m) - m, int(m.sum())


def positive_index(cbeg, cend, device=None):
    """(i, j) int64 tensors: the pair behind every entry of collect()'s list, by index arithmetic."""
    pos_off, total = positive_offsets(cbeg, cend)
    m = torch.from_numpy(np.asarray(cend, dtype=np.int64) - np.arange(len(cend), dtype=np.int64) - 1).to(device)
    i = torch.repeat_interleave(torch.arange(len(cend), device=device), m)
    j = torch.arange(total, device=device) - torch.from_numpy(pos_off).to(device)[i] + i + 1
    return i, j


def condition_mask(i, j, spk, condition):
    """bool per same-type pair (i, j): it is a positive under `condition` (spk: int tensor per token, or None)."""
    if condition not in CONDITIONS:
        raise ValueError('condition must be one of %s, not %r' % (CONDITIONS, condition))
    if condition == 'all':
        return torch.ones_like(i, dtype=torch.bool)
    if spk is None:
        raise ValueError('condition=%r needs the tokens\' speakers' % condition)
    same = spk[i] == spk[j]
    return same if condition == 'swsp' else ~same


def speaker_ids(files, speakers):
    """int32 speaker number per file name in `files`; speakers: {file: speaker}, a callable, or the path of a
    "<file> <speaker>" list (utils.read_spkid_file)."""
    if isinstance(speakers, str):
        from .utils import read_spkid_file
        speakers = read_spkid_file(speakers)
    look = speakers if callable(speakers) else speakers.__getitem__
    number = {}
    try:
        return np.array([number.setdefault(look(f), len(number)) for f in files], dtype=np.int32)
    except KeyError as e:
        raise ValueError('samediff: no speaker for file %r' % (e.args[0],))


# ---------------------------------------------------------------------------------------------------------------
# table level

def _table(X, cbeg, cend):
    _lib.require_device(X)
    if X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError('samediff: X must be a [n, d] float32 table')
    n, d = X.shape
    if d < 4 or d > _lib.SD_MAX_D or d % 4:
        raise ValueError('samediff: d = %d; the kernel takes multiples of 4 in 4 .. %d' % (d, _lib.SD_MAX_D))
    if n < 1 or n > _lib.SD_MAX_N:
        raise ValueError('samediff: n = %d; the kernel takes 1 .. %d tokens' % (n, _lib.SD_MAX_N))
    to_host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else a
    cbeg, cend = check_ranges(to_host(cbeg), to_host(cend))
    if len(cbeg) != n:
        raise ValueError('samediff: %d rows, %d type ranges' % (n, len(cbeg)))
    return n, d, cbeg, cend, torch.from_numpy(cbeg).to(X.device), torch.from_numpy(cend).to(X.device)


def collect(X, cbeg, cend):
    """abn_sd_collect: (pos_sim float32 device tensor, pos_off int64 host array) -- sim(i, j) of every same-type pair
    i < j at pos_sim[pos_off[i] + (j - i - 1)].  X [n, d]: float32 device rows sorted by type; cbeg / cend: the rows'
    type ranges (sort_by_type).  positive_index gives the (i, j) of every entry."""
    n, d, cbeg, cend, d_beg, d_end = _table(X, cbeg, cend)
    pos_off, total = positive_offsets(cbeg, cend)
    pos_sim = torch.empty(total, dtype=torch.float32, device=X.device)
    if total == 0:                                         # singletons only: nothing to write
        return pos_sim, pos_off
    d_off = torch.from_numpy(pos_off).to(X.device)
    _lib.check(_lib.load().abn_sd_collect(_lib.ptr(X), n, d, _lib.ptr(d_beg), _lib.ptr(d_end), _lib.ptr(d_off),
                                          _lib.ptr(pos_sim), _lib.stream()), 'abn_sd_collect')
    return pos_sim, pos_off


def pair_histogram(X, cbeg, cend, thr, spk=None, condition='all'):
    """abn_sd_count: (hist int64 device tensor [len(thr) + 1], n_bad int) of the module docstring's pool.
    thr: float32 device tensor, descending; spk: int32 per row (array or tensor), needed by 'swdp' / 'swsp'."""
    if condition not in CONDITIONS:
        raise ValueError('condition must be one of %s, not %r' % (CONDITIONS, condition))
    n, d, cbeg, cend, d_beg, d_end = _table(X, cbeg, cend)
    thr = torch.as_tensor(thr, dtype=torch.float32).to(X.device).contiguous()
    if thr.dim() != 1 or thr.numel() > _lib.SD_MAX_THR:
        raise ValueError('samediff: thr must be one row of at most %d thresholds' % _lib.SD_MAX_THR)
    if thr.numel() > 1 and not bool((thr[1:] <= thr[:-1]).all()):
        raise ValueError('samediff: thr must be descending (and free of NaN)')
    d_spk = None
    if spk is not None:
        d_spk = torch.as_tensor(spk).to(device=X.device, dtype=torch.int32).contiguous()
        if tuple(d_spk.shape) != (n,):
            raise ValueError('samediff: %d rows, %d speakers' % (n, d_spk.numel()))
    elif condition != 'all':
        raise ValueError('condition=%r needs the tokens\' speakers' % condition)
    hist = torch.empty(thr.numel() + 1, dtype=torch.int64, device=X.device)
    bad = torch.empty(1, dtype=torch.int64, device=X.device)
    _lib.check(_lib.load().abn_sd_count(_lib.ptr(X), n, d, _lib.ptr(d_beg), _lib.ptr(d_end), _lib.ptr(d_spk),
                                        _lib.SD_CONDITION[condition], _lib.ptr(thr) if thr.numel() else None, thr.numel(),
                                        _lib.ptr(hist), _lib.ptr(bad), _lib.stream()), 'abn_sd_count')
    return hist, int(bad.item())


def vector_histogram(X, cbeg, cend, spk=None, condition='all'):
    """(thr float32 descending, hist int64 [P + 1], n_bad), thr and hist on the device: collect, the mask by
    `condition`, the sort, pair_histogram -- the 'vectors' route over a table of rows sorted by type."""
    pos_sim, _ = collect(X, cbeg, cend)
    i, j = positive_index(cbeg, cend, X.device)
    d_spk = None if spk is None else torch.as_tensor(spk).to(X.device)
    v = pos_sim[condition_mask(i, j, d_spk, condition)]
    thr = torch.sort(v[torch.isfinite(v)], descending=True)[0]
    hist, n_bad = pair_histogram(X, cbeg, cend, thr, spk, condition)
    return thr, hist, n_bad


class Scores(object):
    """ap, prb (float64; nan without positives) and, per tie group of the thresholds, precision / recall (float64
    arrays) with the groups' first / last + 1 threshold indices."""

    def __init__(self, ap, prb, precision, recall, first, last):
        self.ap, self.prb, self.precision, self.recall, self.first, self.last = ap, prb, precision, recall, first, last


def scores_from_histogram(thr, hist):
    """Scores of the module docstring from the sorted thresholds (descending similarities or ascending distances:
    only their tie groups are read) and hist [len(thr) + 1].  Runs on the host."""
    host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    thr, hist = host(thr), host(hist).astype(np.int64)
    P = len(thr)
    if hist.shape != (P + 1,):
        raise ValueError('samediff: %d thresholds need a histogram of %d buckets, not %s' % (P, P + 1, hist.shape))
    empty = np.zeros(0)
    if P == 0:
        return Scores(float('nan'), float('nan'), empty, empty, empty.astype(np.int64), empty.astype(np.int64))
    new = np.ones(P, dtype=bool)
    new[1:] = thr[1:] != thr[:-1]
    f = np.flatnonzero(new)
    l = np.append(f[1:], P)
    A = np.cumsum(hist)[f]
    if (A < l).any():
        raise ValueError('samediff: the histogram holds fewer pairs than positives (not this threshold list\'s)')
    precision, recall = l / A.astype(np.float64), l / float(P)
    # AP = sum_g (l - f) l / A / P, rounded ONCE: each quotient in 256-bit fixed point (Python integers in numpy object
    # arrays; floor: below the exact value by < 2^-256 each).  A float64 sum of the groups' terms is not enough for
    # the definition's exact cases: 49 separated positives of 49 different similarities give sum(49 x fl(1 / 49)),
    # which is 1 - 2^-53 however it is summed (math.fsum included).
    total = ((((l - f) * l).astype(object) << _AP_BITS) // A.astype(object)).sum()
    ap = float(Fraction(int(total), P << _AP_BITS))
    # PRB: float64 finds the candidates, exact fractions choose among them
    gap = np.abs(precision - recall)
    cand = np.flatnonzero(gap <= gap.min() + 1e-9)
    exact = [abs(Fraction(int(l[g]), int(A[g])) - Fraction(int(l[g]), P)) for g in cand]
    g = int(cand[exact.index(min(exact))])
    return Scores(ap, float(precision[g]), precision, recall, f, l)


# ---------------------------------------------------------------------------------------------------------------
# the DTW route

def upper_pairs(n, i0, i1):
    """(i, j) int64 host arrays: the pairs i < j < n with i0 <= i < i1, row after row, by index arithmetic."""
    rows = np.arange(i0, i1, dtype=np.int64)
    m = n - 1 - rows
    i = np.repeat(rows, m)
    j = np.arange(int(m.sum()), dtype=np.int64) - np.repeat(np.cumsum(m) - m, m) + i + 1
    return i, j


def row_chunks(n, chunk=DTW_CHUNK):
    """[(i0, i1)]: runs of rows whose pairs number at most `chunk` (a run is never empty)."""
    out, i0 = [], 0
    while i0 < n - 1:
        i1, count = i0, 0
        while i1 < n - 1 and (i1 == i0 or count + (n - 1 - i1) <= chunk):
            count += n - 1 - i1
            i1 += 1
        out.append((i0, i1))
        i0 = i1
    return out


def dtw_distances(table, row0, length, i, j, distance='dtw'):
    """(dist float64 device, ok bool device) of the token pairs (i, j): total_cost / path_len of abx.dtw_cost_batch
    (cosine frames for 'dtw', symmetrised KL over kl_tables' triple for 'dtw-kl'); ok is False where the kernel
    dropped the pair (path_len 0) or the distance is not finite.  A token 2 beyond abn_dtw_cost_max_n2() raises."""
    from . import abx
    cap = _lib.load().abn_dtw_cost_max_n2()
    n2 = np.asarray(length)[j]
    if len(n2) and n2.max() > cap:
        raise ValueError('samediff: a token of %d frames; the DTW cost kernel takes at most %d as token 2' % (n2.max(), cap))
    cost, plen = abx.dtw_cost_batch(table, row0[i], length[i], table, row0[j], length[j],
                                    distance='kl' if distance == 'dtw-kl' else 'cosine')
    dist = cost / plen.to(torch.float64)
    ok = (plen > 0) & torch.isfinite(dist)
    return dist, ok


def dtw_histogram(table, row0, length, cbeg, cend, spk=None, condition='all', distance='dtw', chunk=DTW_CHUNK):
    """(thr float64 ascending, hist int64 [P + 1], n_bad), all on the host, of the tokens (row0, length: host arrays,
    sorted by type) under DTW.  Two passes: the same-type pairs give the thresholds, then every pair its bucket."""
    cbeg, cend = check_ranges(cbeg, cend)
    n = len(cbeg)
    row0, length = np.asarray(row0, dtype=np.int64), np.asarray(length, dtype=np.int32)
    dev = (table[0] if isinstance(table, tuple) else table).device
    d_spk = None if spk is None else torch.as_tensor(spk).to(dev)
    d_end = torch.from_numpy(cend.astype(np.int64)).to(dev)
    pi, pj = positive_index(cbeg, cend)
    keep = condition_mask(pi.to(dev), pj.to(dev), d_spk, condition).cpu().numpy()
    pi, pj = pi.numpy()[keep], pj.numpy()[keep]
    parts = []
    for a in range(0, len(pi), chunk):
        dist, ok = dtw_distances(table, row0, length, pi[a:a + chunk], pj[a:a + chunk], distance)
        parts.append(dist[ok])
    thr = torch.sort(torch.cat(parts))[0] if parts else torch.zeros(0, dtype=torch.float64, device=dev)
    hist = torch.zeros(thr.numel() + 1, dtype=torch.int64, device=dev)
    n_bad = 0
    for i0, i1 in row_chunks(n, chunk):
        i, j = upper_pairs(n, i0, i1)
        di, dj = torch.from_numpy(i).to(dev), torch.from_numpy(j).to(dev)
        same = dj < d_end[di]
        pool = (~same | condition_mask(di, dj, d_spk, condition)).cpu().numpy()
        i, j = i[pool], j[pool]
        dist, ok = dtw_distances(table, row0, length, i, j, distance)
        n_bad += int((~ok).sum())
        # b(x) = #{r : v_r < x}
        hist += torch.bincount(torch.searchsorted(thr, dist[ok], right=False), minlength=thr.numel() + 1)
    return thr.cpu().numpy(), hist.cpu().numpy(), n_bad


# ---------------------------------------------------------------------------------------------------------------
# the evaluator

class SameDifferentResult(object):
    """ap, prb: the scores (float64).  n_tokens, n_types: the tokens scored and their types; n_positives: P;
    n_pairs: the pool; n_bad: pairs left out for a non-finite similarity or a dropped alignment; n_dropped_tokens:
    tokens without frames or (vectors) with all-zero frames.  scores: the per-group arrays (Scores)."""

    def __init__(self, distance, condition, scores, n_tokens, n_types, n_positives, n_pairs, n_bad, n_dropped_tokens):
        self.distance, self.condition, self.scores = distance, condition, scores
        self.ap, self.prb = scores.ap, scores.prb
        self.n_tokens, self.n_types, self.n_positives, self.n_pairs = n_tokens, n_types, n_positives, n_pairs
        self.n_bad, self.n_dropped_tokens = n_bad, n_dropped_tokens

    def __repr__(self):
        return ('SameDifferentResult(%s, %s: AP %.4f, PRB %.4f, %d tokens of %d types, %d positives in %d pairs, %d bad, '
                '%d tokens dropped)' % (self.distance, self.condition, self.ap, self.prb, self.n_tokens, self.n_types,
                                        self.n_positives, self.n_pairs, self.n_bad, self.n_dropped_tokens))


class SameDifferentEvaluator(object):
    """Same-different scores of the word tokens in `classes` over the frames of `corpus` (module docstring).

    classes: the path of a .classes file or clusters of (file, onset, offset) tokens (tde.read_classes,
    TermEvaluator); a cluster is a word type.  corpus: a DeviceCorpus, a {name: [T, D]} features dict together with
    `times`, or the path of an h5features file (as ABXEvaluator).  speakers: {file: speaker}, a callable, or the path
    of a "<file> <speaker>" list; needed by the 'swdp' / 'swsp' conditions only."""

    def __init__(self, classes, corpus, times=None, speakers=None):
        from .abx import _read_h5features
        from .dataloader import DeviceCorpus
        from .tde import read_classes
        if isinstance(classes, str):
            classes = read_classes(classes)
        if isinstance(corpus, str):
            corpus, times = _read_h5features(corpus)
        if not isinstance(corpus, DeviceCorpus):
            if times is None:
                raise ValueError('SameDifferentEvaluator: a features dict needs its times dict')
            corpus = DeviceCorpus(corpus, times)
        self.corpus = corpus
        self.tokens = [tok for c in classes for tok in c]
        self.types = np.array([k for k, c in enumerate(classes) for _ in c], dtype=np.int64)
        self.row0 = np.zeros(len(self.tokens), dtype=np.int64)
        self.length = np.zeros(len(self.tokens), dtype=np.int32)
        for k, (f, on, off) in enumerate(self.tokens):
            self.row0[k], self.length[k] = corpus.token(f, on, off)
        self.spk = None if speakers is None else speaker_ids([t[0] for t in self.tokens], speakers)
        self._kl = None

    def _sorted(self, keep):
        """The kept tokens sorted by type: (token numbers, cbeg, cend, spk)."""
        kept = np.flatnonzero(keep)
        order, cbeg, cend = sort_by_type(self.types[kept].tolist())
        sel = kept[order]
        return sel, cbeg, cend, (None if self.spk is None else self.spk[sel])

    def evaluate(self, distance='vectors', frames=10, condition='all'):
        if distance not in DISTANCES:
            raise ValueError('distance must be one of %s, not %r' % (DISTANCES, distance))
        if condition not in CONDITIONS:
            raise ValueError('condition must be one of %s, not %r' % (CONDITIONS, condition))
        if condition != 'all' and self.spk is None:
            raise ValueError('condition=%r needs `speakers`' % condition)
        keep = self.length > 0
        if distance == 'vectors':
            from .discovery import segment_vectors
            d = frames * self.corpus.dim
            if frames < 1 or d < 4 or d > _lib.SD_MAX_D or d % 4:
                raise ValueError('SameDifferentEvaluator: frames x feature dimension = %d; the kernel takes multiples of '
                                 '4 in 4 .. %d' % (d, _lib.SD_MAX_D))
            some = np.flatnonzero(keep)
            vec, nonzero = segment_vectors(self.corpus.table, self.row0[some], self.length[some], frames)
            keep[some[~nonzero.cpu().numpy()]] = False
        sel, cbeg, cend, spk = self._sorted(keep)
        n, n_dropped = len(sel), len(keep) - len(sel)
        n_types = len(np.unique(cbeg))
        if n > _lib.SD_MAX_N:
            raise ValueError('SameDifferentEvaluator: %d tokens; the kernel takes at most %d' % (n, _lib.SD_MAX_N))
        if n == 0:
            return SameDifferentResult(distance, condition, scores_from_histogram(np.zeros(0), np.zeros(1)), 0, 0, 0, 0, 0,
                                       n_dropped)
        if distance == 'vectors':
            pos = np.full(len(keep), -1, dtype=np.int64)
            pos[some] = np.arange(len(some))
            X = vec[torch.from_numpy(pos[sel]).to(vec.device)].contiguous()
            thr, hist, n_bad = vector_histogram(X, cbeg, cend, spk, condition)
            hist = hist.cpu().numpy()
        else:
            if distance == 'dtw-kl' and self._kl is None:
                from .abx import kl_tables
                self._kl = kl_tables(self.corpus.table)
            table = self._kl if distance == 'dtw-kl' else self.corpus.table
            thr, hist, n_bad = dtw_histogram(table, self.row0[sel], self.length[sel], cbeg, cend, spk, condition, distance)
        return SameDifferentResult(distance, condition, scores_from_histogram(thr, hist), n, n_types, len(thr),
                                   int(hist.sum()), n_bad, n_dropped)


def parser():
    ap = argparse.ArgumentParser(prog='python -m abnet3_amd.samediff',
                                 description='same-different word discrimination: average precision over all token pairs')
    ap.add_argument('classes', help='.classes file of gold word tokens: one class per word type')
    ap.add_argument('features', help='h5features file')
    ap.add_argument('--distance', choices=DISTANCES, default='vectors')
    ap.add_argument('--frames', type=int, default=10, help='frames sampled per token (vectors)')
    ap.add_argument('--condition', choices=CONDITIONS, default='all')
    ap.add_argument('--spk', default=None, help='"<file> <speaker>" list (needed by swdp / swsp)')
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    r = SameDifferentEvaluator(args.classes, args.features, speakers=args.spk).evaluate(args.distance, args.frames,
                                                                                        args.condition)
    print('same-different (%s, %s): AP %.4f, PRB %.4f (%d tokens, %d types, %d positives, %d pairs, %d bad, %d tokens dropped)'
          % (r.distance, r.condition, r.ap, r.prb, r.n_tokens, r.n_types, r.n_positives, r.n_pairs, r.n_bad,
             r.n_dropped_tokens))
    return 0


if __name__ == '__main__':
    sys.exit(main())
