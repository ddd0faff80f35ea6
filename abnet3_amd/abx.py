"""ABX phone discriminability of embeddings (the ZeroSpeech 2017 track-1 measure) on the MI355X.

    python -m abnet3_amd.abx FEATURES ITEMS [--mode within|across|both] [--distance cosine|kl] [--floor F]

The definition this module computes:

* Item file: ZeroSpeech 2017 format, header ``#file onset offset #phone prev-phone next-phone speaker``, fields
  separated by whitespace, times in seconds.  An item's context is the pair (prev-phone, next-phone).
* Token: ``DeviceCorpus.token(file, onset, offset)``, the frames with onset <= t <= offset.  An item with no frame
  is dropped and reported (``ABXResult.dropped``).
* Distance: d(P, Q) = total_cost / path_len in float64 of the DTW alignment of P (token 1, rows) with Q (token 2)
  over the angular frame distance -- exactly what ``utils.dtw_align_batch`` computes, by the cost-only kernel
  ``abn_dtw_cost_batched``.  Not symmetrised.  A pair the alignment drops (a NaN frame distance: identical or
  parallel frames whose cosine rounds above 1, or non-finite values) raises ValueError naming the items.  With
  ``parallel='zero'`` (default 'drop': the reference's rule) a cosine that rounds beyond +-1 is read as distance 0
  (1 for opposite frames) instead, the rule of the search kernel: the setting for corpora made of repeated frames,
  such as ``KMeansQuantizer.quantize`` returns; every pair without such a cell keeps its bits.  An
  all-zero frame is not dropped: it is at distance 1 from every other frame and 0 from another zero frame
  (the reference's rule, csrc/dist_ref.h).
* Distance, ``distance='kl'`` (posteriorgrams: the rows a softmax network trained with KLLoss emits, the ZeroSpeech
  evaluation's ``KL`` option): the same DTW over the symmetrised Kullback-Leibler divergence of the frames, by
  ``abn_dtw_cost_kl_batched``.  The reference has no ABX code and no KL frame distance (its KLLoss is a training loss
  over pairs of rows), so this definition is the build's own, like the DTW recurrence ("parity unpinned");
  tests/abx_kl_np.py restates it in numpy bit for bit.
  - Tables (``kl_tables``, ``abn_kl_tables``): for the feature table x [rows, D] float32 and a floor f (float32,
    default 1e-6, > 0): P[r, k] = max(x[r, k], f) in float32, L[r, k] = float32(log(float64(P[r, k]))).  No
    renormalisation.  A row with a non-finite or a negative value is BAD (flagged per row, its P / L contents
    unspecified).  Zeros are legal (a saturated softmax) and are floored.
  - Cell, for frames p (token 1) and q (token 2), in float32 with no fused multiply-add, in ascending k:
    acc = 0; for k: acc = acc + ((P_p[k] - P_q[k]) * (L_p[k] - L_q[k])), each of the four operations rounded to float32
    on its own, subnormals kept; d = 0.5f * acc.  For rows that sum to one this is half the sum of KL(p||q) and
    KL(q||p).  The direct form is deliberate: every term is >= 0 (the rounded logarithm is monotone), so d >= 0
    always and d == 0 exactly for identical frames; the expanded form (entropies minus cross dot products) cancels to
    a few 1e-7 of either sign for near-identical frames, which breaks both properties and the ties the tie-break
    relies on.
  - Recurrence, tie-break, path length and d(P, Q) = total_cost / path_len: those of the cosine route (float64
    cost = d + min(diag, up, left), first minimum in the order diag, up, left, the length carried along the chosen
    predecessor).  Not symmetrised over the pair.
  - A pair one of whose frames lies in a BAD row is dropped (path_len = 0) and raises ValueError naming the items.
  - A token 2 of more than abn_dtw_cost_max_n2() frames (256: 2.56 s; ABX items are phones) raises ValueError: this
    distance has no second kernel to fall back to.  Token 1 is unbounded.
* Within speaker: A, B, X share context and speaker; phone(A) = phone(X) = p, phone(B) = q != p, A != X.  The
  cell is (p, q, context, speaker).
* Across speaker: A, B, X share context; A and B share speaker s, X has speaker t != s; phone(A) = phone(X) = p,
  phone(B) = q != p.  The cell is (p, q, context, s, t).
* A triplet scores 1 when d(A, X) < d(B, X), 1/2 when equal, 0 otherwise.  A cell's score is the mean over its
  triplets (cells without triplets do not exist); cell scores are averaged (unweighted) over contexts, giving one
  score per (p, q, speaker key); those over speaker keys, one per (p, q); those over (p, q), giving S.  The error
  is 100 (1 - S).

Every ordered item pair a mode needs is aligned once (one batched launch), the distances stay on the device and
``abn_abx_score`` counts each cell's triplet scores as integers (2 x score), so the result does not depend on the
order of any sum but the final float64 averages.  Memory is linear in the number of needed pairs.
"""
import argparse
import sys
from collections import defaultdict, namedtuple

import numpy as np
import torch

from . import _lib

MODES = ('within', 'across')
DISTANCES = ('cosine', 'kl')

# what distance='kl' reads of one feature table (kl_tables): P and L [rows, D] float32, bad [rows] uint8, on the device
KLTables = namedtuple('KLTables', ['P', 'L', 'bad'])


class Items(object):
    """The columns of an item file (one entry per item)."""

    def __init__(self, files, onsets, offsets, phones, prev, next_, speakers):
        self.files = list(files)
        self.onsets = np.asarray(onsets, dtype=np.float64)
        self.offsets = np.asarray(offsets, dtype=np.float64)
        self.phones = list(phones)
        self.contexts = list(zip(prev, next_))
        self.speakers = list(speakers)

    def __len__(self):
        return len(self.files)

    def describe(self, i):
        return '%s %.4f-%.4f (phone %s, speaker %s)' % (self.files[i], self.onsets[i], self.offsets[i],
                                                        self.phones[i], self.speakers[i])


def read_item_file(path):
    """Items of a ZeroSpeech 2017 item file (header line first, whitespace-separated, times in seconds)."""
    cols = [[] for _ in range(7)]
    with open(path) as f:
        header = f.readline().split()
        if len(header) < 7 or not header[0].startswith('#'):
            raise ValueError('%s: not an item file (header %r)' % (path, ' '.join(header)))
        for ln, line in enumerate(f, start=2):
            fields = line.split()
            if not fields:
                continue
            if len(fields) != 7:
                raise ValueError('%s:%d: expected 7 fields, got %d' % (path, ln, len(fields)))
            for c, v in zip(cols, fields):
                c.append(v)
    return Items(cols[0], [float(v) for v in cols[1]], [float(v) for v in cols[2]], *cols[3:])


# ---------------------------------------------------------------------------------------------------------------
# enumeration: cells, needed pairs, score rows

class Plan(object):
    """What a mode needs.  ``cells``: cell keys (phone labels, context, speaker key).  ``P``, ``Q``: item indices of the
    needed ordered pairs, each listed once, laid out so that every score row reads two contiguous ranges: d(A, X) over
    a cell's A for one X, and d(B, X) over its B.  Row r: (a_off, a_len, b_off, b_len, cell)."""

    def __init__(self, cells, P, Q, rows):
        self.cells = cells
        self.P = np.asarray(P, dtype=np.int64)
        self.Q = np.asarray(Q, dtype=np.int64)
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
        self.a_off, self.a_len, self.b_off, self.b_len, self.row_cell = (rows[:, k].copy() for k in range(5))


def enumerate_cells(phones, contexts, speakers, mode):
    """The Plan of `mode` for items with these labels (indices into the lists)."""
    if mode not in MODES:
        raise ValueError('mode must be one of %s, not %r' % (MODES, mode))
    cells, cell_id = [], {}
    P, Q, rows = [], [], []

    def cell(key):
        c = cell_id.get(key)
        if c is None:
            c = cell_id[key] = len(cells)
            cells.append(key)
        return c

    def segment(members, x, skip_x=False):
        off = len(P)
        P.extend([m for m in members if m != x] if skip_x else members)
        Q.extend([x] * (len(P) - off))
        return off, len(P) - off

    if mode == 'within':
        groups = defaultdict(lambda: defaultdict(list))       # (context, speaker) -> phone -> items
        for i, (p, c, s) in enumerate(zip(phones, contexts, speakers)):
            groups[(c, s)][p].append(i)
        for (c, s), byph in groups.items():
            if len(byph) < 2:
                continue
            for p, A in byph.items():
                if len(A) < 2:
                    continue
                ids = {q: cell((p, q, c, s)) for q in byph if q != p}
                for x in A:
                    ao, al = segment(A, x, skip_x=True)
                    for q, cid in ids.items():
                        bo, bl = segment(byph[q], x)
                        rows.append((ao, al, bo, bl, cid))
    else:
        groups = defaultdict(lambda: defaultdict(lambda: defaultdict(list)))    # context -> speaker -> phone -> items
        for i, (p, c, s) in enumerate(zip(phones, contexts, speakers)):
            groups[c][s][p].append(i)
        for c, byspk in groups.items():
            for s, phs in byspk.items():
                if len(phs) < 2:
                    continue
                for t, pht in byspk.items():
                    if t == s:
                        continue
                    for p, A in phs.items():
                        Xs = pht.get(p)
                        if not Xs:
                            continue
                        ids = {q: cell((p, q, c, (s, t))) for q in phs if q != p}
                        for x in Xs:
                            ao, al = segment(A, x)
                            for q, cid in ids.items():
                                bo, bl = segment(phs[q], x)
                                rows.append((ao, al, bo, bl, cid))
    return Plan(cells, P, Q, rows)


def aggregate(cells, score2, count):
    """(error in percent, {(p, q): score}, [cell scores]) from each cell's integer 2 x score sum and triplet count:
    cell means, then unweighted means over contexts, over speaker keys, over (p, q)."""
    score2 = np.asarray(score2, dtype=np.int64)
    count = np.asarray(count, dtype=np.int64)
    cell_score = [float(s2) / (2.0 * float(n)) for s2, n in zip(score2, count)]
    by_spk = defaultdict(list)                      # (p, q, speaker key) -> cell scores over contexts
    for (p, q, _c, sk), sc in zip(cells, cell_score):
        by_spk[(p, q, sk)].append(sc)
    by_pair = defaultdict(list)
    for (p, q, sk) in sorted(by_spk, key=repr):
        v = by_spk[(p, q, sk)]
        by_pair[(p, q)].append(sum(v) / len(v))
    pair_score = {k: sum(v) / len(v) for k, v in sorted(by_pair.items(), key=lambda kv: repr(kv[0]))}
    if not pair_score:
        return float('nan'), pair_score, cell_score
    S = sum(pair_score.values()) / len(pair_score)
    return 100.0 * (1.0 - S), pair_score, cell_score


# ---------------------------------------------------------------------------------------------------------------
# device work

def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _kl_triples(who, t1, t2):
    """ValueError unless t1 and t2 are (P, L, bad) as kl_tables returns them, on the device, of one frame width."""
    _lib.require_device(*(t1 + t2))
    for P_, L_, b_ in (t1, t2):
        if (P_.dim() != 2 or L_.shape != P_.shape or b_.shape != P_.shape[:1] or P_.dtype != torch.float32 or
                L_.dtype != torch.float32 or b_.dtype != torch.uint8 or
                not (P_.is_contiguous() and L_.is_contiguous() and b_.is_contiguous())):
            raise ValueError('%s: distance=\'kl\' takes (P, L, bad) as kl_tables returns them' % who)
    if t1[0].shape[1] != t2[0].shape[1]:
        raise ValueError('%s: the two sides have different frame widths' % who)


def _pair_table(who, rows1, off1, n1, rows2, off2, n2):
    """A pair table's columns, checked to lie inside tables of rows1 / rows2 rows: (host arrays, device tensors)."""
    off1, off2 = (np.ascontiguousarray(a, dtype=np.int64) for a in (off1, off2))
    n1, n2 = (np.ascontiguousarray(a, dtype=np.int32) for a in (n1, n2))
    if not (len(off1) == len(off2) == len(n2) == len(n1)):
        raise ValueError('%s: the pair table\'s columns differ in length' % who)
    if len(n1) and (n1.min() < 0 or n2.min() < 0 or off1.min() < 0 or off2.min() < 0 or
                    (off1 + n1).max() > rows1 or (off2 + n2).max() > rows2):
        raise ValueError('%s: a pair reads outside the feature tables' % who)
    cols = (off1, n1, off2, n2)
    return cols, [_dev(a, a.dtype) for a in cols]


def _beyond_cap(message, n, cap):
    long_ = np.flatnonzero(n > cap)
    if len(long_):
        raise ValueError(message % (long_[0], n[long_[0]], cap, len(long_)))


def kl_tables(table, floor=1e-6):
    """KLTables (P, L, bad) of the device feature table [rows, D] float32 (abn_kl_tables): P = max(table, floor),
    L = float32(log(float64(P))), bad[r] = 1 when row r holds a non-finite or a negative value."""
    floor = np.float32(floor)
    if not (floor > 0 and np.isfinite(floor)):
        raise ValueError('kl_tables: the floor must be a positive finite float32, not %r' % (floor,))
    lib = _lib.load()
    if table.dim() != 2 or table.dtype != torch.float32:
        raise ValueError('kl_tables: a [rows, D] float32 table is needed')
    table = table.contiguous()
    _lib.require_device(table)
    P, L = torch.empty_like(table), torch.empty_like(table)
    bad = torch.empty(table.shape[0], dtype=torch.uint8, device=table.device)
    if table.shape[0]:
        _lib.check(lib.abn_kl_tables(_lib.ptr(table), table.shape[0], table.shape[1], float(floor), _lib.ptr(P), _lib.ptr(L),
                                     _lib.ptr(bad), _lib.stream()), 'abn_kl_tables')
    return KLTables(P, L, bad)


PARALLEL = ('drop', 'zero')


def dtw_cost_batch(feats1, off1, n1, feats2, off2, n2, distance='cosine', parallel='drop'):
    """(total_cost float64, path_len int32) device tensors of pair p = rows [off1[p], off1[p]+n1[p]) of feats1 against
    [off2[p], off2[p]+n2[p]) of feats2.

    distance='cosine': feats* are [rows, D] float32 device tables; the result equals dtw_align_batch's:
    abn_dtw_cost_batched for every pair whose token 2 fits its cap (abn_dtw_cost_max_n2() frames), abn_dtw_batched
    (utils.dtw_align_batch) for the others.
    distance='kl': feats* are KLTables (or any (P, L, bad) triple) as kl_tables returns them;
    abn_dtw_cost_kl_batched.  A token 2 beyond the cap raises ValueError (there is no second kernel); a pair with a
    BAD row comes back with path_len = 0.
    parallel='zero' (cosine only): abn_dtw_cost_parallel_batched -- a cosine rounded beyond +-1 is distance 0 / 1, the
    pair is not dropped; it has no second kernel either, so a token 2 beyond the cap raises ValueError."""
    if distance not in DISTANCES:
        raise ValueError('distance must be one of %s, not %r' % (DISTANCES, distance))
    if parallel not in PARALLEL or (parallel == 'zero' and distance != 'cosine'):
        raise ValueError('parallel must be one of %s (\'zero\': distance=\'cosine\' only), not %r' % (PARALLEL, parallel))
    lib = _lib.load()
    kl = distance == 'kl'
    if kl:
        (feats1, L1, bad1), (feats2, L2, bad2) = feats1, feats2
        _kl_triples('dtw_cost_batch', (feats1, L1, bad1), (feats2, L2, bad2))
    else:
        _lib.require_tensor('dtw_cost_batch', 'feats1', feats1, torch.float32, 2)
        _lib.require_tensor('dtw_cost_batch', 'feats2', feats2, torch.float32, 2)
        if feats1.shape[1] != feats2.shape[1]:
            raise ValueError('dtw_cost_batch: the two sides have different frame widths')
    (off1, n1, off2, n2), d_tab = _pair_table('dtw_cost_batch', feats1.shape[0], off1, n1, feats2.shape[0], off2, n2)
    P = len(n1)
    cap = lib.abn_dtw_cost_max_n2()
    if kl:
        _beyond_cap('dtw_cost_batch: token 2 of pair %d has %d frames; distance=\'kl\' takes at most %d '
                    '(%d pair(s) beyond it)', n2, cap)
    if parallel == 'zero':
        _beyond_cap('dtw_cost_batch: token 2 of pair %d has %d frames; parallel=\'zero\' takes at most %d '
                    '(%d pair(s) beyond it)', n2, cap)
    cost = torch.empty(P, dtype=torch.float64, device=feats1.device)
    plen = torch.empty(P, dtype=torch.int32, device=feats1.device)
    if P == 0:
        return cost, plen
    tail = [_lib.ptr(t) for t in d_tab] + [P, feats1.shape[1]]
    out = [_lib.ptr(cost), _lib.ptr(plen), _lib.stream()]
    if kl:
        _lib.check(lib.abn_dtw_cost_kl_batched(_lib.ptr(feats1), _lib.ptr(L1), feats1.shape[0], _lib.ptr(feats2), _lib.ptr(L2),
                                               feats2.shape[0], *(tail + [_lib.ptr(bad1), _lib.ptr(bad2)] + out)),
                   'abn_dtw_cost_kl_batched')
        return cost, plen
    if parallel == 'zero':
        _lib.check(lib.abn_dtw_cost_parallel_batched(_lib.ptr(feats1), feats1.shape[0], _lib.ptr(feats2), feats2.shape[0],
                                                     *(tail + out)), 'abn_dtw_cost_parallel_batched')
        return cost, plen
    _lib.check(lib.abn_dtw_cost_batched(_lib.ptr(feats1), feats1.shape[0], _lib.ptr(feats2), feats2.shape[0], *(tail + out)),
               'abn_dtw_cost_batched')
    long_ = np.flatnonzero(n2 > cap)
    if len(long_):
        from .utils import dtw_align_batch
        res = dtw_align_batch(feats1, off1[long_], n1[long_], feats2, off2[long_], n2[long_])
        idx = torch.from_numpy(long_).to(feats1.device)
        cost[idx] = res.total_cost
        plen[idx] = res.path_len
    return cost, plen


def abx_score(dist, plan):
    """Per cell of `plan`: (2 x score sum, triplet count), int64 host arrays, from the device distances of plan's
    pairs (abn_abx_score)."""
    lib = _lib.load()
    nc = len(plan.cells)
    if not isinstance(dist, torch.Tensor) or dist.dtype != torch.float64 or dist.dim() != 1 or dist.numel() != len(plan.P):
        raise ValueError('abx_score: dist must be a float64 [%d] tensor, one distance per pair of the plan, not %s' % (
            len(plan.P), '%s %s' % (tuple(dist.shape), dist.dtype) if isinstance(dist, torch.Tensor) else type(dist).__name__))
    if not dist.is_cuda:
        raise _lib.HipLibraryError('abx_score: dist must be on the MI355X (HIP) device, not %s' % dist.device)
    score2 = torch.empty(nc, dtype=torch.int64, device=dist.device)
    count = torch.empty(nc, dtype=torch.int64, device=dist.device)
    refused = torch.empty(1, dtype=torch.int32, device=dist.device)
    dist = dist.contiguous()
    rows = [_dev(a, dt) for a, dt in ((plan.a_off, np.int64), (plan.a_len, np.int32), (plan.b_off, np.int64),
                                      (plan.b_len, np.int32), (plan.row_cell, np.int32))]
    _lib.check(lib.abn_abx_score(_lib.ptr(dist), dist.numel(), *[_lib.ptr(r) for r in rows], len(plan.a_off), nc,
                                 _lib.ptr(score2), _lib.ptr(count), _lib.ptr(refused), _lib.stream()), 'abn_abx_score')
    if int(refused.item()) != 0:
        raise RuntimeError('abn_abx_score refused %d rows of a plan this module built' % int(refused.item()))
    return score2.cpu().numpy(), count.cpu().numpy()


class ABXResult(object):
    """error: percent.  cells: [(key, n_triplets, score)] with key = (phone p, phone q, context, speaker key) --
    speaker key = speaker (within) or (speaker of A and B, speaker of X) (across).  by_phone_pair: {(p, q): score}.
    n_items (kept), n_pairs (DTW alignments), n_triplets, dropped: [(item index, description)].  distance: the frame
    distance of the alignments ('cosine' or 'kl')."""

    def __init__(self, mode, error, cells, by_phone_pair, n_items, n_pairs, n_triplets, dropped, distance='cosine'):
        self.mode, self.error, self.cells, self.by_phone_pair = mode, error, cells, by_phone_pair
        self.n_items, self.n_pairs, self.n_triplets, self.dropped = n_items, n_pairs, n_triplets, dropped
        self.distance = distance

    def __repr__(self):
        return ('ABXResult(%s, %s: error %.4f %%, %d cells, %d items, %d pairs, %d triplets, %d dropped)'
                % (self.mode, self.distance, self.error, len(self.cells), self.n_items, self.n_pairs, self.n_triplets,
                   len(self.dropped)))


def _read_h5features(path):
    try:
        import h5features
    except ImportError:
        raise ImportError('ABXEvaluator reads h5features files like the reference; the h5features package is '
                          'not installed. Pass a DeviceCorpus or in-memory features and times instead.')
    with h5features.Reader(path, 'features') as fh:
        data = fh.read()
    return dict(zip(data.items(), data.features())), dict(zip(data.items(), data.labels()))


class ABXEvaluator(object):
    """ABX error of the embeddings in `corpus` on the items of `items`.

    items: an Items (read_item_file) or the path of an item file.
    corpus: a DeviceCorpus (e.g. ``DeviceCorpus.from_table(embedder.embed_table(table), names, lengths, times)``),
    a {name: [T, D]} features dict together with `times` ({name: [T] frame times in seconds}), or the path of an
    h5features file (needs the h5features package).
    distance: 'cosine' (embeddings) or 'kl' (posteriorgrams: the symmetrised Kullback-Leibler divergence over the
    tables of kl_tables(corpus.table, floor), built here once and kept for every run).
    parallel: 'drop' (default, the reference's rule: identical or parallel frames whose cosine rounds above 1 drop the
    pair, which raises) or 'zero' (such frames are at distance 0: for quantised corpora; cosine only)."""

    def __init__(self, items, corpus, times=None, distance='cosine', floor=1e-6, parallel='drop'):
        if distance not in DISTANCES:
            raise ValueError('distance must be one of %s, not %r' % (DISTANCES, distance))
        if parallel not in PARALLEL or (parallel == 'zero' and distance != 'cosine'):
            raise ValueError('parallel must be one of %s (\'zero\': distance=\'cosine\' only), not %r' % (PARALLEL, parallel))
        self.parallel = parallel
        from .dataloader import DeviceCorpus
        self.distance = distance
        self.items = read_item_file(items) if isinstance(items, str) else items
        if isinstance(corpus, str):
            corpus, times = _read_h5features(corpus)
        if not isinstance(corpus, DeviceCorpus):
            if times is None:
                raise ValueError('ABXEvaluator: a features dict needs its times dict')
            corpus = DeviceCorpus(corpus, times)
        self.corpus = corpus
        self.row = np.zeros(len(self.items), dtype=np.int64)
        self.n = np.zeros(len(self.items), dtype=np.int32)
        for i in range(len(self.items)):
            r, n = corpus.token(self.items.files[i], self.items.onsets[i], self.items.offsets[i])
            self.row[i], self.n[i] = r, n
        self.kept = np.flatnonzero(self.n > 0)
        self.dropped = [(int(i), self.items.describe(i)) for i in np.flatnonzero(self.n == 0)]
        self.tables = kl_tables(corpus.table, floor) if distance == 'kl' else None

    def plan(self, mode):
        k = self.kept
        it = self.items
        return enumerate_cells([it.phones[i] for i in k], [it.contexts[i] for i in k], [it.speakers[i] for i in k],
                               mode)

    def distances(self, plan):
        """d(P, Q) of every needed pair of `plan` (float64, device)."""
        P, Q = self.kept[plan.P], self.kept[plan.Q]
        t = self.tables if self.distance == 'kl' else self.corpus.table
        cost, plen = dtw_cost_batch(t, self.row[P], self.n[P], t, self.row[Q], self.n[Q], distance=self.distance,
                                    parallel=self.parallel)
        ln = plen.cpu().numpy()
        bad = np.flatnonzero(ln <= 0)
        if len(bad):
            b = bad[0]
            why = ('a frame with a non-finite or negative value' if self.distance == 'kl' else
                   'a NaN frame distance: identical or parallel frames, or non-finite values')
            raise ValueError('ABX: the alignment of item %d (%s) with item %d (%s) was dropped (%s); %d pair(s) in all'
                             % (P[b], self.items.describe(P[b]), Q[b], self.items.describe(Q[b]), why, len(bad)))
        return cost / plen.to(torch.float64)

    def run(self, mode='within'):
        plan = self.plan(mode)
        if len(plan.cells):
            dist = self.distances(plan)
            score2, count = abx_score(dist, plan)
        else:
            score2 = count = np.zeros(0, dtype=np.int64)
        error, by_pair, cell_score = aggregate(plan.cells, score2, count)
        cells = [(key, int(n), sc) for key, n, sc in zip(plan.cells, count, cell_score)]
        return ABXResult(mode, error, cells, by_pair, len(self.kept), len(plan.P), int(count.sum()), self.dropped,
                         self.distance)


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m abnet3_amd.abx', description='ABX error of embeddings (ZeroSpeech 2017 items)')
    ap.add_argument('features', help='h5features file of the embeddings')
    ap.add_argument('items', help='item file (#file onset offset #phone prev-phone next-phone speaker)')
    ap.add_argument('--mode', choices=MODES + ('both',), default='both')
    ap.add_argument('--distance', choices=DISTANCES, default='cosine',
                    help="frame distance: 'cosine' (embeddings) or 'kl' (posteriorgrams, symmetrised Kullback-Leibler)")
    ap.add_argument('--floor', type=float, default=1e-6, help="floor of the probabilities under --distance kl")
    args = ap.parse_args(argv)
    ev = ABXEvaluator(args.items, args.features, distance=args.distance, floor=args.floor)
    for mode in (MODES if args.mode == 'both' else (args.mode,)):
        r = ev.run(mode)
        print('%s-speaker ABX error: %.3f %% (%d cells, %d triplets, %d items, %d dropped)'
              % (mode, r.error, len(r.cells), r.n_triplets, r.n_items, len(r.dropped)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
