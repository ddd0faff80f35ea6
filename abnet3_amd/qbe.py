"""Query-by-example search (spoken term detection) over embeddings or posteriorgrams on the MI355X.

    python -m abnet3_amd.qbe FEATURES QUERIES [--distance cosine|kl] [--floor F] [--top K]

The definition this module computes (tests/qbe_np.py restates it in numpy; the SEARCH mode of csrc/dtw_wave.h is the kernel):

* A pair is a query Q of M frames and an utterance U of N frames.  A path consumes ALL of Q and ANY contiguous run of
  U (subsequence DTW).  Cell (i, j) pairs utterance frame i with query frame j.
* Cells are the project's frame distances, as float32, unchanged: ``distance='cosine'`` the angular cosine distance of
  csrc/dist_ref.h (the cell of ``abn_dtw_batched`` / ``abn_dtw_cost_batched``; an all-zero frame is at distance 1
  from every other frame and 0 from another zero frame), ``distance='kl'`` the symmetrised Kullback-Leibler
  divergence over the tables of ``abx.kl_tables`` (the cell of ``abn_dtw_cost_kl_batched``).  The search adds:
  - a cosine cell that comes out NaN while the dot product is finite and the (float32) product of the two norms is
    finite and non-zero is a rounding of |cos| above 1: d = 0 for dot > 0 (parallel frames), d = 1 for dot < 0;
  - any other NaN cell is BLOCKED: d = +inf.  A KL cell that touches a BAD row (``kl_tables``) is blocked too;
  - the zero-frame rule is the cell's own and comes first: an all-zero frame is at distance 1 from ANY other frame,
    a non-finite one included (that cell is not NaN, so it is not blocked);
  - a pair is never dropped as a whole (ABX drops it): a query cut out of the corpus has to find itself, and one
    bad frame must not hide an utterance.  Paths go round blocked cells.
* Recurrence, in float64: C(i, j) = d(i, j) + min(diag, up, left) with diag = C(i-1, j-1), up = C(i-1, j),
  left = C(i, j-1); the first minimum wins in the order diag, up, left (the existing kernels' rule); the path length
  and the start frame are carried along the chosen predecessor.  The free start: for EVERY utterance frame i the
  virtual cell (i-1, -1) has cost 0, length 0 and start i -- so C(i, 0) = d(i, 0) or d(i, 0) + C(i-1, 0) -- and there is
  no left predecessor in query column 0.  Cells outside the matrix cost +inf.
* Result per pair: among the utterance frames i with finite C(i, M-1), the FIRST that minimises
  C(i, M-1) / len(i, M-1) (float64 division): ``total_cost``, ``path_len``, ``start``, ``end`` = i, utterance-relative
  and inclusive.  No finite end: path_len = 0, start = end = -1, cost 0; the same for an empty query or utterance.
  A pair outside the tables, a negative length or a query beyond the cap (``abn_dtw_search_max_query()`` = 256
  frames; the utterance is unbounded): path_len = -1 and nothing is read.
* Profile (optional): for every utterance frame i of every pair, C(i, M-1), len, start -- what peak picking for several
  detections per recording needs; +inf, 0, -1 where C(i, M-1) is not finite (and for every frame under an empty query).

``QbeSearcher`` ranks the utterances of a corpus for each query by score = total_cost / path_len (+inf: no detection).
"""
import argparse
import sys
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .abx import DISTANCES, _beyond_cap, _dev, _kl_triples, _pair_table, _read_h5features, kl_tables

# the per-frame output of subsequence_dtw_batch(profile=True): entry offset[p] + i is utterance frame i of pair p
Profile = namedtuple('Profile', ['cost', 'len', 'start', 'offset'])


def max_query():
    """The longest query, in frames, the kernel takes."""
    return int(_lib.load().abn_dtw_search_max_query())


def subsequence_dtw_batch(q, q_off, q_n, u, u_off, u_n, distance='cosine', profile=False):
    """(total_cost float64, path_len int32, start int32, end int32[, Profile]) device tensors of pair p = query rows
    [q_off[p], q_off[p]+q_n[p]) of q searched in utterance rows [u_off[p], u_off[p]+u_n[p]) of u (module docstring).

    distance='cosine': q and u are [rows, D] float32 device tables (abn_dtw_search_batched).
    distance='kl': q and u are KLTables (or any (P, L, bad) triple) as abx.kl_tables returns them
    (abn_dtw_search_kl_batched).  A query of more than max_query() frames raises ValueError."""
    if distance not in DISTANCES:
        raise ValueError('distance must be one of %s, not %r' % (DISTANCES, distance))
    lib = _lib.load()
    kl = distance == 'kl'
    if kl:
        (q, Lq, badq), (u, Lu, badu) = q, u
        _kl_triples('subsequence_dtw_batch', (q, Lq, badq), (u, Lu, badu))
    else:
        _lib.require_device(q, u)
        if q.dim() != 2 or u.dim() != 2 or q.dtype != torch.float32 or u.dtype != torch.float32:
            raise ValueError('subsequence_dtw_batch: [rows, D] float32 tables are needed')
        if q.shape[1] != u.shape[1]:
            raise ValueError('subsequence_dtw_batch: the two sides have different frame widths')
    (u_off, u_n, q_off, q_n), d_tab = _pair_table('subsequence_dtw_batch', u.shape[0], u_off, u_n, q.shape[0], q_off, q_n)
    P = len(q_n)
    _beyond_cap('subsequence_dtw_batch: the query of pair %d has %d frames; at most %d are taken (%d pair(s) beyond it)',
                q_n, lib.abn_dtw_search_max_query())
    dev = u.device
    cost = torch.empty(P, dtype=torch.float64, device=dev)
    plen, start, end = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))
    prof = None
    if profile:
        off = np.zeros(P + 1, dtype=np.int64)
        np.cumsum(u_n, out=off[1:])
        rows = int(off[-1])
        prof = Profile(torch.empty(rows, dtype=torch.float64, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
                       torch.empty(rows, dtype=torch.int32, device=dev), off[:-1].copy())
    if P:
        table = [_lib.ptr(t) for t in d_tab] + [P, u.shape[1]]
        d_poff = _dev(prof.offset, np.int64) if profile else None
        tail = [_lib.ptr(cost), _lib.ptr(plen), _lib.ptr(start), _lib.ptr(end), _lib.ptr(d_poff),
                prof.cost.numel() if profile else 0, _lib.ptr(prof.cost if profile else None),
                _lib.ptr(prof.len if profile else None), _lib.ptr(prof.start if profile else None), _lib.stream()]
        if kl:
            _lib.check(lib.abn_dtw_search_kl_batched(_lib.ptr(u), _lib.ptr(Lu), u.shape[0], _lib.ptr(q), _lib.ptr(Lq), q.shape[0],
                                                     *(table + [_lib.ptr(badu), _lib.ptr(badq)] + tail)),
                       'abn_dtw_search_kl_batched')
        else:
            _lib.check(lib.abn_dtw_search_batched(_lib.ptr(u), u.shape[0], _lib.ptr(q), q.shape[0], *(table + tail)),
                       'abn_dtw_search_batched')
    return (cost, plen, start, end, prof) if profile else (cost, plen, start, end)


class QbeResult(object):
    """Arrays [Q, U] (queries x utterances): score = total_cost / path_len (float64, +inf: no detection), start_frame /
    end_frame (int32, utterance-relative, inclusive, -1: none), start_time / end_time (the corpus' frame times of those
    frames, NaN: none).  queries: the [(file, onset, offset)] searched; utterances: the corpus names searched."""

    def __init__(self, queries, utterances, score, start_frame, end_frame, start_time, end_time):
        self.queries, self.utterances = queries, utterances
        self.score, self.start_frame, self.end_frame = score, start_frame, end_frame
        self.start_time, self.end_time = start_time, end_time

    def ranking(self, q):
        """Utterance indices of query q, best first (a stable sort: ties in corpus order)."""
        return np.argsort(self.score[q], kind='stable')

    def __repr__(self):
        return 'QbeResult(%d queries x %d utterances, %d detections)' % (
            self.score.shape[0], self.score.shape[1], int(np.isfinite(self.score).sum()))


class QbeSearcher(object):
    """Searches the utterances of `corpus` for spoken queries.

    corpus: a DeviceCorpus (e.g. ``DeviceCorpus.from_table(embedder.embed_table(table), names, lengths, times)``), a
    {name: [T, D]} features dict together with `times`, or the path of an h5features file (needs h5features).
    distance: 'cosine' (embeddings) or 'kl' (posteriorgrams; the tables of kl_tables(corpus.table, floor) are built
    once).  chunk_pairs: how many (query, utterance) pairs one launch takes -- Q x U need not fit at once."""

    def __init__(self, corpus, times=None, distance='cosine', floor=1e-6, chunk_pairs=1 << 18):
        if distance not in DISTANCES:
            raise ValueError('distance must be one of %s, not %r' % (DISTANCES, distance))
        if chunk_pairs < 1:
            raise ValueError('chunk_pairs must be positive')
        self.distance, self.floor, self.chunk_pairs = distance, floor, int(chunk_pairs)
        self.corpus = self._corpus(corpus, times)
        self.tables = kl_tables(self.corpus.table, floor) if distance == 'kl' else None

    @staticmethod
    def _corpus(corpus, times):
        from .dataloader import DeviceCorpus
        if isinstance(corpus, str):
            corpus, times = _read_h5features(corpus)
        if not isinstance(corpus, DeviceCorpus):
            if times is None:
                raise ValueError('QbeSearcher: a features dict needs its times dict')
            corpus = DeviceCorpus(corpus, times)
        return corpus

    def search(self, queries, query_corpus=None, utterances=None, query_times=None):
        """QbeResult of `queries` = [(file, onset, offset)] -- tokens of `query_corpus` (default: the searched corpus
        itself) -- against `utterances` (names of the corpus; default: all of them, in corpus order)."""
        queries = [tuple(q) for q in queries]
        qc = self.corpus if query_corpus is None else self._corpus(query_corpus, query_times)
        if qc.dim != self.corpus.dim:
            raise ValueError('QbeSearcher: queries have %d values per frame, the corpus %d' % (qc.dim, self.corpus.dim))
        names = list(self.corpus.names) if utterances is None else [self.corpus._name(u) for u in utterances]
        tok = np.array([qc.token(f, on, off) for f, on, off in queries], dtype=np.int64).reshape(-1, 2)
        cap = max_query()
        for (f, on, off), n in zip(queries, tok[:, 1]):
            if n > cap:
                raise ValueError('QbeSearcher: query %s %.4f-%.4f has %d frames; at most %d are taken' % (f, on, off, n, cap))
        u_row = np.array([self.corpus.offset[k] for k in names], dtype=np.int64)
        u_len = np.array([self.corpus.length[k] for k in names], dtype=np.int32)
        if self.distance == 'kl':
            ut = self.tables
            qt = ut if qc is self.corpus else kl_tables(qc.table, self.floor)
        else:
            ut, qt = self.corpus.table, qc.table
        Q, U = len(queries), len(names)
        cost = np.zeros(Q * U, dtype=np.float64)
        plen, start, end = (np.zeros(Q * U, dtype=np.int32) for _ in range(3))
        for lo in range(0, Q * U, self.chunk_pairs):                # pair lo + k = (query (lo + k) // U, utterance (lo + k) % U)
            idx = np.arange(lo, min(Q * U, lo + self.chunk_pairs))
            qi, ui = idx // U, idx % U
            out = subsequence_dtw_batch(qt, tok[qi, 0], tok[qi, 1], ut, u_row[ui], u_len[ui], distance=self.distance)
            for dst, t in zip((cost, plen, start, end), out):
                dst[idx] = t.cpu().numpy()
        if (plen < 0).any():
            raise RuntimeError('the search kernel refused %d pairs of a table this module built' % int((plen < 0).sum()))
        found = plen > 0
        score = np.full(Q * U, np.inf)
        score[found] = cost[found] / plen[found].astype(np.float64)
        st, et = np.full(Q * U, np.nan), np.full(Q * U, np.nan)
        for k in np.flatnonzero(found):
            t = self.corpus.times[names[k % U]]
            st[k], et[k] = t[start[k]], t[end[k]]
        shape = (Q, U)
        return QbeResult(queries, names, score.reshape(shape), start.reshape(shape), end.reshape(shape),
                         st.reshape(shape), et.reshape(shape))


def _ranked_relevance(score, relevant):
    score = np.asarray(score, dtype=np.float64)
    relevant = np.asarray(relevant, dtype=bool)
    if score.ndim != 2 or score.shape != relevant.shape:
        raise ValueError('score and relevant must be [Q, U] arrays of the same shape')
    order = np.argsort(score, axis=1, kind='stable')                # ascending: best first; ties in column order
    return np.take_along_axis(relevant, order, axis=1)


def mean_average_precision(score, relevant):
    """The mean over the queries that have a relevant utterance of the average precision of their ranking by ascending
    score (host numpy; `relevant`: boolean [Q, U]).  NaN when no query has one."""
    rel = _ranked_relevance(score, relevant)
    ap = []
    for r in rel:
        hits = np.flatnonzero(r)
        if len(hits):
            ap.append(float(np.mean(np.arange(1, len(hits) + 1) / (hits + 1.0))))
    return float(np.mean(ap)) if ap else float('nan')


def precision_at_n(score, relevant):
    """The mean over the queries that have a relevant utterance of the share of relevant ones among their best N, N being
    the query's own number of relevant utterances (host numpy).  NaN when no query has one."""
    rel = _ranked_relevance(score, relevant)
    p = [float(r[:int(r.sum())].mean()) for r in rel if r.any()]
    return float(np.mean(p)) if p else float('nan')


def read_query_file(path):
    """[(file, onset, offset)] of a query list: one query per line, whitespace-separated, times in seconds; lines that
    start with # are comments."""
    out = []
    with open(path) as f:
        for ln, line in enumerate(f, start=1):
            fields = line.split()
            if not fields or fields[0].startswith('#'):
                continue
            if len(fields) < 3:
                raise ValueError('%s:%d: expected file onset offset' % (path, ln))
            out.append((fields[0], float(fields[1]), float(fields[2])))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m abnet3_amd.qbe',
                                 description='Query-by-example search: where in the corpus does each query occur?')
    ap.add_argument('features', help='h5features file of the corpus (embeddings or posteriorgrams; needs the h5features package)')
    ap.add_argument('queries', help='query list: lines of `file onset offset` naming stretches of the corpus')
    ap.add_argument('--distance', choices=DISTANCES, default='cosine',
                    help="frame distance: 'cosine' (embeddings) or 'kl' (posteriorgrams, symmetrised Kullback-Leibler)")
    ap.add_argument('--floor', type=float, default=1e-6, help='floor of the probabilities under --distance kl')
    ap.add_argument('--top', type=int, default=5, help='detections printed per query')
    args = ap.parse_args(argv)
    queries = read_query_file(args.queries)
    res = QbeSearcher(args.features, distance=args.distance, floor=args.floor).search(queries)
    for q, (f, on, off) in enumerate(queries):
        print('%s %.3f-%.3f' % (f, on, off))
        for u in res.ranking(q)[:args.top]:
            if not np.isfinite(res.score[q, u]):
                break
            name = res.utterances[u]
            print('  %-24s %.3f-%.3f  score %.6f' % (name.decode() if isinstance(name, bytes) else name,
                                                    res.start_time[q, u], res.end_time[q, u], res.score[q, u]))
    return 0


if __name__ == '__main__':
    sys.exit(main())
