"""Unsupervised pair discovery on the MI355X: a k-nearest-neighbour search over fixed-size segment vectors that
writes the pairs file PairsDataLoader reads.  No labels at any point:
features -> KnnPairMiner -> PairsDataLoader -> train -> embed -> ABX.

    python -m abnet3_amd.discovery FEATURES OUT_DIR [--lengths 40,60,80] [--shift 5] [--frames 10] [-k 10]
                                   [--min-similarity 0] [--no-mutual] [--max-pairs N]

The definition this module computes:

* Input: a DeviceCorpus, a {name: [T, D]} features dict with its times dict, or the path of an h5features file.
* Segments: for each file of n frames, for each L in `lengths` (default (40, 60, 80)), every start
  s = 0, shift, 2 shift, ... with s + L <= n (default shift = 5).  Files are numbered in sorted name order;
  segments are numbered file-major, then by L (in the order given), then by s.
* Segment vector: the K frames (default 10) at t_j = s + ((2j + 1) L) // (2K), j = 0 .. K - 1, concatenated to K D
  floats and L2-normalised (sum of squares in float64, scale applied in fp32: `abn_segment_vectors`).  An all-zero
  segment is left out (the remaining segments keep their order and are renumbered).
* Neighbours: for every segment the k (default 10) segments of largest cosine similarity, fp32 on the matrix
  cores (`abn_knn_topk`), among those that do not overlap it: same file and intersecting frame intervals
  [s, s + L) are excluded, the segment itself included.  Sorted by descending similarity, ties by ascending number.
* Pairs: the unordered pair {a < b} exists when b is in a's list or a in b's; with mutual=True (default) only when
  both hold.  Its similarity is the one in a's list when b is there, else the one in b's list.  Pairs with
  similarity < min_similarity (default 0) are dropped; the rest is sorted by descending similarity, then (a, b),
  and truncated to max_pairs when given.
* Output: OUT_DIR/pairs_knn.txt, one line `id1 id2 b1 e1 b2 e2 dist` per pair with dist = 1 - sim printed %.11f,
  b = s and e = s + L: the end is EXCLUSIVE, because the loader reads a token as features[file][b:e]
  (DeviceCorpus.token_frames); OUT_DIR/id_to_file.txt, `id name` per line.  These are what
  PairsDataLoader(pairs_path, features_path, id_to_file) reads back.

The candidates table is materialised once (n_segments x K D floats); the queries go through the search in chunks of
`query_chunk` rows so that the lists' workspace stays bounded.  The n x n similarities never exist in memory.
"""
import argparse
import os
import sys

import numpy as np
import torch

from . import _lib

DEFAULT_LENGTHS = (40, 60, 80)


def enumerate_segments(n_frames, lengths=DEFAULT_LENGTHS, shift=5):
    """(file, begin, length) int32 arrays of every segment of files with `n_frames[f]` frames, in the module's order."""
    if shift < 1 or any(L < 1 for L in lengths):
        raise ValueError('shift and lengths must be positive')
    files, begins, lens = [], [], []
    for f, n in enumerate(n_frames):
        for L in lengths:
            if n >= L:
                s = np.arange(0, n - L + 1, shift, dtype=np.int32)
                files.append(np.full(len(s), f, dtype=np.int32))
                begins.append(s)
                lens.append(np.full(len(s), L, dtype=np.int32))
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=np.int32)
    return cat(files), cat(begins), cat(lens)


def segment_vectors(table, row0, seg_len, K=10):
    """abn_segment_vectors: ([n, K D] float32 unit rows, [n] bool "not all zero") on table's device for the segments
    that start at table rows `row0` (host int64) and are `seg_len` (host int32) rows long."""
    _lib.require_tensor('segment_vectors', 'table', table, torch.float32, 2)
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
        raise ValueError('segment_vectors: K = %r, a positive number of frames is needed' % (K,))
    K = int(K)
    row0 = np.ascontiguousarray(row0, dtype=np.int64)
    seg_len = np.ascontiguousarray(seg_len, dtype=np.int32)
    if row0.ndim != 1 or seg_len.shape != row0.shape:
        raise ValueError('segment_vectors: row0 and seg_len must be two 1-d arrays of one length')
    n, D = len(row0), table.shape[1]
    if n and (row0.min() < 0 or seg_len.min() < 1 or (row0 + seg_len).max() > table.shape[0]):
        raise ValueError('segment_vectors: a segment lies outside the table')
    out = torch.empty(n, K * D, dtype=torch.float32, device=table.device)
    keep = torch.empty(n, dtype=torch.uint8, device=table.device)
    d_row0, d_len = torch.from_numpy(row0).to(table.device), torch.from_numpy(seg_len).to(table.device)
    _lib.check(_lib.load().abn_segment_vectors(_lib.ptr(table), D, _lib.ptr(d_row0), _lib.ptr(d_len), n, K,
                                               _lib.ptr(out), _lib.ptr(keep), _lib.stream()), 'abn_segment_vectors')
    return out, keep.bool()


def knn_topk(Q, C, k, q_meta=None, c_meta=None):
    """abn_knn_topk: (idx int32 [nq, k], sim float32 [nq, k]) on the device.  Q [nq, d], C [nc, d]: unit rows;
    q_meta / c_meta: int32 [n, 3] device tensors (file, begin, end) for the overlap exclusion, or None."""
    _lib.require_tensor('knn_topk', 'Q', Q, torch.float32, 2)
    _lib.require_tensor('knn_topk', 'C', C, torch.float32, 2)
    _lib.require_device(q_meta, c_meta)
    # (k > nc is legal: the places beyond the candidates hold idx = -1, sim = -inf; the upper limit is the library's)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError('knn_topk: k = %r, a positive number of neighbours is needed' % (k,))
    k = int(k)
    lib = _lib.load()
    nq, nc, d = Q.shape[0], C.shape[0], Q.shape[1]
    if C.shape[1] != d:
        raise ValueError('knn_topk: Q has %d columns, C %d' % (d, C.shape[1]))
    for m, n in ((q_meta, nq), (c_meta, nc)):
        if m is not None and (m.dtype != torch.int32 or tuple(m.shape) != (n, 3)):
            raise ValueError('knn_topk: meta must be int32 [n, 3]')
    idx = torch.empty(nq, k, dtype=torch.int32, device=Q.device)
    sim = torch.empty(nq, k, dtype=torch.float32, device=Q.device)
    need = lib.abn_knn_ws_bytes(nq, nc, k)
    ws = torch.empty(max(need, 0), dtype=torch.uint8, device=Q.device) if need > 0 else None
    _lib.check(lib.abn_knn_topk(_lib.ptr(Q), nq, _lib.ptr(C), nc, d, _lib.ptr(q_meta), _lib.ptr(c_meta), k, _lib.ptr(idx),
                                _lib.ptr(sim), _lib.ptr(ws), max(need, 0), _lib.stream()), 'abn_knn_topk')
    return idx, sim


def pairs_from_lists(idx, sim, min_similarity=0.0, mutual=True, max_pairs=None):
    """The module's pair list from neighbour lists (host arrays idx [n, k] with -1 for unused places, sim [n, k]):
    (a, b, similarity) arrays with a < b, by descending similarity, then (a, b)."""
    idx = np.asarray(idx, dtype=np.int64)
    sim = np.asarray(sim)
    n = idx.shape[0]
    i = np.repeat(np.arange(n, dtype=np.int64), idx.shape[1])
    j, s = idx.ravel(), sim.ravel()
    used = j >= 0
    i, j, s = i[used], j[used], s[used]
    has_reverse = np.isin(j * n + i, i * n + j)
    forward = i < j                        # the entry of a's list: it carries the pair's similarity
    take = (forward & has_reverse) if mutual else (forward | ~has_reverse)
    a, b, s = np.minimum(i, j)[take], np.maximum(i, j)[take], s[take]
    ok = s >= min_similarity
    a, b, s = a[ok], b[ok], s[ok]
    order = np.lexsort((b, a, -s.astype(np.float64)))
    if max_pairs is not None:
        order = order[:max_pairs]
    return a[order], b[order], s[order]


def write_pairs(out_dir, names, seg_file, seg_begin, seg_len, a, b, sim):
    """pairs_knn.txt and id_to_file.txt of the module docstring; returns their paths."""
    os.makedirs(out_dir, exist_ok=True)
    pairs_path, map_path = os.path.join(out_dir, 'pairs_knn.txt'), os.path.join(out_dir, 'id_to_file.txt')
    with open(pairs_path, 'w') as fh:
        for x, y, s in zip(a.tolist(), b.tolist(), np.asarray(sim, dtype=np.float64).tolist()):
            fh.write('%d %d %d %d %d %d %.11f\n' % (seg_file[x], seg_file[y], seg_begin[x], seg_begin[x] + seg_len[x],
                                                    seg_begin[y], seg_begin[y] + seg_len[y], 1.0 - s))
    with open(map_path, 'w') as fh:
        for f, name in enumerate(names):
            fh.write('%d %s\n' % (f, name.decode('UTF-8') if isinstance(name, bytes) else name))
    return pairs_path, map_path


def _read_h5features(path):
    try:
        import h5features
    except ImportError:
        raise ImportError('KnnPairMiner reads h5features files like the loaders; the h5features package is not '
                          'installed. Pass a DeviceCorpus or in-memory features and times instead.')
    with h5features.Reader(path, 'features') as fh:
        data = fh.read()
    return data.dict_features(), data.dict_labels()


class KnnPairMiner(object):
    """Discovers word-like pairs in `corpus` (module docstring).  corpus: a DeviceCorpus, a {name: [T, D]} dict
    together with `times`, or an h5features path.  After mine(): seg_file / seg_begin / seg_len (the kept segments),
    idx / sim (their neighbour lists, host), pairs = (a, b, similarity)."""

    def __init__(self, corpus, times=None, lengths=DEFAULT_LENGTHS, shift=5, frames=10, k=10, min_similarity=0.0,
                 mutual=True, max_pairs=None, query_chunk=1 << 16):
        from .dataloader import DeviceCorpus
        if isinstance(corpus, str):
            corpus, times = _read_h5features(corpus)
        if not isinstance(corpus, DeviceCorpus):
            if times is None:
                raise ValueError('KnnPairMiner: a features dict needs its times dict')
            corpus = DeviceCorpus(corpus, times)
        if (frames * corpus.dim) % 4:
            raise ValueError('KnnPairMiner: frames x feature dimension = %d must be a multiple of 4' % (frames * corpus.dim))
        self.corpus = corpus
        self.lengths, self.shift, self.frames, self.k = tuple(lengths), shift, frames, k
        self.min_similarity, self.mutual, self.max_pairs, self.query_chunk = min_similarity, mutual, max_pairs, query_chunk
        self.names = sorted(corpus.names, key=lambda n: n.decode('UTF-8') if isinstance(n, bytes) else str(n))

    def vectors(self):
        """Enumerates the segments and builds the table of their unit vectors, all-zero segments left out."""
        c = self.corpus
        f, b, L = enumerate_segments([c.length[n] for n in self.names], self.lengths, self.shift)
        base = np.array([c.offset[n] for n in self.names], dtype=np.int64)
        row0 = (base[f] if len(f) else np.zeros(0, dtype=np.int64)) + b
        vec, keep = segment_vectors(c.table, row0, L, self.frames)
        keep_h = keep.cpu().numpy()
        if not keep_h.all():
            vec = vec[keep].contiguous()
            f, b, L = f[keep_h], b[keep_h], L[keep_h]
        self.seg_file, self.seg_begin, self.seg_len = f, b, L
        self.table = vec
        self.meta = torch.from_numpy(np.stack([f, b, b + L], axis=1).astype(np.int32)).to(vec.device).contiguous()
        return vec

    def neighbours(self):
        """The neighbour lists of every kept segment (host arrays), the queries in chunks."""
        n = self.table.shape[0]
        idx = np.full((n, self.k), -1, dtype=np.int32)
        sim = np.full((n, self.k), -np.inf, dtype=np.float32)
        for q0 in range(0, n, self.query_chunk):
            q1 = min(n, q0 + self.query_chunk)
            i, s = knn_topk(self.table[q0:q1], self.table, self.k, self.meta[q0:q1], self.meta)
            idx[q0:q1], sim[q0:q1] = i.cpu().numpy(), s.cpu().numpy()
        self.idx, self.sim = idx, sim
        return idx, sim

    def mine(self):
        self.vectors()
        if self.table.shape[0] == 0:
            self.idx, self.sim = np.zeros((0, self.k), dtype=np.int32), np.zeros((0, self.k), dtype=np.float32)
        else:
            self.neighbours()
        self.pairs = pairs_from_lists(self.idx, self.sim, self.min_similarity, self.mutual, self.max_pairs)
        return self.pairs

    def write(self, out_dir):
        """Mines (if mine() has not run) and writes OUT_DIR/pairs_knn.txt and OUT_DIR/id_to_file.txt; returns
        their paths."""
        if not hasattr(self, 'pairs'):
            self.mine()
        return write_pairs(out_dir, self.names, self.seg_file, self.seg_begin, self.seg_len, *self.pairs)


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m abnet3_amd.discovery',
                                 description='k-nearest-neighbour pair discovery over segment vectors')
    ap.add_argument('features', help='h5features file')
    ap.add_argument('out_dir')
    ap.add_argument('--lengths', default=','.join(str(v) for v in DEFAULT_LENGTHS), help='segment lengths in frames')
    ap.add_argument('--shift', type=int, default=5)
    ap.add_argument('--frames', type=int, default=10, help='frames sampled per segment (K)')
    ap.add_argument('-k', type=int, default=10, help='neighbours per segment')
    ap.add_argument('--min-similarity', type=float, default=0.0)
    ap.add_argument('--no-mutual', action='store_true')
    ap.add_argument('--max-pairs', type=int, default=None)
    args = ap.parse_args(argv)
    miner = KnnPairMiner(args.features, lengths=[int(v) for v in args.lengths.split(',')], shift=args.shift,
                         frames=args.frames, k=args.k, min_similarity=args.min_similarity, mutual=not args.no_mutual,
                         max_pairs=args.max_pairs)
    pairs_path, map_path = miner.write(args.out_dir)
    print('%d segments, %d pairs -> %s, %s' % (miner.table.shape[0], len(miner.pairs[0]), pairs_path, map_path))
    return 0


if __name__ == '__main__':
    sys.exit(main())
