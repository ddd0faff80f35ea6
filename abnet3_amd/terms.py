"""Spoken-term discovery on the MI355X: local-alignment (segmental) DTW of every utterance against every other, the
matching stretches clustered into the `.classes` file SamplerClusterSiamese reads.  No labels at any point:
features -> (GmmPosteriorgram) -> TermDiscoverer -> .classes -> SamplerClusterSiamese -> train -> embed -> ABX / QbE.

    python -m abnet3_amd.terms FEATURES OUT_DIR [--distance cosine|kl] [--floor F] [--theta T] [--min-frames N]
                               [--max-distance D] [--exclude N] [--window N] [--merge-overlap R]
                               [--prefilter [--bits B] [--max-hamming H] [--span S] [--dilate C] [--min-hits N] [--lsh-seed K]]

The definition this module computes (tests/terms_np.py restates it in numpy bit for bit; the LOCAL mode of
csrc/dtw_wave.h is the kernel):

* A pair is a stretch X of N frames (side 1, unbounded) and a stretch Y of M frames (side 2, at most ``max_n2()`` =
  ABN_DTW_LOCAL_MAX_N2 = 512 frames).  Cell (i, j) pairs X's frame i with Y's frame j.  A path is any run of steps
  diag / up / left from any cell to any cell: ANY stretch of X against ANY stretch of Y.
* Cells d(i, j) are the search's (qbe.py), unchanged, as float32.  ``distance='cosine'``: the angular distance of
  csrc/dist_ref.h; the zero-frame rule comes first (an all-zero frame is at distance 1 from any other frame, 0 from
  another zero frame); a NaN cell with a finite dot product and a finite non-zero float32 product of the norms is a
  rounding of |cos| above 1 and counts 0 (dot > 0) or 1 (dot < 0); any other NaN cell is BLOCKED (+inf).
  ``distance='kl'``: the symmetrised Kullback-Leibler divergence over the tables of ``abx.kl_tables``; a cell that
  touches a BAD row is blocked.  No pair is dropped as a whole.
* Exclusion: ``exclude`` >= 0 is an argument of the call.  When it is > 0 a cell with |(off1 + i) - (off2 + j)| <
  exclude is blocked -- off1 + i and off2 + j are TABLE rows, so both sides must be the same table (the C entry
  refuses other pointers, the wrapper raises ValueError).  It removes the trivial match of an utterance with itself.
  The kernel blocks these cells when it computes them; the similarity is taken from the blocked value.
* Similarity: s(i, j) = (double)theta - (double)d(i, j), ONE float64 subtraction of two float32 values, taken where the
  recurrence reads the cell; theta is a float32 argument, finite and > 0.  A blocked cell has s = -inf.
* Recurrence, in float64, Smith-Waterman over s.  The predecessors are diag = H(i-1, j-1), up = H(i-1, j),
  left = H(i, j-1); one outside the matrix is dead: H = 0, length 0.  `best` is the first maximum in the order diag,
  up, left: a later one replaces an earlier one only when strictly greater (the existing kernels' order).  If
  best > 0: H = best + s, length = best's length + 1 and the start cell (si, sj) is carried from it.  Otherwise H = s,
  length = 1, start = (i, j).  If not H > 0 the cell is dead: H = 0, length 0, start (-1, -1).
* Result per pair: the cell of largest H > 0, ties to the smallest i, then the smallest j: ``score`` = H (float64),
  ``path_len``, ``start1``, ``start2``, ``end1`` = i, ``end2`` = j, stretch-relative and inclusive.  The mean frame
  distance along the path is theta - score / path_len.  No live cell or an empty side: path_len = 0, score 0, the four
  bounds -1.  A pair outside its tables, a negative length or M beyond the cap: path_len = -1 and nothing is read.

``TermDiscoverer`` (every order below is fixed, so the written files are reproducible byte for byte):

* Utterances are numbered in sorted name order.  Utterance pairs: every (u, v) with u <= v, u == v included, by
  ascending (u, v); or the list given to ``discover(pairs=...)``, in its order.
* Kernel pairs: side 1 is u whole; side 2 is each window of v -- `window` frames (default and maximum max_n2()), hop
  window // 2, first frames 0, hop, 2 hop, ... below n - window, then the last window flush with the end at n - window;
  one window when v fits, none when it is empty (nor when u is).  Order: the utterance pairs', windows by first frame.
  The pairs of an utterance with ITSELF run with `exclude` (default min_frames), all others with 0 -- in launches of
  their own, because the last rows of one file and the first of the next are neighbours in the table.
* With a prefilter (abnet3_amd/prefilter.py: LSH signatures, the dot plot's longest diagonal run per kernel pair) only
  the kernel pairs it keeps are aligned, in the same order; without one (the default) all are, and nothing else runs.
* A match is kept when path_len > 0, both of its stretches have at least min_frames frames and, if max_distance is
  given, theta - score / path_len <= max_distance.  A repeat of the same (u, first1, last1, v, first2, last2) -- two
  windows that see one match -- is left out.  Matches stay in kernel-pair order.
* Fragments: match k gives fragment 2k = its side-1 stretch and 2k + 1 = its side-2 stretch, (file, first frame, last
  frame) with the match's score.  Union-find: the two fragments of a match are joined; two fragments of the same file
  are joined when their intersection is at least merge_overlap of the shorter one (and at least one frame).
* Within a cluster the fragments of a file are taken by descending score, then first frame, last frame, fragment
  number; one that shares a frame with a fragment already taken is dropped.  The tokens are sorted by (file number,
  first frame); clusters of fewer than two tokens are dropped; the clusters are sorted by their first token.
* ``write(out_dir)``: ``terms.classes`` (`Class k`, then `file onset offset` per token with the corpus' times of the
  first and last frame printed by repr(), then a blank line -- SamplerCluster.parse_input_file's format) and
  ``pairs_terms.txt`` + ``id_to_file.txt`` in discovery.write_pairs' format (`id1 id2 b1 e1 b2 e2 dist`, the ends
  EXCLUSIVE, dist = the mean frame distance printed %.11f) for PairsDataLoader.

`theta`'s default (0.25) is a placeholder: nothing here has been tuned or measured on real speech.  It is a distance --
a frame pair closer than theta adds to a path, one further away costs -- so it lives on the cell's scale: angular
distances lie in [0, 1], the KL cell is unbounded.
"""
import argparse
import os
import sys
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .abx import DISTANCES, _beyond_cap, _kl_triples, _pair_table, _read_h5features, kl_tables

Match = namedtuple('Match', ['file1', 'first1', 'last1', 'file2', 'first2', 'last2', 'score', 'path_len', 'distance'])


def max_n2():
    """The longest side 2, in frames, the kernel takes."""
    return int(_lib.load().abn_dtw_local_max_n2())


def _theta(who, theta):
    t = np.float32(theta)
    if not (np.isfinite(t) and t > 0):
        raise ValueError('%s: theta must be a positive finite float32, not %r' % (who, theta))
    return t


def local_dtw_batch(x, x_off, x_n, y, y_off, y_n, theta, exclude=0, distance='cosine'):
    """(score float64, path_len, start1, start2, end1, end2 int32) device tensors of pair p = any stretch of rows
    [x_off[p], x_off[p]+x_n[p]) of x against any stretch of rows [y_off[p], y_off[p]+y_n[p]) of y (module docstring).

    distance='cosine': x and y are [rows, D] float32 device tables (abn_dtw_local_batched).
    distance='kl': x and y are KLTables (or any (P, L, bad) triple) as abx.kl_tables returns them
    (abn_dtw_local_kl_batched).  A side 2 of more than max_n2() frames raises ValueError; so does exclude > 0 when x
    and y are not the same table."""
    if distance not in DISTANCES:
        raise ValueError('distance must be one of %s, not %r' % (DISTANCES, distance))
    theta = _theta('local_dtw_batch', theta)
    exclude = int(exclude)
    if exclude < 0:
        raise ValueError('local_dtw_batch: exclude must be >= 0')
    lib = _lib.load()
    kl = distance == 'kl'
    if kl:
        (x, Lx, badx), (y, Ly, bady) = x, y
        _kl_triples('local_dtw_batch', (x, Lx, badx), (y, Ly, bady))
        one_table = all(a.data_ptr() == b.data_ptr() for a, b in ((x, y), (Lx, Ly), (badx, bady)))
    else:
        _lib.require_device(x, y)
        if x.dim() != 2 or y.dim() != 2 or x.dtype != torch.float32 or y.dtype != torch.float32:
            raise ValueError('local_dtw_batch: [rows, D] float32 tables are needed')
        if x.shape[1] != y.shape[1]:
            raise ValueError('local_dtw_batch: the two sides have different frame widths')
        if not (x.is_contiguous() and y.is_contiguous()):
            raise ValueError('local_dtw_batch: the tables must be contiguous')
        one_table = x.data_ptr() == y.data_ptr()
    if exclude > 0 and not (one_table and x.shape[0] == y.shape[0]):
        raise ValueError('local_dtw_batch: exclude > 0 counts table rows, so both sides must be the same table')
    (x_off, x_n, y_off, y_n), d_tab = _pair_table('local_dtw_batch', x.shape[0], x_off, x_n, y.shape[0], y_off, y_n)
    P = len(x_n)
    _beyond_cap('local_dtw_batch: side 2 of pair %d has %d frames; at most %d are taken (%d pair(s) beyond it)',
                y_n, lib.abn_dtw_local_max_n2())
    dev = x.device
    score = torch.empty(P, dtype=torch.float64, device=dev)
    plen, s1, s2, e1, e2 = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(5))
    if P:
        table = [_lib.ptr(t) for t in d_tab] + [P, x.shape[1]]
        tail = [float(theta), exclude] + [_lib.ptr(t) for t in (score, plen, s1, s2, e1, e2)] + [_lib.stream()]
        if kl:
            _lib.check(lib.abn_dtw_local_kl_batched(_lib.ptr(x), _lib.ptr(Lx), x.shape[0], _lib.ptr(y), _lib.ptr(Ly), y.shape[0],
                                                    *(table + [_lib.ptr(badx), _lib.ptr(bady)] + tail)),
                       'abn_dtw_local_kl_batched')
        else:
            _lib.check(lib.abn_dtw_local_batched(_lib.ptr(x), x.shape[0], _lib.ptr(y), y.shape[0], *(table + tail)),
                       'abn_dtw_local_batched')
    return score, plen, s1, s2, e1, e2


# ---------------------------------------------------------------------------------------------------------------
# host side: windows, matches, clusters, files (plain Python / numpy; tests/test_terms_host.py runs it without a GPU)

def windows(n, window):
    """[(first frame, frames)] of the side-2 windows of an utterance of n frames (module docstring)."""
    if n <= 0:
        return []
    if n <= window:
        return [(0, n)]
    hop = max(1, window // 2)
    return [(s, window) for s in range(0, n - window, hop)] + [(n - window, window)]


def kernel_pairs(lengths, pairs, window):
    """[(u, v, first frame of the window in v, frames)] in the module's order."""
    return [(u, v, w0, wn) for u, v in pairs if lengths[u] > 0 for w0, wn in windows(lengths[v], window)]


def keep_matches(kp, result, theta, min_frames, max_distance=None):
    """The kept matches of the kernel pairs `kp` and their results (score, path_len, start1, start2, end1, end2 host
    arrays): Match tuples with file NUMBERS, in kernel-pair order, repeats of the same six bounds left out."""
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
            out.append(Match(*(key + (float(sc), int(ln), dist))))
    return out


def cluster_matches(matches, merge_overlap=0.5):
    """The clusters [[(file, first frame, last frame)]] of `matches` (module docstring): union-find over the matches'
    fragments, the collapse inside a cluster, singletons dropped, every list in its defined order."""
    frag = []
    for m in matches:
        frag.append((m.file1, m.first1, m.last1, m.score))
        frag.append((m.file2, m.first2, m.last2, m.score))
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
    by_file = {}
    for x, f in enumerate(frag):
        by_file.setdefault(f[0], []).append(x)
    for members in by_file.values():
        members.sort(key=lambda x: (frag[x][1], frag[x][2], x))
        for k, a in enumerate(members):
            for b in members[k + 1:]:
                if frag[b][1] > frag[a][2]:                         # sorted by first frame: nothing later overlaps a
                    break
                inter = min(frag[a][2], frag[b][2]) - frag[b][1] + 1
                if inter >= 1 and inter >= merge_overlap * min(frag[a][2] - frag[a][1] + 1, frag[b][2] - frag[b][1] + 1):
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


def _text(name):
    return name.decode('UTF-8') if isinstance(name, bytes) else str(name)


def write_classes(path, names, times, clusters):
    """The .classes file of clusters of (file number, first frame, last frame) tokens."""
    with open(path, 'w') as fh:
        for k, tokens in enumerate(clusters):
            fh.write('Class %d\n' % k)
            for f, lo, hi in tokens:
                t = times[names[f]]
                fh.write('%s %r %r\n' % (_text(names[f]), float(t[lo]), float(t[hi])))
            fh.write('\n')
    return path


def write_term_pairs(out_dir, names, matches):
    """pairs_terms.txt and id_to_file.txt of matches with file numbers; returns their paths."""
    pairs_path, map_path = os.path.join(out_dir, 'pairs_terms.txt'), os.path.join(out_dir, 'id_to_file.txt')
    with open(pairs_path, 'w') as fh:
        for m in matches:
            fh.write('%d %d %d %d %d %d %.11f\n' % (m.file1, m.file2, m.first1, m.last1 + 1, m.first2, m.last2 + 1, m.distance))
    with open(map_path, 'w') as fh:
        for f, name in enumerate(names):
            fh.write('%d %s\n' % (f, _text(name)))
    return pairs_path, map_path


class TermDiscoverer(object):
    """Discovers repeated stretches ("terms") in `corpus` and clusters them (module docstring).

    corpus: a DeviceCorpus, a {name: [T, D]} features dict together with `times`, or the path of an h5features file.
    distance: 'cosine' (features, embeddings) or 'kl' (posteriorgrams; kl_tables(corpus.table, floor) is built once).
    theta: the distance below which a frame pair adds to a path (untuned default, module docstring).  min_frames: the
    shortest stretch kept.  max_distance: the largest mean frame distance kept (None: no limit).  exclude: the
    half-width of the band around the diagonal blocked when an utterance meets itself (None: min_frames).  window:
    side-2 window in frames (None: max_n2(), the maximum).  chunk_pairs: how many kernel pairs one launch takes.
    prefilter: a prefilter.TermPrefilter that picks the kernel pairs worth aligning (None: all are aligned).

    After discover(): names (sorted), matches (Match tuples, files as numbers), clusters (lists of (file number, first
    frame, last frame))."""

    def __init__(self, corpus, times=None, distance='cosine', floor=1e-6, theta=0.25, min_frames=50, max_distance=None,
                 exclude=None, window=None, merge_overlap=0.5, chunk_pairs=1 << 18, prefilter=None):
        if distance not in DISTANCES:
            raise ValueError('distance must be one of %s, not %r' % (DISTANCES, distance))
        if chunk_pairs < 1:
            raise ValueError('chunk_pairs must be positive')
        if min_frames < 1:
            raise ValueError('min_frames must be positive')
        if not 0 < merge_overlap:
            raise ValueError('merge_overlap must be positive')
        self.theta = _theta('TermDiscoverer', theta)
        self.exclude = int(min_frames if exclude is None else exclude)
        if self.exclude < 0:
            raise ValueError('exclude must be >= 0')
        from .dataloader import DeviceCorpus
        if isinstance(corpus, str):
            corpus, times = _read_h5features(corpus)
        if not isinstance(corpus, DeviceCorpus):
            if times is None:
                raise ValueError('TermDiscoverer: a features dict needs its times dict')
            corpus = DeviceCorpus(corpus, times)
        cap = max_n2()
        self.window = cap if window is None else int(window)
        if not 1 <= self.window <= cap:
            raise ValueError('TermDiscoverer: window must lie in 1 .. %d frames' % cap)
        self.corpus, self.distance, self.floor = corpus, distance, floor
        self.min_frames, self.max_distance, self.merge_overlap = int(min_frames), max_distance, merge_overlap
        self.chunk_pairs = int(chunk_pairs)
        self.prefilter = prefilter
        self.names = sorted(corpus.names, key=_text)
        self.tables = kl_tables(corpus.table, floor) if distance == 'kl' else None

    def align(self, kp):
        """The kernel's results for kernel pairs `kp`: host arrays (score, path_len, start1, start2, end1, end2)."""
        c = self.corpus
        base = np.array([c.offset[k] for k in self.names], dtype=np.int64)
        length = np.array([c.length[k] for k in self.names], dtype=np.int32)
        kp = np.asarray(kp, dtype=np.int64).reshape(-1, 4)
        u, v, w0, wn = kp[:, 0], kp[:, 1], kp[:, 2], kp[:, 3]
        out = [np.zeros(len(kp), dtype=np.float64)] + [np.zeros(len(kp), dtype=np.int32) for _ in range(5)]
        t = self.tables if self.distance == 'kl' else c.table
        for idx, exclude in ((np.flatnonzero(u == v), self.exclude), (np.flatnonzero(u != v), 0)):
            for lo in range(0, len(idx), self.chunk_pairs):
                k = idx[lo:lo + self.chunk_pairs]
                res = local_dtw_batch(t, base[u[k]], length[u[k]], t, base[v[k]] + w0[k], wn[k], self.theta, exclude=exclude,
                                      distance=self.distance)
                for dst, r in zip(out, res):
                    dst[k] = r.cpu().numpy()
        if (out[1] < 0).any():
            raise RuntimeError('the local-alignment kernel refused %d pairs of a table this module built' % int((out[1] < 0).sum()))
        return tuple(out)

    def discover(self, pairs=None, prefilter=None):
        """(matches, clusters).  pairs: [(name u, name v)] utterance pairs (u is side 1, whole; v is windowed); default:
        every unordered pair, an utterance with itself included.  prefilter (default: the constructor's): a
        prefilter.TermPrefilter -- only the kernel pairs its keep() passes are aligned, in their order; None: all of them,
        without any further launch.  Afterwards n_kernel_pairs, n_aligned_pairs and, with a prefilter, prefilter_best
        (the int32 array of the best runs over ALL kernel pairs; None without one)."""
        n = len(self.names)
        if pairs is None:
            upairs = [(u, v) for u in range(n) for v in range(u, n)]
        else:
            number = {k: f for f, k in enumerate(self.names)}
            upairs = [(number[self.corpus._name(a)], number[self.corpus._name(b)]) for a, b in pairs]
        lengths = [self.corpus.length[k] for k in self.names]
        kp = kernel_pairs(lengths, upairs, self.window)
        prefilter = self.prefilter if prefilter is None else prefilter
        self.n_kernel_pairs, self.prefilter_best = len(kp), None
        if prefilter is not None:
            mask = np.asarray(prefilter.keep(self, kp), dtype=bool)
            if mask.shape != (len(kp),):
                raise ValueError('TermDiscoverer: the prefilter\'s mask does not cover the kernel pairs')
            self.prefilter_best = getattr(prefilter, 'best', None)
            kp = [q for q, m in zip(kp, mask) if m]
        self.n_aligned_pairs = len(kp)
        self.matches = keep_matches(kp, self.align(kp), self.theta, self.min_frames, self.max_distance)
        self.clusters = cluster_matches(self.matches, self.merge_overlap)
        return self.matches, self.clusters

    def term_scores(self, evaluator, words=None, speakers=None):
        """tde.FullTermScores of the discovered clusters under a tde.TermEvaluator (discover() must have run)."""
        return evaluator.evaluate_full(self.clusters, self.names, self.corpus.times, words=words, speakers=speakers)

    def write(self, out_dir):
        """Discovers (if discover() has not run) and writes OUT_DIR/terms.classes, OUT_DIR/pairs_terms.txt and
        OUT_DIR/id_to_file.txt; returns their paths."""
        if not hasattr(self, 'clusters'):
            self.discover()
        os.makedirs(out_dir, exist_ok=True)
        classes = write_classes(os.path.join(out_dir, 'terms.classes'), self.names, self.corpus.times, self.clusters)
        return (classes,) + write_term_pairs(out_dir, self.names, self.matches)


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m abnet3_amd.terms',
                                 description='Spoken-term discovery: local-alignment DTW of every utterance pair, clustered')
    ap.add_argument('features', help='h5features file (features, embeddings or posteriorgrams; needs the h5features package)')
    ap.add_argument('out_dir')
    ap.add_argument('--distance', choices=DISTANCES, default='cosine',
                    help="frame distance: 'cosine' or 'kl' (posteriorgrams, symmetrised Kullback-Leibler)")
    ap.add_argument('--floor', type=float, default=1e-6, help='floor of the probabilities under --distance kl')
    ap.add_argument('--theta', type=float, default=0.25, help='distance below which a frame pair adds to a path (untuned)')
    ap.add_argument('--min-frames', type=int, default=50)
    ap.add_argument('--max-distance', type=float, default=None)
    ap.add_argument('--exclude', type=int, default=None, help='band blocked around the diagonal of a self-pair (default: --min-frames)')
    ap.add_argument('--window', type=int, default=None)
    ap.add_argument('--merge-overlap', type=float, default=0.5)
    ap.add_argument('--prefilter', action='store_true',
                    help='align only the kernel pairs whose dot plot of LSH signatures holds a diagonal run (abnet3_amd.prefilter; untuned)')
    ap.add_argument('--bits', type=int, default=64, help='signature bits, a multiple of 32 in 32 .. 256')
    ap.add_argument('--max-hamming', type=int, default=None, help='most differing bits of a hit (default: bits // 4)')
    ap.add_argument('--span', type=int, default=32, help='frames of the window along a diagonal, 1 .. 64')
    ap.add_argument('--dilate', type=int, default=1, help='columns a hit is spread to either side, 0 .. 8')
    ap.add_argument('--min-hits', type=int, default=None, help='hits a kept pair\'s best window holds (default: 3 * span // 4)')
    ap.add_argument('--lsh-seed', type=int, default=0)
    args = ap.parse_args(argv)
    pre = None
    if args.prefilter:
        from .prefilter import TermPrefilter
        pre = TermPrefilter(bits=args.bits, seed=args.lsh_seed, max_hamming=args.max_hamming, span=args.span, dilate=args.dilate,
                            min_hits=args.min_hits)
    td = TermDiscoverer(args.features, distance=args.distance, floor=args.floor, theta=args.theta, min_frames=args.min_frames,
                        max_distance=args.max_distance, exclude=args.exclude, window=args.window,
                        merge_overlap=args.merge_overlap, prefilter=pre)
    paths = td.write(args.out_dir)
    print('%d utterances, %d matches, %d clusters (%d tokens), %d of %d kernel pairs aligned -> %s' % (
        len(td.names), len(td.matches), len(td.clusters), sum(len(c) for c in td.clusters), td.n_aligned_pairs,
        td.n_kernel_pairs, ', '.join(paths)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
