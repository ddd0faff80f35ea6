"""The prefilter of spoken-term discovery on the MI355X: random-hyperplane signatures of every frame, the sparse "dot
plot" of near-equal signatures of every kernel pair, and the longest diagonal run in it.  TermDiscoverer spends its
local-alignment DTW only on the kernel pairs whose run is long enough (``TermDiscoverer(..., prefilter=TermPrefilter())``
or ``discover(prefilter=...)``); without a prefilter nothing changes.

The definition (tests/prefilter_np.py restates it in numpy; csrc/lsh.hip holds the two kernels):

* ``lsh_planes(D, bits, seed)``: float32 [bits, D] = ``np.random.default_rng(seed).standard_normal((bits, D))`` cast to
  float32 -- the signatures are reproducible from (seed, bits, D) alone.  bits: a multiple of 32 in 32 .. 256.
* ``lsh_signatures(table, planes)`` (abn_lsh_signatures): bit b of row r -- bit b % 32 of word b // 32, least significant
  first -- is 1 iff the float32 dot product <table[r], planes[b]> is > 0.  live[r] = 1 iff every element of the row is
  finite and at least one is non-zero; a dead row's words are 0.  The angular distance arccos(cos) / pi of the DTW cells
  here is the probability that a random hyperplane separates two frames: Hamming distance / bits estimates the cell.
* ``diag_hits_batch`` (abn_lsh_diag_hits_batched), for pair p, 0 <= i < n1, 0 <= j < n2:
  hit(i, j) = both rows live and popcount(sig1[off1+i] ^ sig2[off2+j]) <= max_hamming and (exclude == 0 or
  |(off1+i) - (off2+j)| >= exclude); hd(i, j) = OR of hit(i, j+t) over |t| <= dilate inside the matrix (a path may drift
  off its diagonal); run(i, j) = the sum of hd(i-s, j-s) over s = 0 .. span-1 inside the matrix.  best = the largest run,
  diag = i - j and end1 = i of its cell, ties to the smallest i - j, then the smallest i; no hit or an empty side:
  (0, 0, -1); a refused pair (outside its tables, a negative length, side 2 beyond terms.max_n2()): (-1, 0, -1).
* ``TermPrefilter.keep(discoverer, kp)``: best >= min_hits per kernel pair, over the discoverer's own tables, order,
  windows and exclusion -- the pairs of an utterance with itself in launches of their own, as TermDiscoverer.align runs
  them.  For distance='kl' the signatures are taken over sqrt(P) of the discoverer's kl_tables (the angle between the
  square roots of two distributions is the Bhattacharyya angle); BAD rows are dead.

What ZRTools does and this does not: no median filter over the dot plot, no Hough peak list -- ONE best run per kernel
pair --, and the DTW still runs over the whole kernel pair, not over a band around the diagonal found.

``max_hamming`` (default bits // 4) and ``min_hits`` (default 3 * span // 4) are placeholders: nothing here has been
tuned or measured on real speech.
"""
import numpy as np
import torch

from . import _lib

MAX_BITS, MAX_D, MAX_SPAN, MAX_DILATE = 256, 4096, 64, 8      # include/abnet3_hip.h: ABN_LSH_*
GRID_BLOCKS = 2048                                            # ABN_LSH_GRID_BLOCKS: the pairs one pass of the grid holds


def _bits(who, bits):
    bits = int(bits)
    if not (32 <= bits <= MAX_BITS and bits % 32 == 0):
        raise ValueError('%s: bits must be a multiple of 32 in 32 .. %d, not %d' % (who, MAX_BITS, bits))
    return bits


def lsh_planes(D, bits=64, seed=0):
    """float32 [bits, D] hyperplane normals (module docstring)."""
    bits, D = _bits('lsh_planes', bits), int(D)
    if not 1 <= D <= MAX_D:
        raise ValueError('lsh_planes: D must lie in 1 .. %d, not %d' % (MAX_D, D))
    return np.random.default_rng(seed).standard_normal((bits, D)).astype(np.float32)


def lsh_signatures(table, planes):
    """(sig uint32-as-int32 [rows, bits // 32], live uint8 [rows]) device tensors of the [rows, D] float32 device table
    under planes [bits, D] (a host array, which is uploaded, or a device tensor).  torch has no uint32 arithmetic: the
    words are held in an int32 tensor, bit for bit."""
    if not isinstance(planes, torch.Tensor):
        planes = torch.from_numpy(np.ascontiguousarray(planes, dtype=np.float32)).to(table.device)
    _lib.require_device(table, planes)
    if table.dim() != 2 or planes.dim() != 2 or table.dtype != torch.float32 or planes.dtype != torch.float32:
        raise ValueError('lsh_signatures: a [rows, D] float32 table and [bits, D] float32 planes are needed')
    if table.shape[1] != planes.shape[1]:
        raise ValueError('lsh_signatures: the table and the planes have different frame widths')
    rows, D = table.shape
    bits = _bits('lsh_signatures', planes.shape[0])
    if not 1 <= D <= MAX_D:
        raise ValueError('lsh_signatures: D must lie in 1 .. %d, not %d' % (MAX_D, D))
    sig = torch.empty((rows, bits // 32), dtype=torch.int32, device=table.device)
    live = torch.empty(rows, dtype=torch.uint8, device=table.device)
    if rows:
        _lib.check(_lib.load().abn_lsh_signatures(_lib.ptr(table), rows, D, _lib.ptr(planes), bits, _lib.ptr(sig), _lib.ptr(live),
                                                  _lib.stream()), 'abn_lsh_signatures')
    return sig, live


def _column(who, a, dt, device):
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype={torch.int32: np.int32, torch.int64: np.int64}[dt])).to(device)
    if a.dtype != dt or a.dim() != 1:
        raise ValueError('%s: a 1-d %s column is needed, not %s %s' % (who, dt, a.dtype, tuple(a.shape)))
    a = a.contiguous()
    _lib.require_device(a)
    return a


def diag_hits_batch(sig1, live1, off1, n1, sig2, live2, off2, n2, max_hamming, span=32, dilate=0, exclude=0):
    """(best, diag, end1) int32 device tensors per pair (module docstring).  sig* / live* as lsh_signatures returns them;
    off* int64 and n* int32 columns, device tensors or host arrays, which are uploaded.  Host-detectable misuse raises
    ValueError: signatures of different widths, parameters out of range, exclude > 0 when the two sides are not the
    same tables.  A pair outside its tables, with a negative length or a side 2 beyond terms.max_n2() comes back as
    best = -1: nothing is raised for it."""
    who = 'diag_hits_batch'
    _lib.require_device(sig1, live1, sig2, live2)
    for s, l in ((sig1, live1), (sig2, live2)):
        if s.dim() != 2 or s.dtype != torch.int32 or l.dtype != torch.uint8 or l.shape != s.shape[:1]:
            raise ValueError('%s: (sig int32 [rows, words], live uint8 [rows]) as lsh_signatures returns them are needed' % who)
    words = sig1.shape[1]
    if sig2.shape[1] != words or not 1 <= words <= MAX_BITS // 32:
        raise ValueError('%s: both sides need signatures of the same width, 1 .. %d words' % (who, MAX_BITS // 32))
    max_hamming, span, dilate, exclude = int(max_hamming), int(span), int(dilate), int(exclude)
    if not 0 <= max_hamming <= 32 * words:
        raise ValueError('%s: max_hamming must lie in 0 .. %d (the bits), not %d' % (who, 32 * words, max_hamming))
    if not 1 <= span <= MAX_SPAN:
        raise ValueError('%s: span must lie in 1 .. %d, not %d' % (who, MAX_SPAN, span))
    if not 0 <= dilate <= MAX_DILATE:
        raise ValueError('%s: dilate must lie in 0 .. %d, not %d' % (who, MAX_DILATE, dilate))
    if exclude < 0:
        raise ValueError('%s: exclude must be >= 0' % who)
    one_table = sig1.data_ptr() == sig2.data_ptr() and live1.data_ptr() == live2.data_ptr() and sig1.shape[0] == sig2.shape[0]
    if exclude > 0 and not one_table:
        raise ValueError('%s: exclude > 0 counts table rows, so both sides must be the same table' % who)
    dev = sig1.device
    off1, n1, off2, n2 = (_column(who, off1, torch.int64, dev), _column(who, n1, torch.int32, dev),
                          _column(who, off2, torch.int64, dev), _column(who, n2, torch.int32, dev))
    P = n1.numel()
    if not (off1.numel() == off2.numel() == n2.numel() == P):
        raise ValueError('%s: the pair table\'s columns differ in length' % who)
    best, diag, end1 = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))
    if P:
        _lib.check(_lib.load().abn_lsh_diag_hits_batched(
            _lib.ptr(sig1), _lib.ptr(live1), sig1.shape[0], _lib.ptr(sig2), _lib.ptr(live2), sig2.shape[0], _lib.ptr(off1),
            _lib.ptr(n1), _lib.ptr(off2), _lib.ptr(n2), P, words, max_hamming, span, dilate, exclude, _lib.ptr(best),
            _lib.ptr(diag), _lib.ptr(end1), _lib.stream()), 'abn_lsh_diag_hits_batched')
    return best, diag, end1


def self_and_cross(u, v):
    """The two launches of a kernel-pair list: (indices, uses the exclusion) for the pairs of an utterance with itself,
    then for all others -- TermDiscoverer.align's split."""
    return ((np.flatnonzero(u == v), True), (np.flatnonzero(u != v), False))


class TermPrefilter(object):
    """Keeps the kernel pairs of a TermDiscoverer whose dot plot holds a diagonal run (module docstring).

    bits, seed: the signatures (lsh_planes).  max_hamming: two frames hit when their signatures differ in at most this
    many bits (None: bits // 4).  span: the length of the sliding window along a diagonal, 1 .. 64.  dilate: how many
    columns a hit is spread to either side, 0 .. 8.  min_hits: a kernel pair is kept when its best window holds at
    least this many hits (None: 3 * span // 4).  max_hamming and min_hits are untuned placeholders, as
    TermDiscoverer's theta is: nothing here has been measured on real speech.

    After keep(): best (the int32 host array over the kernel pairs it was given)."""

    def __init__(self, bits=64, seed=0, max_hamming=None, span=32, dilate=1, min_hits=None):
        self.bits, self.seed = _bits('TermPrefilter', bits), seed
        self.span, self.dilate = int(span), int(dilate)
        if not 1 <= self.span <= MAX_SPAN:
            raise ValueError('TermPrefilter: span must lie in 1 .. %d, not %d' % (MAX_SPAN, self.span))
        if not 0 <= self.dilate <= MAX_DILATE:
            raise ValueError('TermPrefilter: dilate must lie in 0 .. %d, not %d' % (MAX_DILATE, self.dilate))
        self.max_hamming = self.bits // 4 if max_hamming is None else int(max_hamming)
        if not 0 <= self.max_hamming <= self.bits:
            raise ValueError('TermPrefilter: max_hamming must lie in 0 .. %d (bits), not %d' % (self.bits, self.max_hamming))
        self.min_hits = 3 * self.span // 4 if min_hits is None else int(min_hits)
        if self.min_hits < 0:
            raise ValueError('TermPrefilter: min_hits must be >= 0')
        self._built = None          # (discoverer, sig, live): the signatures are built once per discoverer

    def signatures(self, discoverer):
        """(sig, live) over the discoverer's table, built at the first call for it."""
        if self._built is None or self._built[0] is not discoverer:
            if discoverer.distance == 'kl':
                t = discoverer.tables
                sig, live = lsh_signatures(torch.sqrt(t.P), lsh_planes(t.P.shape[1], self.bits, self.seed))
                ok = t.bad == 0
                sig, live = sig * ok[:, None].to(torch.int32), live * ok.to(torch.uint8)
            else:
                table = discoverer.corpus.table
                sig, live = lsh_signatures(table, lsh_planes(table.shape[1], self.bits, self.seed))
            self._built = (discoverer, sig.contiguous(), live.contiguous())
        return self._built[1:]

    def best_runs(self, discoverer, kp):
        """The int32 host array of best[p] over the kernel pairs kp [(u, v, first frame of the window, frames)]."""
        c = discoverer.corpus
        sig, live = self.signatures(discoverer)
        base = np.array([c.offset[k] for k in discoverer.names], dtype=np.int64)
        length = np.array([c.length[k] for k in discoverer.names], dtype=np.int32)
        kp = np.asarray(kp, dtype=np.int64).reshape(-1, 4)
        u, v, w0, wn = kp[:, 0], kp[:, 1], kp[:, 2], kp[:, 3]
        best = np.zeros(len(kp), dtype=np.int32)
        for idx, own in self_and_cross(u, v):
            for lo in range(0, len(idx), discoverer.chunk_pairs):
                k = idx[lo:lo + discoverer.chunk_pairs]
                b, _d, _e = diag_hits_batch(sig, live, base[u[k]], length[u[k]], sig, live, base[v[k]] + w0[k], wn[k].astype(np.int32),
                                            self.max_hamming, self.span, self.dilate, discoverer.exclude if own else 0)
                best[k] = b.cpu().numpy()
        if (best < 0).any():
            raise RuntimeError('the prefilter kernel refused %d pairs of a table this module built' % int((best < 0).sum()))
        return best

    def keep(self, discoverer, kp):
        """The boolean mask best >= min_hits over the kernel pairs kp, in their order."""
        self.best = self.best_runs(discoverer, kp)
        return self.best >= self.min_hits
