"""Embedded segmental k-means on the MI355X (Kamper, Livescu & Goldwater 2017, "ES-KMeans"): full-coverage word
segmentation.  Every utterance is cut into word-like segments at landmarks, and all segments are clustered.

    python -m abnet3_amd.eskmeans fit FEATURES MODEL.npz [-k K] [--step N | --units UNITS.npz] [--max-span S] ...
    python -m abnet3_amd.eskmeans segment MODEL.npz FEATURES OUT.classes [--step N | --units UNITS.npz]

The definition this module computes (tests/esk_np.py restates it with explicit loops):

* Landmarks: {name: increasing int64 frame indices}, the first 0 (or the utterance's first used frame) and the last one
  past its last frame; at least two per utterance.  ``uniform_landmarks`` puts one every `step` frames,
  ``landmarks_from_units`` at the unit boundaries ``kmeans.segments`` returns.  On the device they are lm [n_lm] int64
  rows of the corpus table and lm_off [n_utt + 1] int64; utterance u owns lm[lm_off[u] .. lm_off[u + 1]).
* Candidates: (g, s), 1 <= s <= S = max_span <= abn_esk_max_span() (8), runs from landmark g to g + s inside one
  utterance, covers rows lm[g] .. lm[g + s] - 1 (n of them) and lives at index g S + s - 1.  It is allowed if s == 1 or
  n <= max_frames (None: no limit), so a path always exists.
* Segment vector: ``discovery.segment_vectors``' -- the `frames` rows lm[g] + ((2 j + 1) n) // (2 frames), concatenated
  to frames D floats and scaled to unit length (sum of squares in float64, scale in fp32).
* Score: s[c, k] = <v_c, m_k> + b_k with ``kmeans.score_tables`` of the centroids (m fp32, b = -|m|^2 / 2) and a zero
  shift: the assign pass's fp32 GEMM of depth frames D + 1.  cand_best = max_k, cand_id = the lowest k attaining it.
  A candidate that crosses an utterance, is not allowed, is all zero or has a non-finite sampled value: id -1, best NaN.
  ``candidate_scores`` (abn_esk_score, one launch) gives the bits of segment_vectors + kmeans.assign over the table of
  all candidates without forming it: 8 bytes per candidate instead of 4 (frames D) bytes.
* Cost: c = fp32(n) * (1 - 2 best), each operation rounded once in fp32; +inf where id = -1.  For a unit v this is
  n |v - mu|^2, Kamper's duration-weighted distance.
* Segmentation (``segment_dp``, abn_esk_segment, one launch): per utterance with L = landmarks - 1, in fp32,
  gamma[0] = 0, gamma[j] = min_s gamma[j - s] + c(j - s, s), equal sums to the smallest s; the traceback from L marks
  `cut` at every chosen boundary, `word` / `span` at every chosen start (-1 elsewhere); objective = gamma[L].  An
  utterance whose end cannot be reached: objective NaN, n_seg -1, nothing marked.
* Fit: the initial segmentation walks each utterance (corpus order) and draws every span uniformly among the allowed
  ones with numpy.random.default_rng(seed).  Initial centroids: the vectors of K distinct initial segments (sorted
  ``choice(n, K, replace=False)`` of the same generator, all-zero and non-finite segments left out), or ``init``
  [K, frames D].  Iteration i: score, DP, then the vectors of the CHOSEN segments only (a small table), and the existing
  ``kmeans.accumulate`` / update with the chosen ids: each centroid becomes the UNWEIGHTED mean of its segments' unit
  vectors (Kamper's), an empty cluster keeps its centroid.  It stops when no `cut` changed since the previous
  iteration, or after n_iter iterations.  ``objective_[i]`` is the sum of the utterances' objectives of iteration i
  (unreachable ones left out and counted in ``n_unreachable_``), ``n_segments_[i]`` the number of chosen segments.
* The objective is NOT guaranteed to fall: the DP minimises sum n |v - mu|^2 through the identity 1 - 2 score, which
  holds for unit v, while the update takes the unweighted mean -- the minimiser of sum |v - mu|^2, not of the
  duration-weighted sum.  Kamper's code does the same.
* Deviations from Kamper's code: no minimum duration, no Gibbs / BES-GMM variant, K <= 4096 and
  frames D <= 512.  n_clusters, max_span and the landmark density are untuned; nothing was measured on real speech.
"""
import argparse
import sys

import numpy as np
import torch

from . import _lib, kmeans
from .discovery import segment_vectors


def max_span():
    return int(_lib.load().abn_esk_max_span())


def _lengths(corpus):
    from .dataloader import DeviceCorpus
    if isinstance(corpus, DeviceCorpus):
        return {k: int(corpus.length[k]) for k in corpus.names}
    return {k: int(v) if np.ndim(v) == 0 else int(np.asarray(v).shape[0]) for k, v in corpus.items()}


def uniform_landmarks(corpus, step):
    """{name: int64 landmarks}: 0, step, 2 step, ... and the utterance's length.  corpus: a DeviceCorpus, a
    {name: [T, D]} dict or a {name: length} dict; an empty utterance is left out."""
    step = int(step)
    if step < 1:
        raise ValueError('uniform_landmarks: step = %r' % (step,))
    return {k: np.append(np.arange(0, n, step, dtype=np.int64), np.int64(n)) for k, n in _lengths(corpus).items() if n > 0}


def landmarks_from_units(segments, lengths=None):
    """{name: int64 landmarks} from what ``kmeans.segments`` returns ({name: (start, end, unit)}): every start and end of
    a run, sorted; with `lengths` ({name: frames}) 0 and the length as well, so that runs of BAD frames are covered.
    A file without any run (and without a length) is left out."""
    out = {}
    for k, (start, end, _) in segments.items():
        marks = [np.asarray(start, dtype=np.int64).ravel(), np.asarray(end, dtype=np.int64).ravel()]
        if lengths is not None and int(lengths[k]) > 0:
            marks.append(np.array([0, int(lengths[k])], dtype=np.int64))
        lm = np.unique(np.concatenate(marks))
        if len(lm) >= 2:
            out[k] = lm
    return out


def pack_landmarks(landmarks, offsets, lengths, names=None):
    """(names, lm int64 [n_lm] table rows, lm_off int64 [n_utt + 1]) of {name: landmarks}: the utterances in `names`
    order (default: the order of `offsets`), those without landmarks left out.  Checked here, on the host: at least two
    per utterance, strictly increasing, inside 0 .. length."""
    order = [k for k in (names if names is not None else offsets) if k in landmarks]
    if not order:
        raise ValueError('eskmeans: no utterance has landmarks')
    lm, off = [], [0]
    for k in order:
        a = np.asarray(landmarks[k], dtype=np.int64).ravel()
        if len(a) < 2 or (np.diff(a) < 1).any() or a[0] < 0 or a[-1] > int(lengths[k]):
            raise ValueError('eskmeans: the landmarks of %r must be at least two strictly increasing frames in 0 .. %d'
                             % (k, int(lengths[k])))
        lm.append(a + int(offsets[k]))
        off.append(off[-1] + len(a))
    return order, np.concatenate(lm), np.asarray(off, dtype=np.int64)


def _dev_i64(a, device):
    if isinstance(a, torch.Tensor):
        _lib.require_device(a)
        if a.dtype != torch.int64:
            raise ValueError('eskmeans: landmark arrays are int64')
        return a
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device)


def _packed_landmarks(who, lm, lm_off, device):
    """(lm, lm_off) int64 on the device.  Host arrays are held to what the kernels assume, which pack_landmarks builds:
    1-d, lm_off running from 0 to len(lm) without a step back (device tensors are the caller's to have packed)."""
    if not isinstance(lm, torch.Tensor) and not isinstance(lm_off, torch.Tensor):
        a, o = np.asarray(lm), np.asarray(lm_off)
        if a.ndim != 1 or o.ndim != 1 or len(o) < 1 or o[0] != 0 or o[-1] != len(a) or (np.diff(o) < 0).any():
            raise ValueError('%s: lm_off must run from 0 to the %d landmarks of lm (pack_landmarks)' % (who, a.size))
    return _dev_i64(lm, device), _dev_i64(lm_off, device)


def _check_span(who, S):
    S = int(S)
    if S < 1 or S > max_span():
        raise ValueError('%s: max_span = %d, the kernels take 1 .. %d (abn_esk_max_span)' % (who, S, max_span()))
    return S


def candidate_scores(table, lm, lm_off, m, b, frames=10, max_span=6, max_frames=None):
    """(cand_best [n_lm S] float32, cand_id [n_lm S] int32) on the device (abn_esk_score, one launch; module docstring).
    table [T, D] float32 and m [K, frames D], b [K] float32 on the device; lm, lm_off: host arrays or int64 device tensors."""
    lib = _lib.load()
    S = _check_span('eskmeans.candidate_scores', max_span)
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.dtype != torch.float32 or table.shape[0] < 1:
        raise ValueError('eskmeans.candidate_scores: a [T, D] float32 table is needed')
    _lib.require_device(table, m, b)
    T, D = table.shape
    frames = int(frames)
    K = b.shape[0]
    if frames < 1 or frames * D > kmeans.max_d():
        raise ValueError('eskmeans.candidate_scores: frames x D = %d x %d, the kernel takes up to %d (abn_kmeans_max_d)'
                         % (frames, D, kmeans.max_d()))
    if K < 1 or K > kmeans.max_k():
        raise ValueError('eskmeans.candidate_scores: K = %d, the kernel takes 1 .. %d (abn_kmeans_max_k)' % (K, kmeans.max_k()))
    if m.shape != (K, frames * D) or m.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError('eskmeans.candidate_scores: m [K, frames D] and b [K] float32 are needed')
    lm, lm_off = _packed_landmarks('eskmeans.candidate_scores', lm, lm_off, table.device)
    n_lm, n_utt = lm.numel(), lm_off.numel() - 1
    max_frames = (1 << 62) if max_frames is None else int(max_frames)
    if max_frames < 1:
        raise ValueError('eskmeans.candidate_scores: max_frames = %d' % max_frames)
    best = torch.empty(n_lm * S, dtype=torch.float32, device=table.device)
    ids = torch.empty(n_lm * S, dtype=torch.int32, device=table.device)
    _lib.check(lib.abn_esk_score(_lib.ptr(table), T, D, _lib.ptr(lm), _lib.ptr(lm_off), n_utt, n_lm, frames, S, max_frames,
                                 _lib.ptr(m), _lib.ptr(b), K, _lib.ptr(best), _lib.ptr(ids), _lib.stream()), 'abn_esk_score')
    return best, ids


def segment_dp(cand_best, cand_id, lm, lm_off, max_span=6):
    """(cut [n_lm] uint8, word [n_lm] int32, span [n_lm] int32, objective [n_utt] float64, n_seg [n_utt] int32) on the
    device (abn_esk_segment, one launch; module docstring).  lm_off must tile 0 .. n_lm with utterances of at least two
    landmarks (pack_landmarks checks it): the kernel leaves the rows of anything else unwritten."""
    lib = _lib.load()
    S = _check_span('eskmeans.segment_dp', max_span)
    _lib.require_device(cand_best, cand_id)
    lm, lm_off = _packed_landmarks('eskmeans.segment_dp', lm, lm_off, cand_best.device)
    n_lm, n_utt = lm.numel(), lm_off.numel() - 1
    if cand_best.dtype != torch.float32 or cand_id.dtype != torch.int32 or cand_best.numel() != n_lm * S or cand_id.numel() != n_lm * S:
        raise ValueError('eskmeans.segment_dp: cand_best float32 and cand_id int32 of n_lm x S = %d entries are needed' % (n_lm * S))
    dev = cand_best.device
    cut = torch.empty(n_lm, dtype=torch.uint8, device=dev)         # (the kernel writes every row of every utterance)
    word = torch.empty(n_lm, dtype=torch.int32, device=dev)
    span = torch.empty(n_lm, dtype=torch.int32, device=dev)
    obj = torch.empty(n_utt, dtype=torch.float64, device=dev)
    nseg = torch.empty(n_utt, dtype=torch.int32, device=dev)
    _lib.check(lib.abn_esk_segment(_lib.ptr(cand_best), _lib.ptr(cand_id), _lib.ptr(lm), _lib.ptr(lm_off), n_utt, n_lm, S,
                                   _lib.ptr(cut), _lib.ptr(word), _lib.ptr(span), _lib.ptr(obj), _lib.ptr(nseg), _lib.stream()),
               'abn_esk_segment')
    return cut, word, span, obj, nseg


def initial_spans(lm, lm_off, S, max_frames, rng):
    """span int32 [n_lm] of the seeded random initial segmentation (module docstring): the drawn span at every chosen
    start, -1 elsewhere."""
    span = np.full(len(lm), -1, dtype=np.int32)
    for u in range(len(lm_off) - 1):
        lo, hi = int(lm_off[u]), int(lm_off[u + 1])
        g = lo
        while g < hi - 1:
            ok = [s for s in range(1, min(S, hi - 1 - g) + 1) if s == 1 or max_frames is None or lm[g + s] - lm[g] <= max_frames]
            span[g] = ok[int(rng.integers(len(ok)))]
            g += int(span[g])
    return span


class ESKMeans(object):
    """fit / segment of the segmentation the module docstring defines.

    corpus arguments: a DeviceCorpus, or a {name: [T, D] float32} dict together with `times` ({name: [T] seconds};
    default: 10 ms frames from 0).  landmarks: {name: frame indices} (uniform_landmarks, landmarks_from_units)."""

    PARAMS = ('n_clusters', 'frames', 'max_span', 'max_frames', 'n_iter', 'seed')

    def __init__(self, n_clusters, frames=10, max_span=6, max_frames=None, n_iter=10, seed=0):
        if int(n_clusters) < 1 or int(frames) < 1 or int(max_span) < 1 or int(n_iter) < 1:
            raise ValueError('ESKMeans: n_clusters = %r, frames = %r, max_span = %r, n_iter = %r' % (n_clusters, frames, max_span, n_iter))
        if max_frames is not None and int(max_frames) < 1:
            raise ValueError('ESKMeans: max_frames = %r' % (max_frames,))
        self.n_clusters, self.frames, self.max_span = int(n_clusters), int(frames), int(max_span)
        self.max_frames = None if max_frames is None else int(max_frames)
        self.n_iter, self.seed = int(n_iter), int(seed)
        self.centroids_ = self.counts_ = None
        self.objective_, self.n_segments_ = [], []
        self.n_unreachable_ = self.n_empty_ = 0
        self._last = None               # (names, times, {name: (begin, end, ids)}) of the last segmentation

    def whoami(self):
        return {'params': {k: getattr(self, k) for k in self.PARAMS}, 'class_name': self.__class__.__name__}

    # -- inputs ---------------------------------------------------------------------------------------------------
    def _corpus(self, corpus, times):
        from .dataloader import DeviceCorpus
        if not isinstance(corpus, DeviceCorpus):
            for k, f in corpus.items():
                if np.asarray(f).dtype != np.float32:
                    raise ValueError('ESKMeans: features of %r are %s, float32 is needed' % (k, np.asarray(f).dtype))
            if times is None:
                times = {k: 0.01 * np.arange(np.asarray(f).shape[0], dtype=np.float64) for k, f in corpus.items()}
            corpus = DeviceCorpus(corpus, times)
        if self.n_clusters > kmeans.max_k():
            raise ValueError('ESKMeans: K = %d, the kernels take 1 .. %d (abn_kmeans_max_k)' % (self.n_clusters, kmeans.max_k()))
        if self.frames * corpus.dim > kmeans.max_d():
            raise ValueError('ESKMeans: frames x D = %d x %d, the kernels take up to %d (abn_kmeans_max_d)'
                             % (self.frames, corpus.dim, kmeans.max_d()))
        _check_span('ESKMeans', self.max_span)
        return corpus

    def _pack(self, corpus, landmarks):
        names, lm, lm_off = pack_landmarks(landmarks, corpus.offset, corpus.length, corpus.names)
        dev = corpus.table.device
        return names, lm, lm_off, torch.from_numpy(lm).to(dev), torch.from_numpy(lm_off).to(dev)

    def _vectors(self, table, lm, starts, spans):
        """The small table of the given segments' vectors."""
        return segment_vectors(table, lm[starts], (lm[starts + spans] - lm[starts]).astype(np.int32), self.frames)

    def _pass(self, table, lm_d, off_d, m, b):
        best, ids = candidate_scores(table, lm_d, off_d, m, b, self.frames, self.max_span, self.max_frames)
        return segment_dp(best, ids, lm_d, off_d, self.max_span)

    def _result(self, corpus, names, lm, lm_off, word, span):
        out = {}
        for u, k in enumerate(names):
            lo, hi = int(lm_off[u]), int(lm_off[u + 1])
            g = lo + np.flatnonzero(span[lo:hi] >= 1)
            base = int(corpus.offset[k])
            out[k] = (lm[g] - base, lm[g + span[g]] - base, word[g].astype(np.int32))
        self._last = (list(names), {k: corpus.times[k] for k in names}, out)
        return out

    # -- fit ------------------------------------------------------------------------------------------------------
    def iteration(self, table, lm, lm_d, off_d, st, shift):
        """One iteration in place in `st` (a kmeans.LloydState over frames D columns): score, DP, the one read-back,
        the chosen segments' vectors, accumulate and update.  Returns the host cut, word, span, objective, n_seg."""
        cut, word, span, obj, nseg = self._pass(table, lm_d, off_d, st.m, st.b)
        cut_h, word_h, span_h = cut.cpu().numpy(), word.cpu().numpy(), span.cpu().numpy()
        obj_h, nseg_h = obj.cpu().numpy(), nseg.cpu().numpy()
        g = np.flatnonzero(span_h >= 1)
        if len(g):
            vec, _ = self._vectors(table, lm, g, span_h[g])
            st.ids = torch.from_numpy(np.ascontiguousarray(word_h[g])).to(table.device)
            kmeans.accumulate(vec, shift, st)
        return cut_h, word_h, span_h, obj_h, nseg_h

    def fit(self, corpus, landmarks, init=None, times=None):
        corpus = self._corpus(corpus, times)
        table, K, Dv = corpus.table, self.n_clusters, self.frames * corpus.dim
        names, lm, lm_off, lm_d, off_d = self._pack(corpus, landmarks)
        rng = np.random.default_rng(self.seed)
        span0 = initial_spans(lm, lm_off, self.max_span, self.max_frames, rng)
        if init is not None:
            mu = np.array(init, dtype=np.float64)
            if mu.shape != (K, Dv) or not np.isfinite(mu).all():
                raise ValueError('ESKMeans.fit: init must be a finite [%d, %d] array' % (K, Dv))
        else:
            g0 = np.flatnonzero(span0 >= 1)
            vec, keep = self._vectors(table, lm, g0, span0[g0])
            rows = torch.nonzero(keep & torch.isfinite(vec).all(dim=1)).flatten()
            if int(rows.numel()) < K:
                raise ValueError('ESKMeans.fit: %d usable initial segments for K = %d centroids' % (int(rows.numel()), K))
            pick = np.sort(rng.choice(int(rows.numel()), K, replace=False))
            mu = vec[rows[torch.from_numpy(pick).to(rows.device)]].to(torch.float64).cpu().numpy()
        st = kmeans.LloydState(mu, 0, table.device)
        shift = torch.zeros(Dv, dtype=torch.float32, device=table.device)
        self.objective_, self.n_segments_ = [], []
        prev_cut = None
        for it in range(self.n_iter):
            cut_h, word_h, span_h, obj_h, nseg_h = self.iteration(table, lm, lm_d, off_d, st, shift)
            reach = nseg_h >= 0
            self.objective_.append(float(obj_h[reach].sum()))
            self.n_segments_.append(int(nseg_h[reach].sum()))
            self.n_unreachable_ = int((~reach).sum())
            if prev_cut is not None and np.array_equal(cut_h, prev_cut):
                break
            prev_cut = cut_h
        self.centroids_ = st.mu.cpu().numpy()
        self.counts_ = st.sums[:, -1].cpu().numpy()
        self.n_empty_ = int((self.counts_ == 0).sum())
        self.dim_ = int(corpus.dim)
        self._result(corpus, names, lm, lm_off, word_h, span_h)
        return self

    # -- use ------------------------------------------------------------------------------------------------------
    def segment(self, corpus, landmarks, times=None):
        """{name: (begin_frames, end_frames, ids)}: the segments of every utterance under the fitted centroids, frames
        begin .. end - 1 of the utterance (an unreachable utterance: empty arrays)."""
        if self.centroids_ is None:
            raise ValueError('ESKMeans: fit or load first')
        corpus = self._corpus(corpus, times)
        if self.centroids_.shape[1] != self.frames * corpus.dim:
            raise ValueError('ESKMeans: the corpus has D = %d, the model frames x D = %d' % (corpus.dim, self.centroids_.shape[1]))
        names, lm, lm_off, lm_d, off_d = self._pack(corpus, landmarks)
        m, b = (torch.from_numpy(a).to(corpus.table.device) for a in kmeans.score_tables(self.centroids_))
        _, word, span, obj, nseg = self._pass(corpus.table, lm_d, off_d, m, b)
        self.last_objective_, self.last_n_seg_ = obj.cpu().numpy(), nseg.cpu().numpy()
        return self._result(corpus, names, lm, lm_off, word.cpu().numpy(), span.cpu().numpy())

    def _need_last(self):
        if self._last is None:
            raise ValueError('ESKMeans: fit or segment first')
        return self._last

    def boundaries(self):
        """{file: float64 boundary times} of the last segmentation (fit's final one, or segment's), the form
        ``tde.boundary_scores`` takes: one boundary midway between the two frames of every interior cut."""
        names, times, seg = self._need_last()
        out = {}
        for k in names:
            t = np.asarray(times[k], dtype=np.float64).ravel()
            cutf = seg[k][0][1:]
            out[k.decode('UTF-8') if isinstance(k, bytes) else str(k)] = 0.5 * (t[cutf - 1] + t[cutf])
        return out

    @property
    def clusters(self):
        """The non-empty clusters of the last segmentation in id order, each a list of (file number, first frame, last
        frame) tokens: what ``terms.write_classes`` and ``tde.TermEvaluator.evaluate(clusters, names, times)`` take."""
        names, _, seg = self._need_last()
        by = {}
        for f, k in enumerate(names):
            for lo, hi, w in zip(*(a.tolist() for a in seg[k])):
                by.setdefault(w, []).append((f, lo, hi - 1))
        return [by[w] for w in sorted(by)]

    @property
    def names(self):
        return self._need_last()[0]

    @property
    def times(self):
        return self._need_last()[1]

    def term_scores(self, evaluator, words=None, speakers=None):
        """tde.FullTermScores of the last segmentation's clusters under a tde.TermEvaluator."""
        return evaluator.evaluate_full(self.clusters, self.names, self.times, words=words, speakers=speakers)

    def write_classes(self, path):
        from .terms import write_classes
        names, times, _ = self._need_last()
        return write_classes(path, names, times, self.clusters)

    # -- files ----------------------------------------------------------------------------------------------------
    def save(self, path):
        if self.centroids_ is None:
            raise ValueError('ESKMeans.save: fit first')
        with open(path, 'wb') as f:
            np.savez(f, esk_centroids=self.centroids_, counts=self.counts_, objective=np.asarray(self.objective_, dtype=np.float64),
                     n_segments=np.asarray(self.n_segments_, dtype=np.int64), n_clusters=self.n_clusters, frames=self.frames,
                     max_span=self.max_span, max_frames=-1 if self.max_frames is None else self.max_frames, n_iter=self.n_iter,
                     seed=self.seed, dim=self.dim_)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            if 'esk_centroids' not in z.files:
                raise ValueError('%s: not an ESKMeans file' % path)
            mf = int(z['max_frames'])
            self = cls(int(z['n_clusters']), int(z['frames']), int(z['max_span']), None if mf < 0 else mf, int(z['n_iter']), int(z['seed']))
            self.centroids_, self.counts_ = z['esk_centroids'].astype(np.float64), z['counts'].astype(np.float64)
            self.objective_ = [float(v) for v in z['objective']]
            self.n_segments_ = [int(v) for v in z['n_segments']]
            self.dim_ = int(z['dim'])
        if self.centroids_.shape != (self.n_clusters, self.frames * self.dim_):
            raise ValueError('%s: not an ESKMeans file' % path)
        self.n_empty_ = int((self.counts_ == 0).sum())
        return self


def parser():
    ap = argparse.ArgumentParser(prog='python -m abnet3_amd.eskmeans', description='ES-KMeans word segmentation of a feature file')
    sub = ap.add_subparsers(dest='cmd', required=True)
    f = sub.add_parser('fit', help='fit on FEATURES and save the centroids')
    f.add_argument('features', help='h5features file, or an .npz of name -> [T, D]')
    f.add_argument('model', help='the .npz to write')
    f.add_argument('-k', '--n-clusters', type=int, default=100)
    f.add_argument('--frames', type=int, default=10)
    f.add_argument('--max-span', type=int, default=6)
    f.add_argument('--max-frames', type=int, default=None)
    f.add_argument('--n-iter', type=int, default=10)
    f.add_argument('--seed', type=int, default=0)
    s = sub.add_parser('segment', help='segment FEATURES under saved centroids and write a .classes file')
    s.add_argument('model')
    s.add_argument('features', help='h5features file, or an .npz of name -> [T, D]')
    s.add_argument('out', help='the .classes file to write')
    for p in (f, s):
        p.add_argument('--step', type=int, default=5, help='a landmark every STEP frames (untuned)')
        p.add_argument('--units', default=None, metavar='NPZ', help='landmarks at the unit boundaries of name -> [T] ids '
                       '(python -m abnet3_amd.kmeans transform --penalty P) instead')
    return ap


def _landmarks(args, feats):
    if args.units is None:
        return uniform_landmarks(feats, args.step)
    with np.load(args.units) as z:
        ids = {k: z[k] for k in z.files}
    return landmarks_from_units(kmeans.segments(ids), {k: v.shape[0] for k, v in feats.items()})


def main(argv=None):
    from .gmm import _read_features
    args = parser().parse_args(argv)
    feats, times = _read_features(args.features)
    lms = _landmarks(args, feats)
    if args.cmd == 'fit':
        q = ESKMeans(args.n_clusters, args.frames, args.max_span, args.max_frames, args.n_iter, args.seed).fit(feats, lms, times=times)
        q.save(args.model)
        print('%d centroids, %d iterations, %d segments, objective %.6f, %d empty clusters, %d unreachable utterances'
              % (q.n_clusters, len(q.objective_), q.n_segments_[-1], q.objective_[-1], q.n_empty_, q.n_unreachable_))
        return 0
    q = ESKMeans.load(args.model)
    seg = q.segment(feats, lms, times=times)
    q.write_classes(args.out)
    print('%d files, %d segments in %d clusters -> %s' % (len(seg), sum(len(v[0]) for v in seg.values()), len(q.clusters), args.out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
