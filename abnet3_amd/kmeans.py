"""K-means discrete units on the MI355X: vector quantisation of frames or embeddings with no labels.

    python -m abnet3_amd.kmeans fit FEATURES MODEL.npz [-k K] [--n-iter N] [--tol T] [--metric M] [--seed S]
    python -m abnet3_amd.kmeans transform MODEL.npz FEATURES OUT [--quantize] [--penalty P] [--min-duration S]

Unit ids are how the ZeroSpeech 2019 / 2020 / 2021 systems are scored: the ids give the bitrate (``unit_sequences``,
``bitrate``), and ABX is run over the quantised frames (``quantize`` gives the corpus that ``ABXEvaluator`` and
``QbeSearcher`` read).  The centroids are also the usual initialiser of a mixture
(``GmmPosteriorgram.fit(..., init_means=km.centroids_)``).  The reference has no quantiser, so this definition is the
build's own, like the mixture's ("parity unpinned"); tests/kmeans_np.py restates it in numpy.

The definition this module computes:

* Model: K centroids over D-dimensional frames.  Parameters are float64 host arrays after ``fit``: ``centroids_``
  [K, D] and ``counts_`` [K]; ``shift_`` [D] is float32.  1 <= K <= 4096 (abn_kmeans_max_k, the mixture's limit),
  1 <= D <= 512 (abn_kmeans_max_d), checked on the host before any launch.
* metric='euclidean' (default): shift is the float64 mean of the good frames, rounded to fp32;  xc = fp32(x - shift),
  taken in fp32 on load;  m = centroid - shift, rounded once to fp32;  b[k] = fp32(-1/2 sum_d m[k, d]^2), the sum taken
  in float64 over the rounded m.
* metric='cosine' (spherical k-means): no shift (shift = 0);  xc = x / |x|, formed once by this layer with torch (fp32);
  an all-zero row is BAD;  b = 0;  the update renormalises each mean to unit length in float64.
* Score: s[t, k] = sum_d xc[t, d] m[k, d] + b[k]: one fp32 GEMM of depth D + 1 over [xc | 1] . [m | b], accumulated in
  that order on the matrix cores.  Neither augmented operand exists in memory, and no T x K array either.
* Assignment: a[t] = argmax_k s[t, k], int32; equal scores go to the lowest k.  A frame with a non-finite value -- in
  x, or in xc^2 by overflow -- is BAD: its id is -1, it contributes nothing, and it is counted (``n_bad_``).
* Update: N[k] = number of frames with a[t] = k,  S[k, d] = sum of xc[t, d] over them;  the frame's distortion is
  d2[t] = sum_d (xc[t, d] - m[a[t], d])^2, formed directly (not from |x|^2 - 2 s).  Partial sums are fp32 per (centroid,
  range of frames), taken in frame order (the distortions: float64 per lane); the partials are summed in index order in
  float64.  No floating-point atomics: two calls on the same input are bit-identical.  New centroid: S / N in float64;
  a centroid with N = 0 keeps its place and is counted (``n_empty_``).  Inertia: sum_t d2[t] / Tg, Tg = good frames.
* Initialisation: by default, as the mixture does it, the good frames at the sorted indices
  ``numpy.random.default_rng(seed).choice(Tg, K, replace=False)``; or a caller's [K, D] array (``init=``).  Fewer than K
  good frames raise ValueError.  (k-means++ and restarts are not provided.)
* Fit: iteration i assigns under the current centroids, ``inertias[i]`` is the inertia under those centroids and that
  assignment, then it updates.  It stops after n_iter iterations, or when no id changed since the previous iteration,
  or when (inertias[i - 1] - inertias[i]) / inertias[i - 1] < tol.  The number of changed ids is an integer counter the
  assign launch adds to.

Penalised segmentation (``segment``, ``predict(penalty=)``, ``quantize(penalty=)``, ``viterbi``): frame-wise ids flicker,
and every flicker is a symbol of the bitrate.  The ids are smoothed by a constant cost per new segment (Kamper & van
Niekerk 2021, "DPDP"), an HMM Viterbi with a uniform switching cost over the same scores (tests/units_np.py restates it):

* Inputs: the tables xc, m, b and the scores s[t, k] above: the same fp32 GEMM of depth D + 1, ka ascending, on the
  matrix cores.
* Chain: an utterance is a run of len[u] consecutive rows starting at off[u]; within it the chain runs over the good
  frames in order.  A BAD frame keeps id -1; the chain neither breaks there nor pays for it: the state passes through.
* ``penalty`` >= 0 is in the units of the distortion d2 = |xc - m|^2.  Since d2 = |xc|^2 - 2 s the kernel works with
  p = fp32(penalty / 2) in score units, for both metrics.  It has no tuned default: it trades bitrate against ABX and
  has to be swept on the data at hand.
* Objective: choose a[t] to maximise  J(a) = sum_t s[t, a_t] - p #{consecutive good frames with different ids}.
* Recurrence, all in fp32 and normalised so that nothing grows with T.  First good frame: U[k] = s[t, k].  Later good
  frames: stay[t, k] = (W[k] > -p) (strict), U[k] = s[t, k] + (stay[t, k] ? W[k] : -p).  Every good frame:
  M_t = max_k U[k], j*[t] = the lowest k attaining it, W[k] = U[k] - M_t.  objective[u] = the sum of the M_t in frame
  order, accumulated in float64.
* Traceback: the id of the last good frame is its j*; going backwards, the previous good frame's id is the same id if
  stay[t, a_t], otherwise j* of the previous good frame.  n_switch[u] = the number of switches on the path.
* The strict > is deliberate: with penalty = 0 nothing ever stays, every id is j*[t], and the result is
  abn_kmeans_assign's ids bit for bit.
* An utterance with no good frame gives all ids -1, objective 0 and 0 switches; len[u] = 0 is allowed.  Rows outside
  every utterance keep what ``ids`` held.
* Minimum duration (``min_duration`` = S, an integer 1 .. 8, default 1 = everything above; abnx_kmeans_viterbi_dur,
  csrc/vit_wave.h; tests/vit_dur_np.py restates it).  The penalty alone cannot remove one-frame units without smoothing
  real boundaries away; with S > 1 every unit becomes a left-to-right chain of S states over the same score, of which
  only the last may repeat.  Good frames only (BAD frames get -1 and are passed over; durations count good frames): a
  path is a sequence of segments (k_i, n_i), every segment but the utterance's last has n_i >= S (the end of the
  utterance may cut the last one short, so every length has a path), and its score is the sum of the frames' scores
  + lw[k_1] + lr[k_i] for each later segment + max(n_i - S, 0) ls[k_i], here with lw = 0, ls = 0, lr = -p: the
  objective J above, maximised over the labellings whose runs are long enough.  Recurrence, fp32, one rounded add or a
  compare per operation; V[k][0 .. S-1] the normalised previous values, E = max_k V[k][S-1], exitj the lowest k whose
  U[k][S-1] was the largest (0 if all are -inf):
    first good frame:   U[k][0] = s + lw[k], every other state -inf
    later good frames:  U[k][0] = s + (E + lr[k]);   U[k][i] = s + V[k][i-1] for 0 < i < S-1;
                        a = V[k][S-1] + ls[k],  st = a > V[k][S-2]  (strict: a tie goes to the advance),
                        U[k][S-1] = s + (st ? a : V[k][S-2])
    every good frame:   N_t = max over all (k, i) of U,  V = U - N_t,  objective = the sum of the N_t in float64.
  The final state is the lowest k, then the largest i, with V[k][i] == 0.  Stored per frame: the st bits and the previous
  good frame's exitj.  Going backwards: in state S-1 a set bit keeps (k, S-1) and a clear bit goes to (k, S-2); from state
  i, 0 < i < S-1, to (k, i-1); from state 0 to (exitj, S-1).  n_switch = the changes of id along the path.  The same
  workspace, still no T x K x S array: the S states of a centroid live in S registers of the lane that owns it.  No
  duration distribution, no maximum duration, and S is untuned on real speech.
* Limits: K <= abn_kmeans_viterbi_max_k() (4096), D <= abn_kmeans_max_d(), an utterance of at most
  abn_kmeans_viterbi_max_len() frames (2^20).  One launch (abn_kmeans_viterbi) for the whole corpus; no T x K array:
  the workspace is, per workgroup (at most 256), 128 x K scores, one stay bit per (frame of the longest utterance,
  centroid) and an int32 per frame.  With K <= 128 the score slab lives in LDS instead of the workspace.

On the device an iteration is abn_kmeans_assign, abn_kmeans_accumulate and abn_kmeans_update: four launches and one
read-back of five numbers for the stopping rule.
"""
import argparse
import sys

import numpy as np
import torch

from . import _lib
from . import _utt
from . import gmm as _gmm

METRICS = ('euclidean', 'cosine')


def max_d():
    return int(_lib.load().abn_kmeans_max_d())


def max_k():
    return int(_lib.load().abn_kmeans_max_k())


def _check_table(who, table, min_rows=0):
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.dtype != torch.float32:
        raise ValueError('%s: a [T, D] float32 table is needed, not %s' % (
            who, '%s %s' % (tuple(table.shape), table.dtype) if isinstance(table, torch.Tensor) else type(table).__name__))
    if table.shape[1] < 1 or table.shape[1] > max_d():
        raise ValueError('%s: D = %d, the kernels take 1 .. %d (abn_kmeans_max_d)' % (who, table.shape[1], max_d()))
    if table.shape[0] < min_rows:
        raise ValueError('%s: T = %d frames for K = %d centroids (T < K)' % (who, table.shape[0], min_rows))
    _lib.require_device(table)
    return table.contiguous()


def score_tables(mu, metric='euclidean'):
    """(m [K, D], b [K]) float32 host arrays of the float64 centred centroids."""
    m = np.asarray(mu, dtype=np.float64).astype(np.float32)
    if metric == 'cosine':
        return m, np.zeros(m.shape[0], dtype=np.float32)
    return m, (-0.5 * (m.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)


def _ws_bytes(T, K, D, n_ranges):
    need = _lib.load().abn_kmeans_ws_bytes(T, K, D, n_ranges)
    if need < 0:
        raise ValueError('kmeans: %s' % _lib.load().abn_last_error().decode('utf-8', 'replace'))
    return int(need)


def assign(table, shift, m, b, prev=None, ids=None, changed=None, want_best=False):
    """(ids [T] int32, best [T] or None) of the device table under the device tables (abn_kmeans_assign).  With `prev`
    (which may be `ids` itself) the number of ids that differ from it is added to `changed` (int32 [1], device)."""
    lib = _lib.load()
    table = _check_table('kmeans.assign', table)
    T, D = table.shape
    K = b.shape[0]
    _lib.require_device(shift, m, b)
    if m.shape != (K, D) or shift.shape != (D,) or any(t.dtype != torch.float32 for t in (shift, m, b)):
        raise ValueError('kmeans.assign: shift [D], m [K, D], b [K] float32 are needed')
    if K < 1 or K > max_k():
        raise ValueError('kmeans.assign: K = %d, the kernels take 1 .. %d (abn_kmeans_max_k)' % (K, max_k()))
    if ids is None:
        ids = torch.empty(T, dtype=torch.int32, device=table.device)
    assert ids.shape == (T,) and ids.dtype == torch.int32 and ids.is_contiguous()
    if prev is not None:
        assert prev.shape == (T,) and prev.dtype == torch.int32 and prev.is_contiguous()
        assert changed is not None and changed.dtype == torch.int32 and changed.numel() >= 1
    _lib.require_device(ids, prev, changed)
    best = torch.empty(T, dtype=torch.float32, device=table.device) if want_best else None
    if T:
        _lib.check(lib.abn_kmeans_assign(_lib.ptr(table), T, D, _lib.ptr(shift), _lib.ptr(m), _lib.ptr(b), K, _lib.ptr(prev),
                                         _lib.ptr(ids), _lib.ptr(best), _lib.ptr(changed if prev is not None else None),
                                         _lib.stream()), 'abn_kmeans_assign')
    return ids, best


def viterbi_max_len():
    return int(_lib.load().abn_kmeans_viterbi_max_len())


def viterbi_max_k():
    return int(_lib.load().abn_kmeans_viterbi_max_k())


def check_penalty(who, penalty):
    try:
        p = float(penalty)
    except (TypeError, ValueError):
        raise ValueError('%s: penalty = %r, a finite number >= 0 is needed' % (who, penalty))
    if not (p >= 0.0 and p / 2.0 <= float(np.finfo(np.float32).max)):
        raise ValueError('%s: penalty = %r, a finite number >= 0 is needed' % (who, penalty))
    return p


def viterbi(table, off, lens, shift, m, b, penalty, ids=None, want_objective=False, min_duration=1):
    """(ids [T] int32, objective [n_utt] float64 or None, n_switch [n_utt] int32 or None) of the penalised segmentation
    the module docstring defines (abn_kmeans_viterbi, one launch).  off, lens: the utterances' first rows and lengths
    (host sequences or device tensors); they must not overlap.  Rows outside every utterance keep what `ids` held (-1
    in a fresh `ids`).  min_duration = S > 1: every unit lasts at least S good frames (abnx_kmeans_viterbi_dur, the same
    workspace); 1 is abn_kmeans_viterbi itself."""
    lib = _lib.load()
    penalty = check_penalty('kmeans.viterbi', penalty)
    min_duration = _utt.check_min_duration('kmeans.viterbi', min_duration)
    table = _check_table('kmeans.viterbi', table)
    T, D = table.shape
    K = b.shape[0]
    _lib.require_device(shift, m, b)
    if m.shape != (K, D) or shift.shape != (D,) or any(t.dtype != torch.float32 for t in (shift, m, b)):
        raise ValueError('kmeans.viterbi: shift [D], m [K, D], b [K] float32 are needed')
    if K < 1 or K > viterbi_max_k():
        raise ValueError('kmeans.viterbi: K = %d, the kernel takes 1 .. %d (abn_kmeans_viterbi_max_k)' % (K, viterbi_max_k()))
    off_h, len_h, n_utt, max_len = _utt.utterance_spans('kmeans.viterbi', off, lens, T, viterbi_max_len(), 'abn_kmeans_viterbi_max_len')
    if ids is None:
        ids = torch.full((T,), -1, dtype=torch.int32, device=table.device)
    if ids.shape != (T,) or ids.dtype != torch.int32 or not ids.is_contiguous():
        raise ValueError('kmeans.viterbi: ids must be a contiguous [T] int32 tensor')
    _lib.require_device(ids)
    obj = torch.zeros(n_utt, dtype=torch.float64, device=table.device) if want_objective else None
    nsw = torch.zeros(n_utt, dtype=torch.int32, device=table.device) if want_objective else None
    if T and n_utt and max_len:
        ws, off_d, len_d = _utt.workspace('kmeans.viterbi', lib.abn_kmeans_viterbi_ws_bytes, off_h, len_h, max_len, K, D, table.device)
        args = (_lib.ptr(table), T, D, _lib.ptr(off_d), _lib.ptr(len_d), n_utt, _lib.ptr(shift), _lib.ptr(m), _lib.ptr(b), K,
                float(np.float32(penalty / 2.0)), _lib.ptr(ids), _lib.ptr(obj), _lib.ptr(nsw), _lib.ptr(ws), ws.numel(), _lib.stream())
        if min_duration == 1:
            _lib.check(lib.abn_kmeans_viterbi(*args), 'abn_kmeans_viterbi')
        else:
            _lib.check(lib.abnx_kmeans_viterbi_dur(*(args + (min_duration,))), 'abnx_kmeans_viterbi_dur')
    return ids, obj, nsw


class LloydState(object):
    """The device side of a fit: float64 centred centroids mu, the fp32 tables (m, b), the ids of the last assignment,
    the counter of changed ids, the statistics of the last iteration (sums [K, D + 1] = [S | N]) and stats [4] = (sum
    of the distortions, BAD frames, empty centroids, good frames)."""

    def __init__(self, mu, T, device, metric='euclidean'):
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
        self.K, self.D = mu.shape
        self.cosine = int(metric == 'cosine')
        self.mu = dev(mu, np.float64)
        self.m, self.b = (dev(a, np.float32) for a in score_tables(mu, metric))
        self.ids = torch.full((T,), -2, dtype=torch.int32, device=device)
        self.changed = torch.zeros(1, dtype=torch.int32, device=device)
        self.sums = torch.zeros((self.K, self.D + 1), dtype=torch.float64, device=device)
        self.stats = torch.zeros(4, dtype=torch.float64, device=device)
        self.ws = None
        self.assigned = False


def accumulate(table, shift, st, n_ranges=0, update=True):
    """abn_kmeans_accumulate and abn_kmeans_update for the ids in `st`; update=False leaves the centroids alone
    (statistics only).  Nothing is read back."""
    lib = _lib.load()
    table = _check_table('kmeans.accumulate', table)
    T, D = table.shape
    _lib.require_device(shift)
    if D != st.D or shift.shape != (D,) or shift.dtype != torch.float32 or st.ids.shape != (T,):
        raise ValueError('kmeans.accumulate: a [%d, %d] table (the state\'s ids and D) and shift [D] float32 are needed'
                         % (st.ids.shape[0], st.D))
    need = _ws_bytes(T, st.K, D, n_ranges)
    if st.ws is None or st.ws.numel() < need:
        st.ws = torch.empty(max(need, 16), dtype=torch.uint8, device=table.device)
    _lib.check(lib.abn_kmeans_accumulate(_lib.ptr(table), T, D, _lib.ptr(shift), _lib.ptr(st.m), st.K, _lib.ptr(st.ids),
                                         n_ranges, _lib.ptr(st.ws), st.ws.numel(), _lib.stream()), 'abn_kmeans_accumulate')
    out = (st.mu, st.m, st.b) if update else (None, None, None)
    _lib.check(lib.abn_kmeans_update(_lib.ptr(st.ws), st.ws.numel(), _lib.ptr(st.ids), T, st.K, D, n_ranges, st.cosine,
                                     _lib.ptr(st.sums), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]),
                                     _lib.ptr(st.stats), _lib.stream()), 'abn_kmeans_update')


def lloyd_iteration(table, shift, st, n_ranges=0):
    """One Lloyd iteration on the device, in place in `st` (a LloydState): abn_kmeans_assign (the changed ids are
    counted from the second call on), abn_kmeans_accumulate, abn_kmeans_update.  Nothing is read back."""
    st.changed.zero_()
    assign(table, shift, st.m, st.b, prev=st.ids if st.assigned else None, ids=st.ids, changed=st.changed)
    st.assigned = True
    accumulate(table, shift, st, n_ranges)


def prepare(table, metric):
    """(xc source table, shift [D] float32 device, good [T] bool device): the euclidean metric centres on load, on the
    float64 mean of the frames without a non-finite value; the cosine metric scales each row to unit length here."""
    D = table.shape[1]
    if metric == 'cosine':
        table = table / table.norm(dim=1, keepdim=True)
        shift = torch.zeros(D, dtype=torch.float32, device=table.device)
        return table, shift, torch.isfinite(table * table).all(dim=1)
    fin = torch.isfinite(table).all(dim=1)
    if not bool(fin.any()):
        raise ValueError('KMeansQuantizer.fit: the table has no frame without a non-finite value')
    shift = table[fin].to(torch.float64).mean(dim=0).to(torch.float32)
    xc = table - shift
    return table, shift, torch.isfinite(xc * xc).all(dim=1)


def initial_centroids(table, shift, good, K, seed, metric='euclidean', init=None):
    """float64 host array [K, D] of the centred centroids of the documented initialisation."""
    rows = torch.nonzero(good).flatten()
    Tg = int(rows.numel())
    if Tg < K:
        raise ValueError('KMeansQuantizer.fit: %d good frames for K = %d centroids (T < K)' % (Tg, K))
    if init is not None:
        mu = np.array(init, dtype=np.float64)
        if mu.shape != (K, table.shape[1]) or not np.isfinite(mu).all():
            raise ValueError('KMeansQuantizer.fit: init must be a finite [%d, %d] array' % (K, table.shape[1]))
        if metric == 'cosine':
            return mu / np.sqrt((mu * mu).sum(axis=1, keepdims=True))
        return mu - shift.cpu().numpy().astype(np.float64)
    pick = np.sort(np.random.default_rng(seed).choice(Tg, K, replace=False))
    return (table[rows[torch.from_numpy(pick).to(rows.device)]] - shift).to(torch.float64).cpu().numpy()


class KMeansQuantizer(object):
    """fit / predict / quantize / score of the quantiser the module docstring defines.

    corpus arguments: a DeviceCorpus, a {name: [T, D]} dict, a [T, D] float32 device table, or the path of an
    h5features file (needs the h5features package)."""

    def __init__(self, n_clusters, n_iter=20, tol=1e-4, metric='euclidean', seed=0):
        if int(n_clusters) < 1:
            raise ValueError('KMeansQuantizer: n_clusters = %r' % (n_clusters,))
        if metric not in METRICS:
            raise ValueError('KMeansQuantizer: metric = %r, one of %s' % (metric, ', '.join(METRICS)))
        self.n_clusters, self.n_iter, self.tol = int(n_clusters), int(n_iter), float(tol)
        self.metric, self.seed = metric, int(seed)
        self.centroids_ = self.counts_ = self.shift_ = None
        self.inertias = []
        self.n_changed = []             # per iteration: ids that differ from the previous iteration's (None for the first)
        self.n_bad_ = self.n_empty_ = 0
        self.last_objective_ = self.last_n_switch_ = None      # segment(): per utterance, in corpus order
        self._tables = None

    def whoami(self):
        return {'params': {k: getattr(self, k) for k in ('n_clusters', 'n_iter', 'tol', 'metric', 'seed')},
                'class_name': self.__class__.__name__}

    # -- inputs ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _corpus(corpus):
        """(device table, DeviceCorpus or None, {name: rows} or None)"""
        from .dataloader import DeviceCorpus
        if isinstance(corpus, str):
            from .abx import _read_h5features
            corpus = DeviceCorpus(*_read_h5features(corpus))
        if isinstance(corpus, DeviceCorpus):
            return corpus.table, corpus, {k: corpus.length[k] for k in corpus.names}
        if isinstance(corpus, dict):
            for k, f in corpus.items():
                if np.asarray(f).dtype != np.float32:
                    raise ValueError('KMeansQuantizer: features of %r are %s, float32 is needed' % (k, np.asarray(f).dtype))
            table = torch.from_numpy(np.concatenate([np.asarray(f) for f in corpus.values()], axis=0)).cuda()
            return table, None, {k: np.asarray(f).shape[0] for k, f in corpus.items()}
        return corpus, None, None

    def _check_k(self):
        if self.n_clusters > max_k():
            raise ValueError('KMeansQuantizer: K = %d, the kernels take 1 .. %d (abn_kmeans_max_k)' % (self.n_clusters, max_k()))

    # -- fit ------------------------------------------------------------------------------------------------------
    def fit(self, corpus, init=None, n_ranges=0):
        self._check_k()
        table, _, _ = self._corpus(corpus)
        K = self.n_clusters
        table = _check_table('KMeansQuantizer.fit', table, min_rows=K)
        table, shift, good = prepare(table, self.metric)
        mu = initial_centroids(table, shift, good, K, self.seed, self.metric, init)
        st = LloydState(mu, table.shape[0], table.device, self.metric)
        self.inertias, self.n_changed = [], []
        for it in range(self.n_iter):
            lloyd_iteration(table, shift, st, n_ranges)
            d2_sum, bad, empty, tg, changed = torch.cat([st.stats, st.changed.to(torch.float64)]).cpu().tolist()   # the iteration's one read-back
            self.inertias.append(d2_sum / tg)
            self.n_changed.append(int(changed) if it > 0 else None)
            self.n_bad_, self.n_empty_ = int(bad), int(empty)
            if it > 0:
                before, now = self.inertias[-2], self.inertias[-1]
                if changed == 0 or before <= 0.0 or (before - now) / before < self.tol:
                    break
        self.shift_ = shift.cpu().numpy()
        self.centroids_ = st.mu.cpu().numpy() + self.shift_.astype(np.float64)
        self.counts_ = st.sums[:, -1].cpu().numpy()
        self._tables = None
        return self

    # -- use ------------------------------------------------------------------------------------------------------
    def device_tables(self, device):
        """(shift, m, b, centroids as float32) on the device, rounded once from the float64 parameters."""
        if self.centroids_ is None:
            raise ValueError('KMeansQuantizer: fit or load first')
        if self._tables is None or self._tables[0].device != device:
            mu = self.centroids_ - self.shift_.astype(np.float64)
            self._tables = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in
                                 (self.shift_,) + score_tables(mu, self.metric) + (self.centroids_.astype(np.float32),))
        return self._tables

    def _assign(self, table, want_state=False, n_ranges=0):
        if self.centroids_ is None:
            raise ValueError('KMeansQuantizer: fit or load first')
        table = _check_table('KMeansQuantizer', table)
        if table.shape[1] != self.shift_.shape[0]:
            raise ValueError('KMeansQuantizer: the table has D = %d, the model D = %d' % (table.shape[1], self.shift_.shape[0]))
        if self.metric == 'cosine':
            table = table / table.norm(dim=1, keepdim=True)
        shift, m, b, _ = self.device_tables(table.device)
        if not want_state:
            return assign(table, shift, m, b)[0]
        st = LloydState(self.centroids_ - self.shift_.astype(np.float64), table.shape[0], table.device, self.metric)
        assign(table, shift, st.m, st.b, ids=st.ids)
        if table.shape[0]:
            accumulate(table, shift, st, n_ranges, update=False)
        return st

    def _segment_ids(self, table, rows, penalty, min_duration=1):
        """Device ids of the penalised segmentation; fills last_objective_ / last_n_switch_."""
        penalty = check_penalty('KMeansQuantizer.segment', penalty)
        min_duration = _utt.check_min_duration('KMeansQuantizer.segment', min_duration)
        if self.centroids_ is None:
            raise ValueError('KMeansQuantizer: fit or load first')
        lens = np.array([table.shape[0]] if rows is None else list(rows.values()), dtype=np.int64)
        if isinstance(table, torch.Tensor) and table.dim() == 2 and table.dtype == torch.float32:      # (host checks first)
            if table.shape[1] != self.shift_.shape[0]:
                raise ValueError('KMeansQuantizer: the table has D = %d, the model D = %d' % (table.shape[1], self.shift_.shape[0]))
            if self.n_clusters > viterbi_max_k():
                raise ValueError('KMeansQuantizer.segment: K = %d, the kernel takes 1 .. %d (abn_kmeans_viterbi_max_k)'
                                 % (self.n_clusters, viterbi_max_k()))
            if len(lens) and int(lens.max()) > viterbi_max_len():
                raise ValueError('KMeansQuantizer.segment: an utterance of %d frames, the kernel takes up to %d '
                                 '(abn_kmeans_viterbi_max_len); pass a corpus of utterances' % (int(lens.max()), viterbi_max_len()))
        table = _check_table('KMeansQuantizer.segment', table)
        off = _utt.starts(lens)
        if self.metric == 'cosine':
            table = table / table.norm(dim=1, keepdim=True)
        shift, m, b, _ = self.device_tables(table.device)
        ids, obj, nsw = viterbi(table, off, lens, shift, m, b, penalty, want_objective=True, min_duration=min_duration)
        self.last_objective_, self.last_n_switch_ = obj.cpu().numpy(), nsw.cpu().numpy()
        return ids

    @staticmethod
    def _duration(who, min_duration):
        """The keyword that hands a checked min_duration on: none at 1, where every call is the one it was without it."""
        min_duration = _utt.check_min_duration(who, min_duration)
        return {} if min_duration == 1 else {'min_duration': min_duration}

    @staticmethod
    def _by_name(ids, rows):
        return ids if rows is None else _gmm._split_rows(ids.cpu().numpy(), rows.items())

    def segment(self, corpus, penalty, min_duration=1):
        """The unit ids of the penalised segmentation (module docstring), in predict's forms.  Each file of a corpus is
        an utterance; a [T, D] table is ONE utterance (ValueError beyond abn_kmeans_viterbi_max_len frames).
        ``last_objective_`` (float64) and ``last_n_switch_`` (int32) hold the utterances' objectives and switch counts.
        min_duration = S (an integer 1 .. 8): every unit but an utterance's last lasts at least S good frames."""
        extra = self._duration('KMeansQuantizer.segment', min_duration)
        table, _, rows = self._corpus(corpus)
        return self._by_name(self._segment_ids(table, rows, penalty, **extra), rows)

    def predict(self, corpus, penalty=None, min_duration=1):
        """The unit ids, int32, -1 for a BAD frame: a device tensor [rows] for a table, {name: host array} in corpus
        order for a DeviceCorpus, a dict or a file.  penalty=None: the frame-wise ids; a number: ``segment`` (with its
        min_duration; without a penalty min_duration must be 1)."""
        if penalty is not None:
            return self.segment(corpus, penalty, min_duration)
        if self._duration('KMeansQuantizer.predict', min_duration):
            raise ValueError('KMeansQuantizer.predict: min_duration = %d needs a penalty (0 is one)' % min_duration)
        table, _, rows = self._corpus(corpus)
        return self._by_name(self._assign(table), rows)

    def quantize(self, corpus, penalty=None, min_duration=1):
        """Each frame replaced by its centroid, [rows, D] float32 on the device (a BAD frame: zeros); for a DeviceCorpus
        a new DeviceCorpus with the same names, lengths and times.  penalty: the ids of ``segment`` (with its
        min_duration) instead of the frame-wise ones; without a penalty min_duration must be 1."""
        from .dataloader import DeviceCorpus
        extra = self._duration('KMeansQuantizer.quantize', min_duration)
        if penalty is None and extra:
            raise ValueError('KMeansQuantizer.quantize: min_duration = %d needs a penalty (0 is one)' % min_duration)
        table, dc, rows = self._corpus(corpus)
        ids = self._assign(table) if penalty is None else self._segment_ids(table, rows, penalty, **extra)
        cent = self.device_tables(ids.device)[3]
        out = cent[ids.clamp(min=0).to(torch.int64)]
        out[ids < 0] = 0.0
        if dc is None:
            return out
        return DeviceCorpus.from_table(out, dc.names, [dc.length[k] for k in dc.names], dc.times)

    def score(self, corpus):
        """The mean distortion over the good frames."""
        table, _, _ = self._corpus(corpus)
        st = self._assign(table, want_state=True)
        d2_sum, _, _, tg = st.stats.cpu().tolist()
        return d2_sum / max(1.0, tg)

    # -- files ----------------------------------------------------------------------------------------------------
    def save(self, path):
        if self.centroids_ is None:
            raise ValueError('KMeansQuantizer.save: fit first')
        with open(path, 'wb') as f:
            np.savez(f, centroids=self.centroids_, counts=self.counts_, shift=self.shift_,
                     inertias=np.asarray(self.inertias, dtype=np.float64), n_clusters=self.n_clusters, n_iter=self.n_iter,
                     tol=self.tol, metric=self.metric, seed=self.seed, n_bad=self.n_bad_, n_empty=self.n_empty_)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            if 'centroids' not in z.files:
                raise ValueError('%s: not a KMeansQuantizer file' % path)
            self = cls(int(z['n_clusters']), int(z['n_iter']), float(z['tol']), str(z['metric']), int(z['seed']))
            self.centroids_, self.counts_ = z['centroids'].astype(np.float64), z['counts'].astype(np.float64)
            self.shift_ = z['shift'].astype(np.float32)
            self.inertias = [float(v) for v in z['inertias']]
            self.n_bad_, self.n_empty_ = int(z['n_bad']), int(z['n_empty'])
        if self.centroids_.shape != (self.n_clusters, self.shift_.shape[0]) or self.counts_.shape != (self.n_clusters,):
            raise ValueError('%s: not a KMeansQuantizer file' % path)
        return self


def unit_sequences(ids_by_name, collapse=True):
    """{name: int array}: each file's unit ids without the BAD frames' -1; collapse=True merges runs of equal ids."""
    out = {}
    for k, ids in ids_by_name.items():
        a = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids).astype(np.int64).ravel()
        a = a[a >= 0]
        if collapse and a.size:
            a = a[np.concatenate(([True], a[1:] != a[:-1]))]
        out[k] = a
    return out


def segments(ids_by_name):
    """{name: (start, end, unit) int64 arrays}: the runs of equal ids of each file, frames start .. end - 1; the BAD
    frames (id -1) are left out, and a BAD frame ends a run."""
    out = {}
    for k, ids in ids_by_name.items():
        a = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids).astype(np.int64).ravel()
        if not a.size:
            out[k] = tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
            continue
        start = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))
        end = np.concatenate((start[1:], [a.size]))
        keep = a[start] >= 0
        out[k] = (start[keep], end[keep], a[start][keep])
    return out


def bitrate(sequences, total_seconds):
    """(n / total_seconds) H, n the number of symbols of all sequences and H = -sum p log2 p over the symbol
    distribution of the whole set: the ZeroSpeech 2019 bitrate, in bits per second."""
    if not total_seconds > 0:
        raise ValueError('bitrate: total_seconds = %r' % (total_seconds,))
    seqs = sequences.values() if isinstance(sequences, dict) else sequences
    syms = np.concatenate([np.asarray(s).ravel() for s in seqs] + [np.zeros(0, dtype=np.int64)])
    if syms.size == 0:
        return 0.0
    _, cnt = np.unique(syms, return_counts=True)
    p = cnt / float(syms.size)
    return float(syms.size / float(total_seconds) * -(p * np.log2(p)).sum())


def parser():
    ap = argparse.ArgumentParser(prog='python -m abnet3_amd.kmeans', description='K-means discrete units of a feature file')
    sub = ap.add_subparsers(dest='cmd', required=True)
    f = sub.add_parser('fit', help='fit a quantiser on FEATURES and save it')
    f.add_argument('features', help='h5features file, or an .npz of name -> [T, D]')
    f.add_argument('model', help='the .npz to write')
    f.add_argument('-k', '--n-clusters', type=int, default=50)
    f.add_argument('--n-iter', type=int, default=20)
    f.add_argument('--tol', type=float, default=1e-4)
    f.add_argument('--metric', choices=METRICS, default='euclidean')
    f.add_argument('--seed', type=int, default=0)
    t = sub.add_parser('transform', help='unit ids (or quantised frames) of FEATURES under a saved quantiser')
    t.add_argument('model')
    t.add_argument('features', help='h5features file, or an .npz of name -> [T, D]')
    t.add_argument('out', help='.npz of name -> [T] ids or [T, D] frames, or an h5features file (when the input has times)')
    t.add_argument('--quantize', action='store_true', help='write each frame\'s centroid instead of its id')
    t.add_argument('--penalty', type=float, default=None, metavar='P',
                   help='penalised segmentation: cost of a new segment, in units of the distortion (no tuned default)')
    t.add_argument('--min-duration', type=int, default=1, metavar='S',
                   help='with --penalty: every unit lasts at least S frames (1 .. 8; default 1, no minimum)')
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    feats, times = _gmm._read_features(args.features)
    if args.cmd == 'fit':
        q = KMeansQuantizer(args.n_clusters, args.n_iter, args.tol, args.metric, args.seed).fit(feats)
        q.save(args.model)
        print('%d centroids, %d iterations, inertia %.6f, %d BAD frames, %d empty centroids'
              % (q.n_clusters, len(q.inertias), q.inertias[-1], q.n_bad_, q.n_empty_))
        return 0
    q = KMeansQuantizer.load(args.model)
    if args.quantize:
        out = _gmm._split_rows(q.quantize(feats, penalty=args.penalty, min_duration=args.min_duration).cpu().numpy(),
                               ((k, v.shape[0]) for k, v in feats.items()))
    else:
        out = q.predict(feats, penalty=args.penalty, min_duration=args.min_duration)
    _gmm._write_named(args.out, out, times, as_column=not args.quantize)
    print('%d files, %d frames, K = %d -> %s' % (len(out), sum(v.shape[0] for v in out.values()), q.n_clusters, args.out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
