"""Gaussian posteriorgrams on the MI355X: a diagonal-covariance mixture fitted on raw features with no labels.

    python -m abnet3_amd.gmm fit FEATURES MODEL.npz [-k K] [--n-iter N] [--tol T] [--var-floor F] [--seed S]
    python -m abnet3_amd.gmm transform MODEL.npz FEATURES OUT

The per-frame component posteriors of such a mixture are the "Gaussian posteriorgram" of Zhang & Glass (2009), the
classic zero-resource input of query-by-example search and the baseline of every ABX table: ``transform`` gives
the [rows, K] table that ``ABXEvaluator(distance='kl')`` and ``QbeSearcher(distance='kl')`` read.  The reference
has no mixture model, so this definition is the build's own, like the DTW recurrence and the KL frame distance
("parity unpinned"); tests/gmm_np.py restates it in numpy.

The definition this module computes:

* Model: K components over D-dimensional frames, diagonal covariance: weights w [K], means mu [K, D], variances
  v [K, D], and a fixed shift [D] (float32), the per-dimension mean of the training table.  Parameters are float64
  (``weights_``, ``means_``, ``variances_``; host arrays after ``fit``).
* Centred frame: xc = float32(x - shift), taken in fp32 on load; everything below is defined on xc, so tables that
  were not mean-normalised do not lose the fp32 expansion to cancellation.
* Score tables, float32, rounded once from float64 with m = mu - shift:
  A = m / v,  B = -0.5 / v,  c[k] = log w[k] - 0.5 sum_d (log(2 pi v[k, d]) + m[k, d]^2 / v[k, d]).
* Score: s[t, k] = c[k] + sum_d xc[t, d] A[k, d] + sum_d xc[t, d]^2 B[k, d]: one fp32 GEMM of depth 2D + 1 over the
  augmented row [xc | xc^2 | 1] (xc^2 rounded to fp32), accumulated in that order on the matrix cores.
* Frame log-likelihood: lse[t] = max_k s + log sum_k exp(s - max);  posterior: g[t, k] = exp(s[t, k] - lse[t]).
* A frame with a non-finite value -- in x, or in xc^2 by overflow -- is BAD: its lse is NaN, its posterior row all
  zeros, it contributes nothing to the statistics, and it is counted (``n_bad_``).
* Sufficient statistics: N[k] = sum_t g,  S1[k, d] = sum_t g xc,  S2[k, d] = sum_t g xc^2.  Partial sums are fp32
  per (tile of 128 components, range of frames) slab; the slabs are summed in index order in float64.  No
  floating-point atomics: two calls on the same input are bit-identical.
* M-step, float64, Tg = number of good frames:  w = N / Tg,  m = S1 / N,  v = max(S2 / N - m^2, var_floor gv[d]),
  gv the per-dimension variance of the training table.  A component with N[k] < min_count keeps its mean and
  variance; its weight is N[k] / Tg like the others; then the weights are renormalised to sum 1.  The number of
  such components is reported (``n_starved_``).
* Initialisation: the means are K distinct good frames of the training table, those at the sorted indices
  ``numpy.random.default_rng(seed).choice(Tg, K, replace=False)`` into the good frames;  v = gv;  w = 1 / K.
  Fewer than K (good) frames raise ValueError.
* Fit: iteration i computes lse under the current parameters (``log_likelihoods[i]`` is its mean over the good
  frames), then applies the M-step.  After at most n_iter iterations, or as soon as log_likelihoods[i] -
  log_likelihoods[i - 1] < tol, it stops.

On the device an iteration is abn_gmm_posteriors (likelihoods only), abn_gmm_accumulate and abn_gmm_mstep: four
launches, no T x K matrix, and one read-back of four numbers for the stopping rule.
"""
import argparse
import sys

import numpy as np
import torch

from . import _lib

TRANSFORM_CHUNK = 1 << 20          # rows per abn_gmm_posteriors call of transform / score


def max_d():
    return int(_lib.load().abn_gmm_max_d())


def max_k():
    return int(_lib.load().abn_gmm_max_k())


def _check_table(who, table, min_rows=0):
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.dtype != torch.float32:
        raise ValueError('%s: a [T, D] float32 table is needed, not %s' % (
            who, '%s %s' % (tuple(table.shape), table.dtype) if isinstance(table, torch.Tensor) else type(table).__name__))
    if table.shape[1] < 1 or table.shape[1] > max_d():
        raise ValueError('%s: D = %d, the kernels take 1 .. %d (abn_gmm_max_d)' % (who, table.shape[1], max_d()))
    if table.shape[0] < min_rows:
        raise ValueError('%s: T = %d frames for K = %d components (T < K)' % (who, table.shape[0], min_rows))
    _lib.require_device(table)
    return table.contiguous()


def score_tables(w, m, v):
    """(A, B, c) float32 host arrays of float64 weights [K], centred means [K, D] and variances [K, D]."""
    w, m, v = (np.asarray(a, dtype=np.float64) for a in (w, m, v))
    with np.errstate(divide='ignore'):
        c = np.log(w) - 0.5 * (np.log(2.0 * np.pi * v) + m * m / v).sum(axis=1)
    return (m / v).astype(np.float32), (-0.5 / v).astype(np.float32), c.astype(np.float32)


def posteriors(table, shift, A, B, c, want_post=True, out=None):
    """(lse [T], g [T, K] or None) of the device table under the device score tables (abn_gmm_posteriors)."""
    lib = _lib.load()
    table = _check_table('gmm.posteriors', table)
    T, D = table.shape
    K = c.shape[0]
    _lib.require_device(shift, A, B, c)
    if A.shape != (K, D) or B.shape != (K, D) or shift.shape != (D,) or any(
            t.dtype != torch.float32 for t in (shift, A, B, c)):
        raise ValueError('gmm.posteriors: shift [D], A [K, D], B [K, D], c [K] float32 are needed')
    if K > max_k():
        raise ValueError('gmm.posteriors: K = %d, the kernels take 1 .. %d (abn_gmm_max_k)' % (K, max_k()))
    lse = torch.empty(T, dtype=torch.float32, device=table.device)
    g = None
    if want_post:
        g = out if out is not None else torch.empty((T, K), dtype=torch.float32, device=table.device)
        assert g.shape == (T, K) and g.dtype == torch.float32 and g.is_contiguous()
        _lib.require_device(g)
    if T:
        _lib.check(lib.abn_gmm_posteriors(_lib.ptr(table), T, D, _lib.ptr(shift), _lib.ptr(A), _lib.ptr(B), _lib.ptr(c), K,
                                          _lib.ptr(lse), _lib.ptr(g), _lib.stream()), 'abn_gmm_posteriors')
    return lse, g


class EMState(object):
    """The device side of a fit: float64 parameters (w, centred means mu, variances var), the fp32 score tables, the
    statistics of the last iteration (sums [K, 2D + 1] = [S1 | S2 | N]) and stats [4] = (sum of lse over the good
    frames, BAD frames, starved components, good frames)."""

    def __init__(self, w, m, v, gv, device):
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
        self.K, self.D = m.shape
        self.w, self.mu, self.var, self.gv = dev(w, np.float64), dev(m, np.float64), dev(v, np.float64), dev(gv, np.float64)
        self.A, self.B, self.c = (dev(a, np.float32) for a in score_tables(w, m, v))
        self.sums = torch.zeros((self.K, 2 * self.D + 1), dtype=torch.float64, device=device)
        self.stats = torch.zeros(4, dtype=torch.float64, device=device)
        self.ws = None


def em_iteration(table, shift, st, var_floor=0.01, min_count=1.0, n_ranges=0):
    """One EM iteration on the device, in place in `st` (an EMState): abn_gmm_posteriors (likelihoods only),
    abn_gmm_accumulate, abn_gmm_mstep.  Returns lse [T].  Nothing is read back."""
    lib = _lib.load()
    table = _check_table('gmm.em_iteration', table)       # (the dense copy of a strided table: all three launches read it)
    T, D = table.shape
    if D != st.D:
        raise ValueError('gmm.em_iteration: D = %d, the state was built for D = %d' % (D, st.D))
    lse, _ = posteriors(table, shift, st.A, st.B, st.c, want_post=False)
    need = lib.abn_gmm_ws_bytes(T, st.K, D, n_ranges)
    if need < 0:
        raise ValueError('gmm: %s' % lib.abn_last_error().decode('utf-8', 'replace'))
    if st.ws is None or st.ws.numel() < need:
        st.ws = torch.empty(max(need, 16), dtype=torch.uint8, device=table.device)
    head = [_lib.ptr(table), T, D, _lib.ptr(shift), _lib.ptr(st.A), _lib.ptr(st.B), _lib.ptr(st.c), st.K]
    _lib.check(lib.abn_gmm_accumulate(*(head + [_lib.ptr(lse), n_ranges, _lib.ptr(st.ws), st.ws.numel(), _lib.stream()])),
               'abn_gmm_accumulate')
    _lib.check(lib.abn_gmm_mstep(_lib.ptr(st.ws), st.ws.numel(), _lib.ptr(lse), T, st.K, D, n_ranges, _lib.ptr(st.gv),
                                 float(var_floor), float(min_count), _lib.ptr(st.sums), _lib.ptr(st.w), _lib.ptr(st.mu),
                                 _lib.ptr(st.var), _lib.ptr(st.A), _lib.ptr(st.B), _lib.ptr(st.c), _lib.ptr(st.stats),
                                 _lib.stream()), 'abn_gmm_mstep')
    return lse


def training_moments(table):
    """(shift [D] float32 device, gv [D] float64 host, good [T] bool device) of a training table: the mean of the
    frames without a non-finite value (float64, rounded to fp32), and the variance of xc over the good frames."""
    fin = torch.isfinite(table).all(dim=1)
    if not bool(fin.any()):
        raise ValueError('GmmPosteriorgram.fit: the table has no frame without a non-finite value')
    shift = table[fin].to(torch.float64).mean(dim=0).to(torch.float32)
    xc = table - shift
    good = torch.isfinite(xc * xc).all(dim=1)
    x64 = xc[good].to(torch.float64)
    gv = (x64 * x64).mean(dim=0) - x64.mean(dim=0) ** 2
    return shift, gv.cpu().numpy(), good


def initial_parameters(table, shift, gv, good, K, seed):
    """(w, m, v) float64 host arrays of the documented initialisation."""
    rows = torch.nonzero(good).flatten()
    Tg = int(rows.numel())
    if Tg < K:
        raise ValueError('GmmPosteriorgram.fit: %d good frames for K = %d components (T < K)' % (Tg, K))
    pick = np.sort(np.random.default_rng(seed).choice(Tg, K, replace=False))
    xc = (table[rows[torch.from_numpy(pick).to(rows.device)]] - shift).to(torch.float64).cpu().numpy()
    return np.full(K, 1.0 / K), xc, np.tile(np.asarray(gv, dtype=np.float64), (K, 1))


class GmmPosteriorgram(object):
    """fit / transform / score of the mixture the module docstring defines.

    corpus arguments: a DeviceCorpus, a {name: [T, D]} dict, a [T, D] float32 device table, or the path of an
    h5features file (needs the h5features package)."""

    def __init__(self, n_components, n_iter=20, tol=1e-4, var_floor=0.01, min_count=1.0, seed=0):
        if int(n_components) < 1:
            raise ValueError('GmmPosteriorgram: n_components = %r' % (n_components,))
        self.n_components, self.n_iter, self.tol = int(n_components), int(n_iter), float(tol)
        self.var_floor, self.min_count, self.seed = float(var_floor), float(min_count), int(seed)
        self.weights_ = self.means_ = self.variances_ = self.shift_ = self.gv_ = None
        self.log_likelihoods = []
        self.n_bad_ = self.n_starved_ = 0
        self._tables = None

    def whoami(self):
        return {'params': {k: getattr(self, k) for k in ('n_components', 'n_iter', 'tol', 'var_floor', 'min_count', 'seed')},
                'class_name': self.__class__.__name__}

    # -- inputs ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _corpus(corpus):
        """(device table, DeviceCorpus or None)"""
        from .dataloader import DeviceCorpus
        if isinstance(corpus, str):
            from .abx import _read_h5features
            corpus = DeviceCorpus(*_read_h5features(corpus))
        if isinstance(corpus, DeviceCorpus):
            return corpus.table, corpus
        if isinstance(corpus, dict):
            for k, f in corpus.items():
                if np.asarray(f).dtype != np.float32:
                    raise ValueError('GmmPosteriorgram: features of %r are %s, float32 is needed' % (k, np.asarray(f).dtype))
            return torch.from_numpy(np.concatenate([np.asarray(f) for f in corpus.values()], axis=0)).cuda(), None
        return corpus, None

    def _check_k(self):
        if self.n_components > max_k():
            raise ValueError('GmmPosteriorgram: K = %d, the kernels take 1 .. %d (abn_gmm_max_k)' % (self.n_components, max_k()))

    # -- fit ------------------------------------------------------------------------------------------------------
    def fit(self, corpus, n_ranges=0, init_means=None):
        """init_means: a [K, D] array of means to start from (KMeansQuantizer.centroids_, say) instead of the
        documented draw; the variances and weights start as documented."""
        self._check_k()
        table, _ = self._corpus(corpus)
        K = self.n_components
        table = _check_table('GmmPosteriorgram.fit', table, min_rows=K)
        shift, gv, good = training_moments(table)
        if not (gv > 0).all():
            raise ValueError('GmmPosteriorgram.fit: dimension %d of the table is constant' % int(np.argmin(gv > 0)))
        w, m, v = initial_parameters(table, shift, gv, good, K, self.seed)
        if init_means is not None:
            m = np.array(init_means, dtype=np.float64)
            if m.shape != (K, table.shape[1]) or not np.isfinite(m).all():
                raise ValueError('GmmPosteriorgram.fit: init_means must be a finite [%d, %d] array' % (K, table.shape[1]))
            m -= shift.cpu().numpy().astype(np.float64)
        st = EMState(w, m, v, gv, table.device)
        self.log_likelihoods = []
        for it in range(self.n_iter):
            em_iteration(table, shift, st, self.var_floor, self.min_count, n_ranges)
            ll_sum, bad, starved, tg = st.stats.cpu().tolist()          # the iteration's one read-back
            self.log_likelihoods.append(ll_sum / tg)
            self.n_bad_, self.n_starved_ = int(bad), int(starved)
            if it > 0 and self.log_likelihoods[-1] - self.log_likelihoods[-2] < self.tol:
                break
        self.shift_ = shift.cpu().numpy()
        self.gv_ = np.asarray(gv, dtype=np.float64)
        self.weights_ = st.w.cpu().numpy()
        self.means_ = st.mu.cpu().numpy() + self.shift_.astype(np.float64)
        self.variances_ = st.var.cpu().numpy()
        self._tables = None
        return self

    # -- use ------------------------------------------------------------------------------------------------------
    def device_tables(self, device):
        """(shift, A, B, c) on the device, rounded once from the float64 parameters."""
        if self.weights_ is None:
            raise ValueError('GmmPosteriorgram: fit or load first')
        if self._tables is None or self._tables[0].device != device:
            m = self.means_ - self.shift_.astype(np.float64)
            self._tables = tuple(torch.from_numpy(a).to(device) for a in
                                 (self.shift_,) + score_tables(self.weights_, m, self.variances_))
        return self._tables

    def _sweep(self, table, want_post):
        if self.weights_ is None:
            raise ValueError('GmmPosteriorgram: fit or load first')
        table = _check_table('GmmPosteriorgram', table)
        if table.shape[1] != self.shift_.shape[0]:
            raise ValueError('GmmPosteriorgram: the table has D = %d, the model D = %d' % (table.shape[1], self.shift_.shape[0]))
        shift, A, B, c = self.device_tables(table.device)
        T = table.shape[0]
        lse = torch.empty(T, dtype=torch.float32, device=table.device)
        out = torch.empty((T, self.n_components), dtype=torch.float32, device=table.device) if want_post else None
        for r0 in range(0, T, TRANSFORM_CHUNK):
            r1 = min(T, r0 + TRANSFORM_CHUNK)
            l, _ = posteriors(table[r0:r1], shift, A, B, c, want_post, out[r0:r1] if want_post else None)
            lse[r0:r1] = l
        return lse, out

    def transform(self, corpus):
        """The posterior table [rows, K] on the device; for a DeviceCorpus a new DeviceCorpus with the same names,
        lengths and times."""
        from .dataloader import DeviceCorpus
        table, dc = self._corpus(corpus)
        _, out = self._sweep(table, True)
        if dc is None:
            return out
        return DeviceCorpus.from_table(out, dc.names, [dc.length[k] for k in dc.names], dc.times)

    def score(self, corpus):
        """The mean frame log-likelihood over the good frames."""
        table, _ = self._corpus(corpus)
        lse, _ = self._sweep(table, False)
        ok = ~torch.isnan(lse)
        return float(lse[ok].to(torch.float64).sum().item() / max(1, int(ok.sum().item())))

    # -- files ----------------------------------------------------------------------------------------------------
    def save(self, path):
        if self.weights_ is None:
            raise ValueError('GmmPosteriorgram.save: fit first')
        with open(path, 'wb') as f:
            np.savez(f, weights=self.weights_, means=self.means_, variances=self.variances_, shift=self.shift_, gv=self.gv_,
                     log_likelihoods=np.asarray(self.log_likelihoods, dtype=np.float64),
                     n_components=self.n_components, n_iter=self.n_iter, tol=self.tol, var_floor=self.var_floor,
                     min_count=self.min_count, seed=self.seed)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            self = cls(int(z['n_components']), int(z['n_iter']), float(z['tol']), float(z['var_floor']), float(z['min_count']),
                       int(z['seed']))
            self.weights_, self.means_, self.variances_ = (z[k].astype(np.float64) for k in ('weights', 'means', 'variances'))
            self.shift_, self.gv_ = z['shift'].astype(np.float32), z['gv'].astype(np.float64)
            self.log_likelihoods = [float(v) for v in z['log_likelihoods']]
        if self.means_.shape != (self.n_components, self.shift_.shape[0]) or self.variances_.shape != self.means_.shape:
            raise ValueError('%s: not a GmmPosteriorgram file' % path)
        return self


def _read_features(path):
    """{name: [T, D] float32}, {name: [T] times} or None: an .npz of name -> array, or an h5features file."""
    if path.endswith('.npz'):
        with np.load(path) as z:
            return {k: z[k].astype(np.float32) for k in z.files}, None
    from .abx import _read_h5features
    feats, times = _read_h5features(path)
    return {k: np.asarray(v, dtype=np.float32) for k, v in feats.items()}, times


def _split_rows(table, names_and_lengths):
    """{name: its rows of the host array `table`} for (name, length) pairs laid end to end."""
    out, o = {}, 0
    for k, n in names_and_lengths:
        out[k] = table[o:o + int(n)]
        o += int(n)
    return out


def _write_named(path, out, times, as_column=False):
    """{name: array} as an .npz of name -> array or, for any other path, as an h5features file with the frame times
    {name: [T]} (as_column: [T] ids go in as a [T, 1] float32 column)."""
    if path.endswith('.npz'):
        np.savez(path, **{str(k): v for k, v in out.items()})
        return
    if times is None:
        raise ValueError('an h5features output needs the frame times: give an h5features input')
    import h5features
    names = list(out)
    items = [out[k].astype(np.float32)[:, None] if as_column else out[k] for k in names]
    with h5features.Writer(path) as wh:
        wh.write(h5features.Data(names, [np.asarray(times[k]) for k in names], items), 'features')


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m abnet3_amd.gmm', description='Gaussian posteriorgrams of a feature file')
    sub = ap.add_subparsers(dest='cmd', required=True)
    f = sub.add_parser('fit', help='fit a mixture on FEATURES and save it')
    f.add_argument('features', help='h5features file, or an .npz of name -> [T, D]')
    f.add_argument('model', help='the .npz to write')
    f.add_argument('-k', '--n-components', type=int, default=256)
    f.add_argument('--n-iter', type=int, default=20)
    f.add_argument('--tol', type=float, default=1e-4)
    f.add_argument('--var-floor', type=float, default=0.01)
    f.add_argument('--min-count', type=float, default=1.0)
    f.add_argument('--seed', type=int, default=0)
    t = sub.add_parser('transform', help='posteriorgrams of FEATURES under a saved mixture')
    t.add_argument('model')
    t.add_argument('features', help='h5features file, or an .npz of name -> [T, D]')
    t.add_argument('out', help='.npz of name -> [T, K], or an h5features file (when the input has times)')
    args = ap.parse_args(argv)
    feats, times = _read_features(args.features)
    if args.cmd == 'fit':
        g = GmmPosteriorgram(args.n_components, args.n_iter, args.tol, args.var_floor, args.min_count, args.seed).fit(feats)
        g.save(args.model)
        print('%d components, %d iterations, mean log-likelihood %.6f, %d BAD frames, %d starved components'
              % (g.n_components, len(g.log_likelihoods), g.log_likelihoods[-1], g.n_bad_, g.n_starved_))
        return 0
    g = GmmPosteriorgram.load(args.model)
    post = g.transform(feats).cpu().numpy()
    out = _split_rows(post, ((k, v.shape[0]) for k, v in feats.items()))
    _write_named(args.out, out, times)
    print('%d files, %d frames, K = %d -> %s' % (len(out), post.shape[0], post.shape[1], args.out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
