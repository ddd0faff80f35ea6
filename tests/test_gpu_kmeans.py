"""abn_kmeans_assign / abn_kmeans_accumulate / abn_kmeans_update and KMeansQuantizer on the MI355X against
tests/kmeans_np.py.

The error bars.  An fp32 dot product of depth D + 1 in any order is within E[t] = gamma(D + 1) max_k (sum_d |xc m| + |b|)
of its float64 value, so a device id is ACCEPTABLE when its float64 score is within 2 E[t] of the row's best (the
winner and the runner-up may each be off by E), and EXACT where the float64 gap exceeds 2 E[t].  Counts are integers:
exact.  An fp32 sum of N terms in any order is within gamma(N) sum |terms| of float64: the bar of the per-cluster sums,
evaluated in float64 over the device's own ids.  New centroids and inertia: the project's 1e-5 relative bar, per tensor
against its largest magnitude (conftest.rel_err).  A centred centroid is a cancelled sum -- with K = 1 it is the mean of
the centred table, zero up to rounding -- whose fp32 error scales with the summands, not with the result, so the
magnitude it is judged against is floored at the mean |xc| of the good frames (as conftest.check_grads floors cancelled
gradients)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_np  # noqa: E402
from conftest import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

TS, KS, DS = (1, 127, 128, 129, 300, 1000), (1, 2, 127, 128, 129, 300), (1, 3, 31, 32, 33, 40, 100, 280)


def shape_cases():
    """24 of the 36 (T, K) pairs, D cycling through its values: every T, K and D occurs at least twice."""
    cases, n = [], 0
    for i, T in enumerate(TS):
        for j, K in enumerate(KS):
            if (i + j) % 3 != 2:
                cases.append((T, K, DS[n % len(DS)]))
                n += 1
    return cases


def dev(a, dt=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def make_case(T, K, D, seed, spread=3.0, offset=0.0, noise=1.0):
    """Frames around K centres and centroids near them: (x, label, shift, mu)."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(K, D)) * spread
    lab = rng.integers(0, K, size=T)
    x = (centres[lab] + noise * rng.normal(size=(T, D)) + offset).astype(np.float32)
    shift = (x.astype(np.float64).mean(axis=0) if T > 1 else np.full(D, offset)).astype(np.float32)
    mu = centres + offset - shift.astype(np.float64) + 0.1 * noise * rng.normal(size=(K, D))
    return x, lab, shift, mu


def run_kernels(x, shift, mu, n_ranges=0, metric='euclidean'):
    """One assign + accumulate + update on the device: dict of host arrays (ws: the partials, byte for byte)."""
    from abnet3_amd import kmeans
    table, dshift = dev(x), dev(shift)
    T, D = x.shape
    st = kmeans.LloydState(mu, T, table.device, metric)
    m0, b0 = host(st.m), host(st.b)
    _, best = kmeans.assign(table, dshift, st.m, st.b, ids=st.ids, want_best=True)
    st.ws = torch.zeros(kmeans._ws_bytes(T, st.K, D, n_ranges), dtype=torch.uint8, device=table.device)
    kmeans.accumulate(table, dshift, st, n_ranges)
    torch.cuda.synchronize()
    return dict(ids=host(st.ids), best=host(best), ws=host(st.ws), sums=host(st.sums), stats=host(st.stats), mu=host(st.mu),
                m=host(st.m), b=host(st.b), m0=m0, b0=b0)


def centre(x, shift):
    with np.errstate(all='ignore'):
        xc = (x - shift).astype(np.float32)
        return xc, ~np.isfinite(xc * xc).all(axis=1)


def check_iteration(x, shift, mu, out, metric='euclidean'):
    """Everything the shape grid asks of one iteration; returns the float64 reference pieces."""
    T, D = x.shape
    K = len(mu)
    xc, bad = centre(x, shift)
    m, b = kmeans_np.tables(mu, metric)
    assert np.array_equal(m, out['m0']) and np.array_equal(b, out['b0'])
    ref_ids, s, E = kmeans_np.assign(xc, bad, m, b)
    ids = out['ids']
    assert ids.dtype == np.int32 and np.array_equal(ids < 0, bad) and (ids[bad] == -1).all() and ids.max(initial=-1) < K
    good = ~bad
    rows = np.flatnonzero(good)
    short = s[rows].max(axis=1) - s[rows, ids[rows]]
    print('ids: %d of %d differ from the float64 argmax, largest shortfall / (2 E) = %.3g'
          % ((ids != ref_ids).sum(), T, (short / (2 * E[rows])).max(initial=0.0)))
    assert (short <= 2 * E[rows]).all(), (short / (2 * E[rows])).max()
    assert (np.abs(out['best'][rows] - s[rows, ids[rows]]) <= E[rows]).all() and np.isnan(out['best'][bad]).all()
    # statistics, float64 side over the DEVICE's ids
    N, S, d2 = kmeans_np.statistics(xc, ids, m, K)
    assert np.array_equal(out['sums'][:, D], N)
    err, bound = np.abs(out['sums'][:, :D] - S), kmeans_np.sum_bound(xc, ids, K)
    print('sums: largest error / bound = %.3g' % (err[bound > 0] / bound[bound > 0]).max(initial=0.0))
    assert (err <= bound).all()
    mu_ref, empty = kmeans_np.update(N, S, mu, metric)
    floor = np.abs(xc[good]).mean() if good.any() else 1e-30
    assert rel_err(out['mu'], mu_ref, floor=floor) < 1e-5, rel_err(out['mu'], mu_ref, floor=floor)
    assert np.array_equal(out['mu'][N == 0], np.asarray(mu, dtype=np.float64)[N == 0])          # kept, bit for bit
    m2, b2 = kmeans_np.tables(out['mu'], metric)
    assert np.array_equal(out['m'], m2) and np.allclose(out['b'], b2, rtol=1e-6, atol=0)
    tg = int(good.sum())
    assert list(out['stats'][1:]) == [T - tg, empty, tg]
    assert abs(out['stats'][0] - d2.sum()) <= 1e-5 * d2.sum(), (out['stats'][0], d2.sum())
    return dict(xc=xc, bad=bad, ref_ids=ref_ids, s=s, E=E, N=N, S=S)


@pytest.mark.parametrize('T,K,D', shape_cases())
def test_one_iteration_on_the_shape_grid(T, K, D):
    x, _, shift, mu = make_case(T, K, D, seed=T * 1000 + K + D)
    base = None
    for n_ranges in (0, 1, 3):
        out = run_kernels(x, shift, mu, n_ranges)
        check_iteration(x, shift, mu, out)
        if base is None:
            base = out
        assert np.array_equal(out['ids'], base['ids']) and np.array_equal(out['sums'][:, D], base['sums'][:, D])
        assert np.array_equal(out['best'], base['best'])


def test_ids_are_exact_on_separated_data():
    x, lab, shift, mu = make_case(1000, 129, 33, seed=11, spread=4.0, noise=0.5)
    xc, bad = centre(x, shift)
    m, b = kmeans_np.tables(mu)
    ref_ids, s, E = kmeans_np.assign(xc, bad, m, b)
    top2 = np.sort(s, axis=1)[:, -2:]
    assert not bad.any() and (top2[:, 1] - top2[:, 0] > 2 * E).all()                # the precondition, on the CPU
    assert np.array_equal(ref_ids, lab)
    out = run_kernels(x, shift, mu)
    assert np.array_equal(out['ids'], ref_ids)                                      # every row


def test_ties_go_to_the_lowest_index_within_a_tile_and_across_tiles():
    K, D, T = 260, 40, 1200
    x, lab, shift, mu = make_case(T, K, D, seed=12, spread=4.0, noise=0.5)
    mu[70] = mu[3]                       # the same 128-centroid tile
    mu[133] = mu[5]                      # the next tile
    lab[:200] = np.array([3, 70, 5, 133] * 50)
    rng = np.random.default_rng(13)
    x[:200] = ((mu + shift.astype(np.float64))[lab[:200]] + 0.5 * rng.normal(size=(200, D))).astype(np.float32)
    xc, bad = centre(x, shift)
    ref_ids, s, E = kmeans_np.assign(xc, bad, *kmeans_np.tables(mu))
    third = np.sort(s, axis=1)[:200, -3]
    assert (s[:200].max(axis=1) - third > 2 * E[:200]).all()                        # nothing else is near
    pair = np.array([3, 3, 5, 5] * 50)                   # (float64 sees each pair as equal up to its own rounding)
    assert ((ref_ids[:200] == pair) | (ref_ids[:200] == np.array([70, 70, 133, 133] * 50))).all()
    out = run_kernels(x, shift, mu)
    assert np.array_equal(out['ids'][:200], pair)                                   # the lower index of each pair, every row
    assert not np.isin(out['ids'], (70, 133)).any()
    assert out['sums'][70, D] == 0 and out['sums'][133, D] == 0 and out['stats'][2] >= 2


def test_bad_rows_are_counted_and_leave_the_statistics_alone():
    x, _, shift, mu = make_case(300, 5, 13, seed=14)
    mu[4] = 1e3                                                                       # far from everything: stays empty
    where = [0, 7, 130, 299]
    xb = np.insert(x, where, 0.0, axis=0)
    rows = np.array(where) + np.arange(4)
    xb[rows[0], 2] = np.nan
    xb[rows[1], 0] = np.inf
    xb[rows[2], 12] = -np.inf
    xb[rows[3], 5] = 3e38                                                             # finite; its centred square is not
    clean = run_kernels(x, shift, mu, n_ranges=1)
    dirty = run_kernels(xb, shift, mu, n_ranges=1)
    check_iteration(xb, shift, mu, dirty)
    assert list(np.flatnonzero(dirty['ids'] == -1)) == list(rows)
    assert np.array_equal(np.delete(dirty['ids'], rows), clean['ids'])
    assert list(dirty['stats']) == [clean['stats'][0], 4.0, 1.0, 300.0] and clean['stats'][1] == 0
    for k in ('sums', 'mu', 'm', 'b', 'ws'):                                          # bit for bit: one range, same frame order
        assert np.array_equal(dirty[k], clean[k]), k
    assert clean['sums'][4, 13] == 0 and np.array_equal(clean['mu'][4], np.full(13, 1e3)) and clean['stats'][2] == 1


@pytest.mark.parametrize('T,K,D', [(1000, 129, 40), (700, 300, 280)])
def test_two_calls_are_bit_identical_and_ranges_agree(T, K, D):
    x, _, shift, mu = make_case(T, K, D, seed=15)
    a, b = run_kernels(x, shift, mu, 3), run_kernels(x, shift, mu, 3)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    ref = check_iteration(x, shift, mu, a)
    for n_ranges in (0, 1, 2, 8):
        c = run_kernels(x, shift, mu, n_ranges)
        assert np.array_equal(c['ids'], a['ids']) and np.array_equal(c['sums'][:, D], a['sums'][:, D])
        assert (np.abs(c['sums'][:, :D] - ref['S']) <= kmeans_np.sum_bound(ref['xc'], a['ids'], K)).all()
        assert rel_err(c['mu'], a['mu']) < 1e-5 and abs(c['stats'][0] - a['stats'][0]) <= 1e-5 * a['stats'][0]


# ---- fit -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def planted():
    rng = np.random.default_rng(21)
    centres = rng.normal(size=(8, 20)) * 4.0 + 2.0
    lab = rng.integers(0, 8, size=2000)
    x = (centres[lab] + rng.normal(size=(2000, 20))).astype(np.float32)
    return x, lab, centres


def test_fit_recovers_planted_clusters_and_stops_when_no_id_changes(planted):
    from abnet3_amd.kmeans import KMeansQuantizer
    x, lab, centres = planted
    rng = np.random.default_rng(22)
    q = KMeansQuantizer(8, n_iter=20, tol=-1.0).fit(dev(x), init=centres + 0.3 * rng.normal(size=centres.shape))
    assert np.array_equal(host(q.predict(dev(x))), lab)
    assert 2 <= len(q.inertias) < 20 and q.n_changed[0] is None and q.n_changed[-1] == 0      # tol = -1 never stops it
    for before, now in zip(q.inertias, q.inertias[1:]):
        assert now <= before * (1 + 1e-5), q.inertias
    means = np.stack([x[lab == k].astype(np.float64).mean(axis=0) for k in range(8)])
    assert rel_err(q.centroids_, means) < 1e-5
    assert np.array_equal(q.counts_, np.bincount(lab, minlength=8)) and (q.n_bad_, q.n_empty_) == (0, 0)
    shift = q.shift_
    assert np.allclose(shift, kmeans_np.prepare(x)[2], rtol=2e-7, atol=0)
    xc, bad = centre(x, shift)
    m, _ = kmeans_np.tables(q.centroids_ - shift.astype(np.float64))
    d2 = kmeans_np.statistics(xc, lab.astype(np.int32), m, 8)[2]
    assert abs(q.score(dev(x)) - d2.mean()) <= 1e-5 * d2.mean()
    assert abs(q.inertias[-1] - d2.mean()) <= 1e-5 * d2.mean()


def test_fit_stops_on_tol_while_ids_still_change():
    from abnet3_amd.kmeans import KMeansQuantizer
    x = np.random.default_rng(23).normal(size=(3000, 10)).astype(np.float32)         # no structure: slow convergence
    full = KMeansQuantizer(16, n_iter=30, tol=-1.0, seed=1).fit(dev(x))
    for before, now in zip(full.inertias, full.inertias[1:]):
        assert now <= before * (1 + 1e-5), full.inertias
    tol = 1e-2
    stop = [i for i in range(1, len(full.inertias))
            if (full.inertias[i - 1] - full.inertias[i]) / full.inertias[i - 1] < tol]
    assert stop and full.n_changed[stop[0]] > 0, (full.inertias, full.n_changed)
    q = KMeansQuantizer(16, n_iter=30, tol=tol, seed=1).fit(dev(x))
    assert q.inertias == full.inertias[:stop[0] + 1] and q.n_changed[-1] > 0         # the same run, cut by tol alone
    assert len(KMeansQuantizer(16, n_iter=3, tol=-1.0, seed=1).fit(dev(x)).inertias) == 3


def test_fit_initialisation_and_refusals():
    from abnet3_amd.kmeans import KMeansQuantizer
    x = np.random.default_rng(24).normal(size=(50, 6)).astype(np.float32) + 3.0
    x[3, 1] = np.nan
    q = KMeansQuantizer(5, n_iter=0, seed=3).fit(dev(x))                              # no iteration: the initial centroids
    shift = q.shift_
    assert np.allclose(shift, kmeans_np.prepare(x)[2], rtol=2e-7, atol=0)
    xc, bad = centre(x, shift)
    good = np.flatnonzero(~bad)
    pick = np.sort(np.random.default_rng(3).choice(49, 5, replace=False))
    assert 3 not in good[pick]
    assert np.array_equal(q.centroids_, xc[good[pick]].astype(np.float64) + shift.astype(np.float64))
    assert q.inertias == []
    init = np.arange(30, dtype=np.float64).reshape(5, 6)
    assert np.allclose(KMeansQuantizer(5, n_iter=0).fit(dev(x), init=init).centroids_, init, rtol=0, atol=1e-6)
    with pytest.raises(ValueError, match='T < K'):
        KMeansQuantizer(60).fit(dev(x))
    with pytest.raises(ValueError, match='T < K'):
        KMeansQuantizer(50).fit(dev(x))                                               # 49 good frames
    with pytest.raises(ValueError, match='init'):
        KMeansQuantizer(5).fit(dev(x), init=np.zeros((4, 6)))


def test_cosine_metric_ignores_scale_and_keeps_unit_centroids():
    from abnet3_amd.kmeans import KMeansQuantizer
    rng = np.random.default_rng(25)
    centres = rng.normal(size=(5, 33))
    x = (centres[rng.integers(0, 5, 300)] + 0.3 * rng.normal(size=(300, 33))).astype(np.float32)
    scale = (2.0 ** rng.integers(-6, 7, size=(300, 1))).astype(np.float32)           # powers of two: x / |x| is bit-identical
    both = np.concatenate([x, x * scale, np.zeros((1, 33), dtype=np.float32)])
    q = KMeansQuantizer(5, n_iter=10, metric='cosine').fit(dev(both))
    ids = host(q.predict(dev(both)))
    assert np.array_equal(ids[:300], ids[300:600]) and ids[600] == -1 and q.n_bad_ == 1 and ids[:600].min() >= 0
    assert not q.shift_.any()
    assert np.abs(np.linalg.norm(q.centroids_[q.counts_ > 0], axis=1) - 1.0).max() < 1e-12
    assert np.abs(np.linalg.norm(q.centroids_, axis=1) - 1.0).max() < 1e-6
    # one iteration against the restatement, on the unit rows torch forms
    table = dev(both[:600])
    unit = host(table / table.norm(dim=1, keepdim=True))
    mu = unit[:5].astype(np.float64)
    out = run_kernels(unit, np.zeros(33, dtype=np.float32), mu, metric='cosine')
    check_iteration(unit, np.zeros(33, dtype=np.float32), mu, out, metric='cosine')
    assert not out['b'].any()


# ---- the public layer ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fitted_corpus():
    from abnet3_amd.dataloader import DeviceCorpus
    from abnet3_amd.kmeans import KMeansQuantizer
    from test_gpu_abx import synthetic_set
    items, feats, times = synthetic_set(np.random.default_rng(5), n_items=60, D=13, n_phones=4)
    corpus = DeviceCorpus(feats, times)
    return items, feats, times, corpus, KMeansQuantizer(8, n_iter=10).fit(corpus)


def test_predict_and_quantize_of_a_corpus_keep_names_lengths_and_times(fitted_corpus):
    from abnet3_amd.dataloader import DeviceCorpus
    from abnet3_amd.kmeans import bitrate, unit_sequences
    items, feats, times, corpus, q = fitted_corpus
    ids = q.predict(corpus)
    assert list(ids) == corpus.names
    flat = host(q.predict(corpus.table))
    for k in corpus.names:
        assert ids[k].dtype == np.int32 and ids[k].shape == (corpus.length[k],)
        assert np.array_equal(ids[k], flat[corpus.offset[k]:corpus.offset[k] + corpus.length[k]])
    assert flat.min() >= 0 and flat.max() < 8
    assert all(np.array_equal(a, b) for a, b in zip(q.predict(feats).values(), ids.values()))
    quant = q.quantize(corpus)
    assert isinstance(quant, DeviceCorpus) and quant.names == corpus.names and quant.dim == 13 and quant.total == corpus.total
    for k in corpus.names:
        assert quant.length[k] == corpus.length[k] and quant.offset[k] == corpus.offset[k]
        assert np.array_equal(quant.times[k], corpus.times[k])
    assert np.array_equal(host(quant.table), q.centroids_.astype(np.float32)[flat])
    assert torch.equal(q.quantize(corpus.table), quant.table)
    seconds = sum(float(t[-1] - t[0]) + 0.01 for t in times.values())
    print('bitrate of the units: %.1f bit/s' % bitrate(unit_sequences(ids), seconds))


def test_quantised_corpus_goes_through_abx(fitted_corpus):
    """A quantised corpus is made of identical frames, whose cosine can round above 1: under the reference's rule
    (parallel='drop', the default) the evaluator drops such pairs and raises; parallel='zero' reads them as distance 0."""
    from abnet3_amd.abx import ABXEvaluator, dtw_cost_batch
    items, feats, times, corpus, q = fitted_corpus
    quant = q.quantize(corpus)
    r = ABXEvaluator(items, quant, parallel='zero').run('within')
    print('ABX on quantised frames:', r)
    assert r.n_triplets > 0 and 0.0 <= r.error < 50.0             # the plumbing, not a quality claim
    with pytest.raises(ValueError, match='identical or parallel'):
        ABXEvaluator(items, quant).run('within')                  # the default is the rule it was
    # on the continuous corpus no cosine rounds above 1: the two rules give the same bits
    ev = ABXEvaluator(items, corpus)
    row, n = ev.row[ev.kept], ev.n[ev.kept]
    a, b = np.repeat(np.arange(len(row)), 3), np.tile(np.arange(3), len(row))
    args = (corpus.table, row[a], n[a], corpus.table, row[b], n[b])
    (c0, l0), (c1, l1) = dtw_cost_batch(*args), dtw_cost_batch(*args, parallel='zero')
    assert int((l0 > 0).sum()) > 0 and torch.equal(l0[l0 > 0], l1[l0 > 0]) and torch.equal(c0[l0 > 0], c1[l0 > 0])
    assert int((l1 <= 0).sum()) == 0                              # (a token against itself: dropped by 'drop' at most)
    # a quantised token against itself: the diagonal is all zeros or rounding-sized angles
    qa = (quant.table, row, n, quant.table, row, n)
    c, l = dtw_cost_batch(*qa, parallel='zero')
    assert int((l <= 0).sum()) == 0 and float((c / l.to(torch.float64)).max()) < 1e-3


def test_kmeans_centroids_initialise_the_mixture_and_the_default_path_is_unchanged():
    from abnet3_amd.gmm import GmmPosteriorgram
    from abnet3_amd.kmeans import KMeansQuantizer
    x, _, _, _ = make_case(600, 4, 5, seed=31)
    table = dev(x)
    first = GmmPosteriorgram(4, n_iter=3).fit(table)
    recorded = {k: getattr(first, k).copy() for k in ('weights_', 'means_', 'variances_', 'shift_')}
    ll = list(first.log_likelihoods)
    km = KMeansQuantizer(4, n_iter=10).fit(table)
    g = GmmPosteriorgram(4, n_iter=3).fit(table, init_means=km.centroids_)
    assert np.isfinite(g.log_likelihoods[0]) and len(g.log_likelihoods) >= 1
    again = GmmPosteriorgram(4, n_iter=3).fit(table)
    for k, v in recorded.items():
        assert np.array_equal(getattr(again, k), v), k
    assert again.log_likelihoods == ll
    with pytest.raises(ValueError, match='init_means'):
        GmmPosteriorgram(4).fit(table, init_means=np.zeros((3, 5)))
