"""abn_sd_collect / abn_sd_count / SameDifferentEvaluator on the MI355X against the restatement (tests/samediff_np.py).

The counting is pinned EXACTLY, without asking numpy to reproduce an MFMA accumulation chain: on small-integer rows
every dot product is exact in fp32 in any order, and on float rows the restatement is fed the similarities the kernel
itself returns (abn_sd_collect with every token declared one type), which are in turn held to the kNN tests' bound
against float64 and to abn_knn_topk's bits.

Shapes: n in {1, 2, 127, 128, 129, 257, 300} and d in {4, 36, 40, 400} reach every branch of a 128-tile with
BK = 32 (one tile, an edge tile, two and three tiles, a depth below one k-tile, a ragged last k-tile); the types hold
singletons, one type of 70 tokens (2415 positives: more than the 1024 splitters, so the search refines in global
memory), a type on rows 120 .. 135 (across the tile boundary), duplicated rows (ties) and two speakers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_np  # noqa: E402
import samediff_np  # noqa: E402

pytestmark = pytest.mark.gpu

CONDITIONS = ('all', 'swdp', 'swsp')


def type_ranges(rng, n):
    """cbeg, cend of n tokens: five singletons, a type of 70, one of 45, one on rows 120 .. 135, then small types."""
    sizes = [n] if n < 8 else [1, 1, 1, 1, 1, 70, 45, 16]
    while sum(sizes) < n:
        sizes.append(int(rng.integers(1, 10)))
    beg, cbeg, cend = 0, [], []
    for s in sizes:
        s = min(s, n - beg)
        cbeg += [beg] * s
        cend += [beg + s] * s
        beg += s
    return np.array(cbeg, dtype=np.int32), np.array(cend, dtype=np.int32)


def integer_rows(rng, n, d):
    X = rng.integers(-3, 4, (n, d)).astype(np.float32)
    X[1::3] = X[0:n - 1:3][:len(X[1::3])]                 # duplicated rows: exact ties
    return X


def unit_rows(rng, n, d):
    from test_gpu_knn import unit_rows as rows
    X = rows(rng, n, d)[0]
    X[1::5] = X[0:n - 1:5][:len(X[1::5])]
    return X


def gpu_collect(X, cbeg, cend):
    from abnet3_amd import samediff
    pos_sim, pos_off = samediff.collect(torch.from_numpy(X).cuda(), cbeg, cend)
    i, j = samediff.positive_index(cbeg, cend)
    torch.cuda.synchronize()
    return pos_sim.cpu().numpy(), i.numpy(), j.numpy()


def gpu_all_pairs(X):
    """Every similarity the kernel forms: collect with all tokens declared one type -> a dense [n, n] upper triangle."""
    n = len(X)
    sims, i, j = gpu_collect(X, np.zeros(n, dtype=np.int32), np.full(n, n, dtype=np.int32))
    assert len(sims) == n * (n - 1) // 2
    return sims, i, j


def gpu_count(X, cbeg, cend, sims_pos, pi, pj, spk, condition):
    """(thr, hist, n_bad, scores) the way the evaluator goes: mask the collected list, sort it, count."""
    from abnet3_amd import samediff
    keep = samediff.condition_mask(torch.from_numpy(pi), torch.from_numpy(pj), torch.from_numpy(spk), condition).numpy()
    v = torch.from_numpy(sims_pos[keep]).cuda()
    thr = torch.sort(v[torch.isfinite(v)], descending=True)[0]
    hist, n_bad = samediff.pair_histogram(torch.from_numpy(X).cuda(), cbeg, cend, thr, spk, condition)
    thr, hist = thr.cpu().numpy(), hist.cpu().numpy()
    return thr, hist, n_bad, samediff.scores_from_histogram(thr, hist)


def close_or_both_nan(a, b, tol=1e-12):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol


def check_against_restatement(X, cbeg, cend, spk, sims, i, j, conditions=CONDITIONS):
    """hist, n_bad, AP and PRB of the kernel route equal the restatement's over the pair similarities `sims`."""
    same = j < cend[i]
    got_pos, pi, pj = gpu_collect(X, cbeg, cend)
    assert np.array_equal(pi, i[same]) and np.array_equal(pj, j[same])
    assert np.array_equal(got_pos.view(np.int32), sims[same].view(np.int32))
    out = {}
    for condition in conditions:
        thr, hist, n_bad, s = gpu_count(X, cbeg, cend, got_pos, pi, pj, spk, condition)
        ref_thr, ref_hist, ref_bad = samediff_np.buckets_hist(sims, i, j, cbeg, cend, spk, condition)
        assert np.array_equal(thr, ref_thr)
        assert np.array_equal(hist, np.array(ref_hist, dtype=np.int64)), np.flatnonzero(hist != np.array(ref_hist))[:10]
        assert n_bad == ref_bad
        ap, prb = samediff_np.scores(ref_thr, ref_hist)
        print('n = %d, d = %d, %s: P = %d, pool %d, bad %d, AP %.6f (restated %.6f), PRB %.6f (%.6f)'
              % (X.shape[0], X.shape[1], condition, len(thr), hist.sum(), n_bad, s.ap, ap, s.prb, prb))
        assert close_or_both_nan(s.ap, ap) and close_or_both_nan(s.prb, prb)
        out[condition] = (thr, hist, n_bad)
    return out


@pytest.mark.parametrize('n,d', [(1, 4), (2, 36), (127, 40), (128, 4), (129, 36), (257, 40), (300, 36), (300, 4)])
def test_exact_arithmetic_inputs(n, d):
    """Integer entries in -3 .. 3, d <= 64: collect EQUALS the integer dot products, hist and n_bad the restatement's."""
    rng = np.random.default_rng(1000 * n + d)
    X = integer_rows(rng, n, d)
    cbeg, cend = type_ranges(rng, n)
    spk = rng.integers(0, 2, n).astype(np.int32)
    i, j = np.triu_indices(n, 1)
    S = (X.astype(np.float64) @ X.astype(np.float64).T).astype(np.float32)
    sims, ai, aj = gpu_all_pairs(X)
    assert np.array_equal(ai, i) and np.array_equal(aj, j)
    assert np.array_equal(sims, S[i, j])
    out = check_against_restatement(X, cbeg, cend, spk, S[i, j], i, j)
    assert all(bad == 0 for _, _, bad in out.values())
    if n >= 75:
        assert len(out['all'][0]) > 2415                     # the two-level search refined in global memory


@pytest.mark.parametrize('n,d', [(2, 4), (33, 400), (32, 36), (129, 40), (257, 36), (300, 400)])
def test_float_rows(n, d):
    """Unit rows: the kernel's similarities lie within knn_np.delta(d) of float64, EQUAL abn_knn_topk's bit for bit
    (n <= 33, k = 32, no exclusion: the lists hold every neighbour but at most one), and the histogram EQUALS the
    restatement fed with those kernel-made similarities."""
    rng = np.random.default_rng(77 * n + d)
    X = unit_rows(rng, n, d)
    cbeg, cend = type_ranges(rng, n)
    spk = rng.integers(0, 2, n).astype(np.int32)
    sims, i, j = gpu_all_pairs(X)
    S = X.astype(np.float64) @ X.astype(np.float64).T
    err = np.abs(sims.astype(np.float64) - S[i, j]).max()
    print('n = %d, d = %d: max |sim - float64| = %.3e, bound %.3e' % (n, d, err, knn_np.delta(d)))
    assert err <= knn_np.delta(d)
    if n <= 33:
        from test_gpu_knn import gpu_topk
        idx, ksim = gpu_topk(X, X, 32)
        found = 0
        for a, b, v in zip(i.tolist(), j.tolist(), sims):
            for q, c in ((a, b), (b, a)):
                at = np.flatnonzero(idx[q] == c)
                if len(at):
                    found += 1
                    assert ksim[q, at[0]].view(np.int32) == v.view(np.int32), (q, c, ksim[q, at[0]], v)
        assert found >= 2 * len(sims) - n
    check_against_restatement(X, cbeg, cend, spk, sims, i, j)


def test_the_grid_does_not_change_a_count(monkeypatch):
    """ABN_SD_TILES (column tiles per workgroup): 1, 2 and the default give the same similarities and counts.  n = 300 is
    three column tiles, so the three settings launch 3, 2 and 1 runs per row block (abn_sd_grid_runs, which shares the
    launch's rule): three different grids really ran."""
    from abnet3_amd import _lib
    rng = np.random.default_rng(5)
    X = unit_rows(rng, 300, 36)
    cbeg, cend = type_ranges(rng, 300)
    spk = rng.integers(0, 2, 300).astype(np.int32)
    outs, runs = {}, {}
    for tiles in ('1', '2', None):
        if tiles is None:
            monkeypatch.delenv('ABN_SD_TILES', raising=False)
        else:
            monkeypatch.setenv('ABN_SD_TILES', tiles)
        runs[tiles] = _lib.load().abn_sd_grid_runs(300)
        sims, pi, pj = gpu_collect(X, cbeg, cend)
        thr, hist, n_bad, _ = gpu_count(X, cbeg, cend, sims, pi, pj, spk, 'swdp')
        outs[tiles] = (sims, thr, hist, n_bad)
    for tiles in ('1', '2'):
        for a, b in zip(outs[tiles], outs[None]):
            assert np.array_equal(a, b), tiles
    assert outs[None][2].sum() > 0
    assert runs == {'1': 3, '2': 2, None: 1}


def test_non_finite_rows_are_counted_apart():
    """A row of NaN and a row of inf: their pairs land in n_bad and nowhere else."""
    rng = np.random.default_rng(9)
    n = 129
    X = unit_rows(rng, n, 40)
    X[3] = np.nan
    X[128] = np.inf
    cbeg, cend = type_ranges(rng, n)
    spk = rng.integers(0, 2, n).astype(np.int32)
    sims, i, j = gpu_all_pairs(X)
    touched = (i == 3) | (j == 3) | (i == 128) | (j == 128)
    assert not np.isfinite(sims[touched]).any() and np.isfinite(sims[~touched]).all()
    out = check_against_restatement(X, cbeg, cend, spk, sims, i, j, ('all', 'swdp'))
    thr, hist, n_bad = out['all']
    assert n_bad == touched.sum() == 2 * (n - 1) - 1
    assert hist.sum() == n * (n - 1) // 2 - n_bad
    clean = samediff_np.buckets_hist(sims[~touched], i[~touched], j[~touched], cbeg, cend, spk, 'all')
    assert np.array_equal(thr, clean[0]) and np.array_equal(hist, np.array(clean[1], dtype=np.int64))


def dtw_tokens(rng, n_tokens=40, D=20):
    length = rng.integers(3, 31, n_tokens).astype(np.int32)
    row0 = (np.cumsum(length) - length).astype(np.int64)
    table = rng.standard_normal((int(length.sum()), D)).astype(np.float32)
    return table, row0, length


@pytest.mark.parametrize('condition', CONDITIONS)
def test_dtw_route_equals_the_restatement(condition):
    """40 tokens of 3 .. 30 frames, D = 20: the distances (bit-exact by the DTW kernels' contract) and the histogram
    equal the restatement built on the C oracle's DTW; a token with a NaN frame is counted in n_bad."""
    import abx_np
    from abnet3_amd import samediff
    rng = np.random.default_rng(21)
    table, row0, length = dtw_tokens(rng)
    n = len(length)
    nan_tok = 17
    table[row0[nan_tok] + 1, 5] = np.nan
    cbeg, cend = type_ranges(rng, n)
    spk = rng.integers(0, 2, n).astype(np.int32)
    i, j = np.triu_indices(n, 1)
    tok = lambda k: table[row0[k]:row0[k] + length[k]]
    ref = np.array([np.nan if nan_tok in (a, b) else abx_np.dtw_distance(tok(a), tok(b)) for a, b in zip(i.tolist(), j.tolist())])
    d_table = torch.from_numpy(table).cuda()
    dist, ok = samediff.dtw_distances(d_table, row0, length, i, j)
    dist, ok = dist.cpu().numpy(), ok.cpu().numpy()
    assert np.array_equal(ok, np.isfinite(ref)) and (~ok).sum() == n - 1
    assert np.array_equal(dist[ok].view(np.int64), ref[ok].view(np.int64))
    thr, hist, n_bad = samediff.dtw_histogram(d_table, row0, length, cbeg, cend, spk, condition, chunk=100)
    ref_thr, ref_hist, ref_bad = samediff_np.buckets_hist(ref, i, j, cbeg, cend, spk, condition, distance=True)
    assert np.array_equal(thr, ref_thr) and thr.dtype == np.float64
    assert np.array_equal(hist, np.array(ref_hist, dtype=np.int64))
    assert n_bad == ref_bad and n_bad > 0
    s = samediff.scores_from_histogram(thr, hist)
    ap, prb = samediff_np.scores(ref_thr, ref_hist)
    assert close_or_both_nan(s.ap, ap) and close_or_both_nan(s.prb, prb)


def planted_words(rng, n_words=6, per_word=8, D=20):
    """Four files (two per speaker) of noise with noisy, linearly time-warped copies of `n_words` templates.
    Returns (features, times, clusters of (file, onset, offset), {file: speaker}); the LAST token's frames are zero."""
    templates = [np.cumsum(rng.standard_normal((50, D)), axis=0) for _ in range(n_words)]
    templates = [3.0 * (t - t.mean(0)) / t.std() for t in templates]
    names = ['spkA_1', 'spkB_1', 'spkA_2', 'spkB_2']
    chunks = {f: [rng.standard_normal((10, D))] for f in names}
    spots = {f: [] for f in names}
    clusters = [[] for _ in range(n_words)]
    for w in range(n_words):
        for c in range(per_word):
            f = names[c % 4]
            ln = int(rng.integers(42, 62))
            src = np.linspace(0, 49, ln)
            lo = np.minimum(np.floor(src).astype(int), 48)
            fr = (src - lo)[:, None]
            x = templates[w][lo] * (1 - fr) + templates[w][lo + 1] * fr + 0.3 * rng.standard_normal((ln, D))
            if w == n_words - 1 and c == per_word - 1:
                x[:] = 0.0
            b = sum(len(a) for a in chunks[f])
            chunks[f] += [x, rng.standard_normal((int(rng.integers(5, 15)), D))]
            spots[f].append((w, b, b + ln))
    feats = {f: np.concatenate(chunks[f]).astype(np.float32) for f in names}
    times = {f: np.arange(len(feats[f])) * 0.01 for f in names}
    for f in names:
        for w, b, e in spots[f]:
            clusters[w].append((f, float(times[f][b]), float(times[f][e - 1])))
    return feats, times, clusters, {f: f[:4] for f in names}


def test_evaluator_end_to_end_on_planted_words(tmp_path):
    from abnet3_amd import samediff
    from abnet3_amd.discovery import segment_vectors
    rng = np.random.default_rng(3)
    feats, times, clusters, speakers = planted_words(rng)
    spk_file = tmp_path / 'spk.txt'
    spk_file.write_text(''.join('%s %s\n' % kv for kv in sorted(speakers.items())))
    ev = samediff.SameDifferentEvaluator(clusters, feats, times, speakers=str(spk_file))
    n_all = sum(len(c) for c in clusters)
    assert len(ev.tokens) == n_all == 48 and (ev.length > 40).all()
    # the table-level route on the same tokens (already in type order: clusters are listed type after type)
    keep = np.ones(n_all, dtype=bool)
    keep[-1] = False
    _, cbeg, cend = samediff.sort_by_type(ev.types[keep].tolist())
    vec, nonzero = segment_vectors(ev.corpus.table, ev.row0, ev.length, 10)
    assert nonzero.cpu().numpy().tolist() == keep.tolist()
    X = vec[:-1].contiguous()
    spk = ev.spk[keep]
    pos_sim, _ = samediff.collect(X, cbeg, cend)
    pi, pj = samediff.positive_index(cbeg, cend)
    _, call_beg, call_end = samediff.sort_by_type(ev.types.tolist())
    for condition in CONDITIONS:
        r = ev.evaluate('vectors', frames=10, condition=condition)
        thr, hist, n_bad, s = gpu_count(X.cpu().numpy(), cbeg, cend, pos_sim.cpu().numpy(), pi.numpy(), pj.numpy(), spk, condition)
        assert (r.ap, r.prb) == (s.ap, s.prb) and r.n_bad == n_bad == 0
        assert (r.n_tokens, r.n_types, r.n_dropped_tokens) == (47, 6, 1)
        assert r.n_positives == len(thr) and r.n_pairs == hist.sum()
        if condition == 'all':
            assert r.n_pairs == 47 * 46 // 2 and r.n_positives == 5 * 28 + 21
        print(r)
        assert r.ap > 0.8
        r = ev.evaluate('dtw', condition=condition)
        thr, hist, n_bad = samediff.dtw_histogram(ev.corpus.table, ev.row0, ev.length, call_beg, call_end, ev.spk, condition)
        s = samediff.scores_from_histogram(thr, hist)
        assert (r.ap, r.prb) == (s.ap, s.prb) and r.n_bad == n_bad
        assert (r.n_tokens, r.n_types, r.n_dropped_tokens, r.n_positives) == (48, 6, 0, len(thr))
        print(r)
        assert r.ap > 0.8
    with pytest.raises(ValueError, match='4096'):
        ev.evaluate('vectors', frames=205)
    with pytest.raises(ValueError, match='speakers'):
        samediff.SameDifferentEvaluator(clusters, feats, times).evaluate(condition='swdp')
