"""Same-different scoring without a GPU: the scores from a histogram against a brute-force walk of the sorted pool
(tests/samediff_np.py), the host tables of abnet3_amd/samediff.py, and the argument checks of abn_sd_collect /
abn_sd_count, which refuse before any launch."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import samediff_np  # noqa: E402

CONDITIONS = ('all', 'swdp', 'swsp')


def random_tokens(rng, n, n_types):
    """Type ranges of n tokens sorted by type and a speaker per token (two speakers)."""
    from abnet3_amd import samediff
    types = np.sort(rng.integers(0, n_types, n))
    order, cbeg, cend = samediff.sort_by_type(types.tolist())
    assert np.array_equal(order, np.arange(n))
    return cbeg, cend, rng.integers(0, 2, n).astype(np.int32)


def all_pairs(n):
    i, j = np.triu_indices(n, 1)
    return i, j


def pool_of(sims, i, j, cbeg, cend, spk, condition):
    """The pool as brute_ap takes it: (similarities, labels)."""
    xs, ys = [], []
    for x, a, b in zip(sims.tolist(), i.tolist(), j.tolist()):
        same = cbeg[a] <= b < cend[a]
        if same and condition != 'all' and (spk[a] == spk[b]) == (condition == 'swdp'):
            continue
        if math.isfinite(x):
            xs.append(x)
            ys.append(same)
    return xs, ys


def same_or_both_nan(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


CASES = [(2, 1), (2, 2), (3, 2), (5, 5), (7, 1), (12, 4), (30, 6), (45, 20), (64, 9), (64, 64)]


@pytest.mark.parametrize('condition', CONDITIONS)
@pytest.mark.parametrize('n,n_types', CASES)
@pytest.mark.parametrize('distance', [False, True])
def test_scores_from_histogram_equal_the_brute_force_walk(n, n_types, condition, distance):
    """Integer similarities in a narrow range: many ties, inside the positives, inside the negatives and across.
    Pools of 1 (n = 2) to 2016 (n = 64) pairs; one type holding every token (n_types = 1); singletons only
    (n_types = n draws repeats, (2, 2) and (5, 5) often none; P = 0 gives nan)."""
    from abnet3_amd import samediff
    rng = np.random.default_rng(n * 31 + n_types + 7 * CONDITIONS.index(condition))
    if n_types == n:
        cbeg, cend = np.arange(n, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32)         # all singletons
        spk = rng.integers(0, 2, n).astype(np.int32)
    else:
        cbeg, cend, spk = random_tokens(rng, n, n_types)
    i, j = all_pairs(n)
    same = j < cend[i]
    sims = (rng.integers(0, 6, len(i)) + np.where(same, 2, 0) * (1 - 2 * distance)).astype(np.float32)
    sims[rng.random(len(i)) < 0.02] = np.nan
    thr, hist, n_bad = samediff_np.buckets_hist(sims, i, j, cbeg, cend, spk, condition, distance)
    xs, ys = pool_of(sims, i, j, cbeg, cend, spk, condition)
    assert sum(hist) == len(xs) and len(thr) == sum(ys)
    ap, prb = samediff_np.brute_ap(xs, ys, distance)
    got = samediff.scores_from_histogram(thr, np.array(hist))
    assert same_or_both_nan(got.ap, ap) and same_or_both_nan(got.prb, prb), (got.ap, ap, got.prb, prb)
    ap2, prb2 = samediff_np.scores(thr, hist)
    assert same_or_both_nan(ap2, ap) and same_or_both_nan(prb2, prb)
    if n_types == n:
        assert len(thr) == 0 and math.isnan(got.ap) and math.isnan(got.prb)
    if len(thr):
        assert 0.0 < got.ap <= 1.0 and len(got.precision) == len(got.recall) == len(samediff_np.groups(thr))
        assert got.recall[-1] == 1.0


@pytest.mark.parametrize('P,N', [(1, 1), (3, 10), (10, 7), (49, 1000), (1000, 3)])
def test_perfect_separation_scores_one(P, N):
    """Every positive above every negative, the positives in tie groups of uneven sizes: AP = PRB = 1.0 exactly."""
    from abnet3_amd import samediff
    rng = np.random.default_rng(P)
    thr = np.sort(rng.integers(10, 10 + max(1, P // 3), P))[::-1].astype(np.float32)
    hist = np.zeros(P + 1, dtype=np.int64)
    for x in thr:
        hist[int((thr > x).sum())] += 1
    hist[P] += N
    s = samediff.scores_from_histogram(thr, hist)
    assert s.ap == 1.0 and s.prb == 1.0
    assert samediff_np.scores(thr, hist.tolist()) == (1.0, 1.0)


@pytest.mark.parametrize('P', [49, 98, 103, 187])
def test_perfect_separation_of_distinct_positives_scores_one(P):
    """P positives of P different similarities above every negative: P tie groups of weight 1 / P each.  A float64 sum of
    the groups' terms gives 1 - 2^-53 at these P (math.fsum([1 / P] * P) != 1); the score must still be 1.0 exactly."""
    from abnet3_amd import samediff
    assert math.fsum([1.0 / P] * P) != 1.0
    thr = np.arange(P, 0, -1).astype(np.float32)
    hist = np.ones(P + 1, dtype=np.int64)
    hist[P] = 12345
    s = samediff.scores_from_histogram(thr, hist)
    assert s.ap == 1.0 and s.prb == 1.0 and len(s.precision) == P and (s.precision == 1.0).all()
    assert samediff_np.scores(thr, hist.tolist()) == (1.0, 1.0)


@pytest.mark.parametrize('P,N', [(1, 1), (3, 10), (7, 10), (49, 1000), (1000, 3001), (123457, 10 ** 12 + 39)])
def test_all_similarities_equal_score_the_positive_share(P, N):
    """One tie group that holds the whole pool of N pairs: AP = PRB = P / N exactly."""
    from abnet3_amd import samediff
    N = max(N, P)
    thr = np.full(P, 0.25, dtype=np.float32)
    hist = np.zeros(P + 1, dtype=np.int64)
    hist[0] = N
    s = samediff.scores_from_histogram(thr, hist)
    assert s.ap == P / N and s.prb == P / N
    assert len(s.precision) == 1 and s.first[0] == 0 and s.last[0] == P


def test_a_histogram_of_another_threshold_list_is_refused():
    from abnet3_amd import samediff
    with pytest.raises(ValueError):
        samediff.scores_from_histogram(np.array([2.0, 1.0]), np.array([1, 0]))
    with pytest.raises(ValueError):
        samediff.scores_from_histogram(np.array([2.0, 1.0]), np.array([1, 0, 5]))      # two positives, one pair above


def test_sorting_by_type_and_the_positive_offsets():
    from abnet3_amd import samediff
    types = ['b', 'a', 'c', 'a', 'b', 'a', 'd']
    order, cbeg, cend = samediff.sort_by_type(types)
    assert [types[k] for k in order] == ['b', 'b', 'a', 'a', 'a', 'c', 'd']          # first appearance, stable
    assert order.tolist() == [0, 4, 1, 3, 5, 2, 6]
    assert cbeg.tolist() == [0, 0, 2, 2, 2, 5, 6] and cend.tolist() == [2, 2, 5, 5, 5, 6, 7]
    assert cbeg.dtype == np.int32 and cend.dtype == np.int32
    samediff.check_ranges(cbeg, cend)
    pos_off, total = samediff.positive_offsets(cbeg, cend)
    assert pos_off.tolist() == [0, 1, 1, 3, 4, 4, 4] and total == 4
    i, j = samediff.positive_index(cbeg, cend)
    assert list(zip(i.tolist(), j.tolist())) == [(0, 1), (2, 3), (2, 4), (3, 4)]
    for a, b in zip(i.tolist(), j.tolist()):
        assert pos_off[a] + (b - a - 1) == list(zip(i.tolist(), j.tolist())).index((a, b))
    for bad_beg, bad_end in (([0, 0, 2], [2, 3, 3]), ([0, 1, 1], [1, 3, 3][::-1]), ([1, 1], [2, 2]), ([0, 0], [3, 3])):
        with pytest.raises(ValueError):
            samediff.check_ranges(np.array(bad_beg), np.array(bad_end))


def test_pair_tables_of_the_dtw_route():
    from abnet3_amd import samediff
    for n in (1, 2, 5, 40):
        ref_i, ref_j = np.triu_indices(n, 1)
        for chunk in (1, 7, 1 << 20):
            runs = samediff.row_chunks(n, chunk)
            got = [samediff.upper_pairs(n, a, b) for a, b in runs]
            assert [a for a, _ in runs] == [0] + [b for _, b in runs][:-1] if runs else n < 2
            for (a, b), (gi, _) in zip(runs, got):
                assert len(gi) <= max(chunk, n - 1 - a) and b > a
            i = np.concatenate([g[0] for g in got]) if got else np.zeros(0, dtype=np.int64)
            j = np.concatenate([g[1] for g in got]) if got else np.zeros(0, dtype=np.int64)
            assert np.array_equal(i, ref_i) and np.array_equal(j, ref_j)


def test_speakers_from_a_dict_a_callable_and_a_file(tmp_path):
    from abnet3_amd import samediff
    files = ['s1_a', 's2_b', 's1_c', 's2_b']
    want = [0, 1, 0, 1]
    assert samediff.speaker_ids(files, {'s1_a': 'x', 's2_b': 'y', 's1_c': 'x'}).tolist() == want
    assert samediff.speaker_ids(files, lambda f: f.split('_')[0]).tolist() == want
    path = tmp_path / 'spk.txt'
    path.write_text('s1_a x\ns2_b y\ns1_c x\n')
    assert samediff.speaker_ids(files, str(path)).tolist() == want
    with pytest.raises(ValueError):
        samediff.speaker_ids(['nobody'], {'s1_a': 'x'})
    import torch
    i, j = torch.tensor([0, 0, 1]), torch.tensor([1, 2, 3])
    spk = torch.tensor(want)
    assert samediff.condition_mask(i, j, spk, 'swdp').tolist() == [True, False, False]
    assert samediff.condition_mask(i, j, spk, 'swsp').tolist() == [False, True, True]
    assert samediff.condition_mask(i, j, None, 'all').tolist() == [True, True, True]
    with pytest.raises(ValueError):
        samediff.condition_mask(i, j, None, 'swdp')


def test_command_line_arguments():
    from abnet3_amd import samediff
    a = samediff.parser().parse_args(['w.classes', 'f.h5f'])
    assert (a.classes, a.features, a.distance, a.frames, a.condition, a.spk) == ('w.classes', 'f.h5f', 'vectors', 10, 'all', None)
    a = samediff.parser().parse_args(['w.classes', 'f.h5f', '--distance', 'dtw-kl', '--frames', '5', '--condition', 'swdp',
                                      '--spk', 'spk.txt'])
    assert (a.distance, a.frames, a.condition, a.spk) == ('dtw-kl', 5, 'swdp', 'spk.txt')
    with pytest.raises(SystemExit):
        samediff.parser().parse_args(['w.classes', 'f.h5f', '--condition', 'across'])
    import abnet3_amd
    assert abnet3_amd.SameDifferentEvaluator is samediff.SameDifferentEvaluator
    assert abnet3_amd.scores_from_histogram is samediff.scores_from_histogram


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def test_arguments_are_refused_before_any_launch(lib):
    from abnet3_amd import _lib
    a = ctypes.c_void_p(0x10000)
    collect = lambda **k: lib.abn_sd_collect(k.get('X', a), k.get('n', 10), k.get('d', 8), a, k.get('cend', a), a, a, None)
    count = lambda **k: lib.abn_sd_count(k.get('X', a), k.get('n', 10), k.get('d', 8), a, a, k.get('spk', None),
                                         k.get('condition', 0), k.get('thr', a), k.get('n_thr', 3), k.get('hist', a), a, None)
    for call in (collect, count):
        name = b'abn_sd_collect' if call is collect else b'abn_sd_count'
        assert call(X=None) == _lib.E_ARG
        assert name in lib.abn_last_error() and b'null' in lib.abn_last_error()
        assert call(n=0) == _lib.E_ARG
        assert b'n = 0' in lib.abn_last_error()
        assert call(d=6) == _lib.E_UNSUPPORTED
        assert b'd = 6' in lib.abn_last_error() and b'4096' in lib.abn_last_error()
        assert call(d=4100) == _lib.E_UNSUPPORTED
        assert call(n=_lib.SD_MAX_N + 1) == _lib.E_UNSUPPORTED
        assert str(_lib.SD_MAX_N).encode() in lib.abn_last_error()
        assert call(X=ctypes.c_void_p(0x10004)) == _lib.E_ARG
        assert b'aligned' in lib.abn_last_error()
    assert collect(cend=None) == _lib.E_ARG
    assert count(hist=None) == _lib.E_ARG
    assert count(thr=None) == _lib.E_ARG
    assert count(n_thr=-1) == _lib.E_ARG
    assert count(n_thr=_lib.SD_MAX_THR + 1) == _lib.E_UNSUPPORTED
    assert str(_lib.SD_MAX_THR).encode() in lib.abn_last_error()
    assert count(condition=3) == _lib.E_ARG
    assert b'condition' in lib.abn_last_error()
    assert count(condition=_lib.SD_CONDITION['swdp']) == _lib.E_ARG
    assert b'spk' in lib.abn_last_error()


def test_grid_runs_follow_the_switch(lib, monkeypatch):
    """abn_sd_grid_runs: column tiles per workgroup from ABN_SD_TILES, or 8 .. 64 by the number of tiles."""
    from abnet3_amd import _lib
    monkeypatch.delenv('ABN_SD_TILES', raising=False)
    assert lib.abn_sd_grid_runs(0) == -1 and lib.abn_sd_grid_runs(_lib.SD_MAX_N + 1) == -1
    assert [lib.abn_sd_grid_runs(n) for n in (1, 300, 1024, 1025, 11000)] == [1, 1, 1, 2, 11]
    assert lib.abn_sd_grid_runs(60888) == 9                  # 476 tiles: 113 526 upper tiles / 2048 = 55 per run
    assert lib.abn_sd_grid_runs(1 << 20) == 128              # 8192 tiles: the cap of 64 per run
    monkeypatch.setenv('ABN_SD_TILES', '1')
    assert lib.abn_sd_grid_runs(300) == 3
    monkeypatch.setenv('ABN_SD_TILES', '2')
    assert lib.abn_sd_grid_runs(300) == 2
    monkeypatch.setenv('ABN_SD_TILES', '5000')              # out of range: the automatic rule
    assert lib.abn_sd_grid_runs(300) == 1
