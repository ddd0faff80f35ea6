"""Query-by-example search without a GPU: the numpy restatement (tests/qbe_np.py) against full DTW over every
window, its rules for NaN and BAD cells, the ranking helpers, the fairness of the end-to-end fixture, and that the
header, the binding and the library carry the new symbols."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abx_kl_np  # noqa: E402
import qbe_np  # noqa: E402


def rounding_frame(rng, D=7):
    """An integer-valued frame whose cosine with itself rounds above 1 (a NaN distance in the reference's cell)."""
    from oracle import dtw_oracle as O
    for _ in range(1000):
        v = rng.integers(-3, 4, (1, D)).astype(np.float32)
        if np.isnan(O.cosine_distance(v, v, check=False)[0][0, 0]):
            return v[0]
    raise AssertionError('no such frame found')


def sign_frames(rng, n, D=16):
    """Frames of +-1 in 16 dimensions: the norm is exactly 4, every cosine k / 16 is exact, identical frames are at
    distance exactly 0 with no rounding involved."""
    return rng.choice(np.float32([-1.0, 1.0]), (n, D))


def test_every_end_equals_the_best_full_dtw_over_its_windows():
    """C(e, M-1) = min over s of the full-DTW cost of the window [s, e], exactly (rounding is monotone, so the minimum
    over paths commutes with it); the reported start is a window that attains it, the length is that window's."""
    rng = np.random.default_rng(0)
    for trial in range(12):
        n, m = int(rng.integers(1, 25)), int(rng.integers(1, 13))
        if trial % 2:
            d = rng.integers(0, 4, (n, m)).astype(np.float32) / np.float32(3)       # many exact ties
        else:
            d = rng.random((n, m)).astype(np.float32)
        C, L, S = qbe_np.last_column(d.astype(np.float64))
        for e in range(n):
            full = [abx_kl_np.dtw(d[s:e + 1]) for s in range(e + 1)]
            assert C[e] == min(c for c, _ in full), (trial, e)
            assert 0 <= S[e] <= e
            assert full[S[e]] == (C[e], L[e]), (trial, e)
            assert max(m, e - S[e] + 1) <= L[e] <= m + e - S[e]


def test_a_query_cut_from_the_utterance_finds_itself():
    rng = np.random.default_rng(1)
    for trial in range(6):
        utt = sign_frames(rng, 50)
        utt[30] = 0.0                                               # an all-zero frame elsewhere: distance 1, harmless
        s, m = int(rng.integers(0, 20)), int(rng.integers(1, 10))
        c, ln, start, end, _ = qbe_np.search(qbe_np.cosine_cells(utt, utt[s:s + m]))
        assert (c, ln, start, end) == (0.0, m, s, s + m - 1), trial
    # ... also when its frames' cosines with themselves round above 1 (ABX drops such a pair: the search must not)
    # (the utterance: integer frames at distance exactly 0 from themselves, by value or by the rule)
    from oracle import dtw_oracle as O
    pool = rng.integers(-3, 4, (400, 7)).astype(np.float32)
    self_d = np.array([O.cosine_distance(f[None], f[None], check=False)[0][0, 0] for f in pool])
    keep = np.flatnonzero(np.isnan(self_d) | (self_d == 0))[:40]
    assert len(keep) == 40 and np.isnan(self_d[keep[10:15]]).any() and np.isnan(self_d[keep]).sum() >= 5
    utt = pool[keep]
    c, ln, start, end, _ = qbe_np.search(qbe_np.cosine_cells(utt, utt[10:15]))
    assert (c, ln, start, end) == (0.0, 5, 10, 14)


def test_nan_rule_case_by_case():
    nan, inf = np.nan, np.inf
    one = np.float32(1)
    d = np.array([[nan, nan, nan, nan, nan, nan, 0.25]])
    dot = np.float32([[2.0, -2.0, nan, inf, 1.0, 1.0, 1.0]])
    ny = np.float32([1.0, 1.0, 1.0, 1.0, 0.0, inf, 1.0])
    got = qbe_np.nan_rule(d, dot, np.float32([one]), ny)
    assert got.tolist() == [[0.0, 1.0, inf, inf, inf, inf, 0.25]]
    # a product of the norms that underflows to zero: blocked
    assert qbe_np.nan_rule(np.array([[nan]]), np.float32([[0.0]]), np.float32([1e-30]), np.float32([1e-30]))[0, 0] == inf
    # the cells themselves
    rng = np.random.default_rng(2)
    v = rounding_frame(rng)
    w = rng.standard_normal(7).astype(np.float32)
    bad = v.copy()
    bad[3] = nan
    big = v.copy()
    big[0] = inf
    tiny = (v * np.float32(1e-30)).astype(np.float32)
    U = np.stack([v, -v, bad, big, np.zeros(7, np.float32), w, tiny])
    d = qbe_np.cosine_cells(U, np.stack([v, w, np.zeros(7, np.float32), tiny]))
    assert d[0, 0] == 0.0 and d[1, 0] == 1.0                    # |cos| rounded above 1
    assert np.isinf(d[2:4, :2]).all()                           # a non-finite frame blocks its cells ...
    assert (d[:, 2:] == [[1, 1], [1, 1], [1, 1], [1, 1], [0, 0], [1, 1], [0, 0]]).all()     # ... but for the reference's zero-frame
    assert d[4].tolist()[:2] == [1.0, 1.0]                      # rules, which come first (`tiny` squares to zero: a zero frame)
    assert 0.0 < d[5, 0] < 1.0 and d[5, 1] < 1e-3
    assert not np.isnan(d).any()


def test_a_nan_query_frame_gives_no_detection_and_a_nan_utterance_frame_is_routed_around():
    rng = np.random.default_rng(3)
    utt = sign_frames(rng, 40)
    q = utt[12:18].copy()
    qn = q.copy()
    qn[2, 5] = np.nan
    assert qbe_np.search(qbe_np.cosine_cells(utt, qn))[:4] == (0.0, 0, -1, -1)
    far = utt.copy()
    far[30] = np.nan                                            # away from the match: nothing changes
    assert qbe_np.search(qbe_np.cosine_cells(far, q))[:4] == (0.0, 6, 12, 17)
    mid = utt.copy()
    mid[14] = np.nan                                            # inside it: no path may use row 14, one starts after it
    c, ln, start, end, (C, L, S) = qbe_np.search(qbe_np.cosine_cells(mid, q))
    assert ln >= 6 and c > 0 and np.isfinite(c) and not (start <= 14 <= end)
    assert np.isinf(C[14]) and L[14] == 0 and S[14] == -1
    assert (S[15:] >= 15).all()
    # KL: a BAD row blocks, the pair is kept
    post = rng.dirichlet(np.ones(8), 30).astype(np.float32)
    post[20, 1] = -0.5
    t = abx_kl_np.tables(post)
    sl = lambda a, b: [x[a:b] for x in t]
    assert qbe_np.search(qbe_np.kl_cells(t, sl(5, 9)))[:4] == (0.0, 4, 5, 8)
    assert qbe_np.search(qbe_np.kl_cells(t, sl(18, 22)))[:4] == (0.0, 0, -1, -1)


def test_empty_and_refused_pairs():
    f = np.random.default_rng(4).standard_normal((30, 5)).astype(np.float32)
    cost, plen, start, end, (pc, pl, ps), off = qbe_np.search_cosine_batch(
        f, [0, 0, 0, 28, -1, 0, 0], [3, 0, 3, 3, 3, -2, 5], f, [0, 0, 5, 0, 0, 0, 25], [10, 10, 0, 10, 10, 10, 6], cap=4)
    assert plen.tolist() == [plen[0], 0, 0, -1, -1, -1, -1] and plen[0] >= 3
    assert start.tolist()[1:] == [-1] * 6 and end.tolist()[1:] == [-1] * 6 and (cost[1:] == 0).all()
    assert off.tolist() == [0, 10, 20, 20, 30, 40, 50]
    assert np.isinf(pc[10:20]).all() and (pl[10:20] == 0).all() and (ps[10:20] == -1).all()      # an empty query
    assert np.isnan(pc[20:]).all() and (pl[20:] == -7).all()                                      # refused: untouched


def test_ranking_helpers():
    from abnet3_amd.qbe import mean_average_precision, precision_at_n
    inf = np.inf
    score = np.array([[0.1, 0.5, 0.2, inf],        # relevant at ranks 1 and 3: AP = (1/1 + 2/3) / 2
                      [0.9, 0.1, 0.2, 0.3],        # relevant at rank 4: AP = 1/4
                      [0.3, 0.3, 0.3, 0.3],        # all tied: column order; relevant at ranks 2, 3
                      [0.1, 0.2, 0.3, 0.4]])       # nothing relevant: not counted
    rel = np.array([[1, 1, 0, 0], [1, 0, 0, 0], [0, 1, 1, 0], [0, 0, 0, 0]], dtype=bool)
    ap = [(1 + 2 / 3) / 2, 1 / 4, (1 / 2 + 2 / 3) / 2]
    assert mean_average_precision(score, rel) == pytest.approx(np.mean(ap), abs=1e-15)
    assert precision_at_n(score, rel) == pytest.approx(np.mean([1 / 2, 0.0, 1 / 2]), abs=1e-15)
    assert mean_average_precision(score[:2, :2], np.eye(2, dtype=bool)[::-1]) == 0.5
    assert np.isnan(mean_average_precision(score, np.zeros_like(rel))) and np.isnan(precision_at_n(score, np.zeros_like(rel)))
    with pytest.raises(ValueError):
        mean_average_precision(score, rel[:2])


def test_the_end_to_end_fixture_is_fair():
    """The restatement finds every planted word: MAP and P@N are 1, each query finds itself at cost 0 and every other
    occurrence within two frames of where it was planted."""
    from abnet3_amd.qbe import mean_average_precision, precision_at_n
    feats, times, queries, relevant, planted = qbe_np.planted_corpus()
    assert len(feats) == 6 and relevant.sum(axis=1).min() >= 2 and not relevant.all()
    score, start, end = qbe_np.search_corpus(feats, times, queries)
    assert mean_average_precision(score, relevant) == 1.0 and precision_at_n(score, relevant) == 1.0
    for (w, u), (lo, hi) in planted.items():
        assert abs(start[w, u] - lo) <= 2 and abs(end[w, u] - hi) <= 2, (w, u)
        if u == w:
            assert (start[w, u], end[w, u]) == (lo, hi) and score[w, u] < 1e-3


def test_header_binding_and_library_carry_the_new_symbols():
    from abnet3_amd import _lib, build
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read(), flags=re.S)
    raw = ctypes.CDLL(build.build())
    for name in ('abn_dtw_search_max_query', 'abn_dtw_search_batched', 'abn_dtw_search_kl_batched'):
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.SYMBOLS, name
        assert hasattr(raw, name), name
    assert len(_lib.SYMBOLS['abn_dtw_search_batched'][1]) == 20 and len(_lib.SYMBOLS['abn_dtw_search_kl_batched'][1]) == 24
    assert re.search(r'^#define ABN_ABI_VERSION 20$', text, flags=re.M)
    assert _lib.ABI_VERSION == 20
    raw.abn_dtw_search_max_query.restype = ctypes.c_int64
    assert raw.abn_dtw_search_max_query() == qbe_np.CAP >= 256
    assert re.search(r'^#define ABN_DTW_SEARCH_MAX_QUERY %d$' % qbe_np.CAP, text, flags=re.M)
    # argument validation happens before any launch
    lib = _lib.load()
    assert lib.abn_dtw_search_batched(None, 1, None, 1, None, None, None, None, 1, 4, None, None, None, None, None, 0, None,
                                      None, None, None) == _lib.E_ARG
    assert b'null' in lib.abn_last_error()


def test_argument_errors_without_a_device(capsys):
    from abnet3_amd import qbe
    with pytest.raises(ValueError, match='distance'):
        qbe.subsequence_dtw_batch(None, [], [], None, [], [], distance='nonsense')
    with pytest.raises(ValueError, match='distance'):
        qbe.QbeSearcher({}, {}, distance='nonsense')
    with pytest.raises(SystemExit):
        qbe.main(['feats.h5f', 'queries', '--distance', 'euclidean'])
    assert 'kl' in capsys.readouterr().err
    try:
        import h5features  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match='h5features'):
            qbe.QbeSearcher('feats.h5f')
