"""ES-KMeans without a GPU: the restated DP (tests/esk_np.py) against brute force over every segmentation on half-integer
cost grids, the landmark helpers, the .classes round trip, the new symbols in header and binding, and the library's
refusals and sizing query (no kernel is launched here)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esk_np  # noqa: E402
from conftest import ROOT  # noqa: E402

NAMES = ('abn_esk_max_span', 'abn_esk_score', 'abn_esk_segment')


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def grid_cases():
    """(c [L, S] float32 half-integer costs, L, S): plenty of ties, some candidates blocked, some utterances cut off."""
    rng = np.random.default_rng(5)
    out = []
    for L in (1, 2, 3, 5, 7, 10):
        for S in (1, 2, 3, 6):
            for rep in range(4):
                c = (rng.integers(0, 7, size=(L, S)) / 2.0).astype(np.float32)
                if rep >= 2:
                    c[rng.random((L, S)) < (0.25 if rep == 2 else 0.6)] = np.inf
                out.append((c, L, S))
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_restated_dp_equals_brute_force():
    n_unreachable = n_tied = 0
    for c, L, S in grid_cases():
        span, obj, n_seg = esk_np.dp_one(c, L, S)
        best, arg = esk_np.brute_force(c, L, S)
        if arg is None:
            n_unreachable += 1
            assert np.isnan(obj) and n_seg == -1 and (span == -1).all()
            continue
        assert obj == best, (c, L, S)                                  # exact: the grid is half-integer
        starts = np.flatnonzero(span >= 1)
        assert list(span[starts]) == arg, (c, L, S)                    # the tie rule: smallest last span, and so on
        assert n_seg == len(arg) and span[L] == -1 and starts[0] == 0
        assert sum(arg) == L
        n_tied += 1
    assert n_unreachable >= 5 and n_tied >= 50


def test_the_tie_goes_to_the_smallest_last_span():
    c = np.array([[1.0, 2.0], [1.0, 2.0], [1.0, 0.0]], dtype=np.float32)       # 1+1+1 = 1+2 = 2+1 = 3
    span, obj, n_seg = esk_np.dp_one(c, 3, 2)
    assert obj == 3.0 and list(span) == [1, 1, 1, -1] and n_seg == 3
    c[0, 0] = 2.0                                                              # 0 -> 2 -> 3 = 2 + 1 alone is left at 3
    span, obj, n_seg = esk_np.dp_one(c, 3, 2)
    assert obj == 3.0 and list(span) == [2, -1, 1, -1] and n_seg == 2


def test_corpus_dp_marks_cuts_words_and_spans():
    lm = np.array([0, 3, 5, 9, 20, 21, 30], dtype=np.int64)
    lm_off = np.array([0, 4, 7], dtype=np.int64)
    S = 2
    best = np.full(len(lm) * S, np.nan, dtype=np.float32)
    ids = np.full(len(lm) * S, -1, dtype=np.int32)
    for g, s, v, k in ((0, 1, 0.5, 3), (1, 1, 0.5, 4), (2, 1, 0.5, 5), (0, 2, 0.5, 6), (1, 2, 1.0, 7), (4, 1, 0.5, 1)):
        best[g * S + s - 1], ids[g * S + s - 1] = v, k
    cut, word, span, obj, n_seg = esk_np.dp(best, ids, lm, lm_off, S)
    # utterance 0: costs n (1 - 2 best): (0,1) 0, (1,1) 0, (2,1) 0, (0,2) 0, (1,2) -6: 0 -> 1 -> 3 = -6
    assert list(cut[:4]) == [1, 1, 0, 1] and list(span[:4]) == [1, 2, -1, -1] and list(word[:4]) == [3, 7, -1, -1]
    assert obj[0] == -6.0 and n_seg[0] == 2
    # utterance 1: (5, 1) is blocked and (4, 2) too: unreachable, nothing marked
    assert np.isnan(obj[1]) and n_seg[1] == -1 and not cut[4:].any() and (word[4:] == -1).all() and (span[4:] == -1).all()


def test_restated_vector_follows_the_sampling_rule():
    rng = np.random.default_rng(2)
    table = rng.standard_normal((30, 3)).astype(np.float32)
    v, keep, bad = esk_np.vector(table, 4, 7, 5)
    rows = [4 + ((2 * j + 1) * 7) // 10 for j in range(5)]
    x = table[rows].ravel().astype(np.float64)
    assert keep and not bad and np.allclose(v, x / np.sqrt((x * x).sum()), rtol=2e-7, atol=0)
    v1, _, _ = esk_np.vector(table, 9, 1, 5)                                   # one frame: the row repeats
    assert np.array_equal(v1[:3], v1[12:])
    table[5] = 0.0
    assert esk_np.vector(table, 5, 1, 5)[1:] == (False, True)
    table[5, 1] = np.nan
    assert esk_np.vector(table, 5, 1, 5)[2]
    assert abs(esk_np.sum_of_squares(np.arange(200, dtype=np.float32)) - float((np.arange(200.0) ** 2).sum())) < 1e-6


# ---- landmarks ---------------------------------------------------------------------------------------------------------
def test_landmark_helpers():
    from abnet3_amd import eskmeans
    lms = eskmeans.uniform_landmarks({'a': 12, 'b': 5, 'c': 0, 'd': np.zeros((11, 2), dtype=np.float32)}, 5)
    assert list(lms) == ['a', 'b', 'd']
    assert list(lms['a']) == [0, 5, 10, 12] and list(lms['b']) == [0, 5] and list(lms['d']) == [0, 5, 10, 11]
    with pytest.raises(ValueError):
        eskmeans.uniform_landmarks({'a': 3}, 0)
    from abnet3_amd.kmeans import segments
    ids = {'a': np.array([2, 2, 5, 5, 5, -1, 1, 1]), 'b': np.array([-1, -1]), 'c': np.array([-1, 3, 3])}
    seg = segments(ids)
    lms = eskmeans.landmarks_from_units(seg)
    assert list(lms['a']) == [0, 2, 5, 6, 8] and 'b' not in lms and list(lms['c']) == [1, 3]
    lms = eskmeans.landmarks_from_units(seg, {'a': 8, 'b': 2, 'c': 3})
    assert list(lms['b']) == [0, 2] and list(lms['c']) == [0, 1, 3]
    names, lm, off = eskmeans.pack_landmarks({'c': [0, 1, 3], 'a': [0, 2, 8]}, {'a': 10, 'b': 18, 'c': 20}, {'a': 8, 'b': 2, 'c': 3})
    assert names == ['a', 'c'] and list(lm) == [10, 12, 18, 20, 21, 23] and list(off) == [0, 3, 6]
    for wrong in ([0], [0, 0, 3], [0, 4], [-1, 2]):
        with pytest.raises(ValueError):
            eskmeans.pack_landmarks({'c': wrong}, {'c': 20}, {'c': 3})


def test_initial_spans_cover_every_utterance_with_allowed_spans():
    from abnet3_amd import eskmeans
    lm = np.array([0, 4, 8, 30, 34, 40, 50, 53], dtype=np.int64)
    off = np.array([0, 5, 8], dtype=np.int64)
    for seed in range(20):
        span = eskmeans.initial_spans(lm, off, 3, 10, np.random.default_rng(seed))
        for lo, hi in ((0, 5), (5, 8)):
            g = lo
            while g < hi - 1:
                s = int(span[g])
                assert 1 <= s <= 3 and g + s <= hi - 1 and (s == 1 or lm[g + s] - lm[g] <= 10)
                assert (span[g + 1:g + s] == -1).all()
                g += s
            assert g == hi - 1 and span[hi - 1] == -1
    assert np.array_equal(eskmeans.initial_spans(lm, off, 3, 10, np.random.default_rng(3)),
                          eskmeans.initial_spans(lm, off, 3, 10, np.random.default_rng(3)))


def test_classes_round_trip(tmp_path):
    from abnet3_amd import eskmeans, tde
    q = eskmeans.ESKMeans(4)
    times = {'u1': 0.0125 + 0.01 * np.arange(30), b'u2': 0.0125 + 0.01 * np.arange(20)}
    seg = {'u1': (np.array([0, 10, 18]), np.array([10, 18, 30]), np.array([2, 0, 2], dtype=np.int32)),
           b'u2': (np.array([0, 5]), np.array([5, 20]), np.array([0, 3], dtype=np.int32))}
    q._last = (['u1', b'u2'], times, seg)
    assert q.clusters == [[(0, 10, 17), (1, 0, 4)], [(0, 0, 9), (0, 18, 29)], [(1, 5, 19)]]
    path = q.write_classes(str(tmp_path / 'esk.classes'))
    back = tde.read_classes(path)
    want = [[('u1', times['u1'][10], times['u1'][17]), ('u2', times[b'u2'][0], times[b'u2'][4])],
            [('u1', times['u1'][0], times['u1'][9]), ('u1', times['u1'][18], times['u1'][29])],
            [('u2', times[b'u2'][5], times[b'u2'][19])]]
    assert back == [[(f, float(a), float(b)) for f, a, b in c] for c in want]
    bd = q.boundaries()
    assert np.array_equal(bd['u1'], 0.5 * (times['u1'][[9, 17]] + times['u1'][[10, 18]]))
    assert np.array_equal(bd['u2'], 0.5 * (times[b'u2'][[4]] + times[b'u2'][[5]]))
    assert q.whoami() == {'class_name': 'ESKMeans', 'params': {'n_clusters': 4, 'frames': 10, 'max_span': 6, 'max_frames': None,
                                                               'n_iter': 10, 'seed': 0}}
    with pytest.raises(ValueError):
        eskmeans.ESKMeans(4).boundaries()
    with pytest.raises(ValueError):
        eskmeans.ESKMeans(0)


# ---- header, binding, library --------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree(lib):
    from abnet3_amd import _lib, build
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read(), flags=re.S)
    raw = ctypes.CDLL(lib._name)
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.SYMBOLS and hasattr(raw, name), name
    assert len(_lib.SYMBOLS['abn_esk_score'][1]) == 16 and len(_lib.SYMBOLS['abn_esk_segment'][1]) == 13
    assert 'eskmeans.hip' in build.SOURCES and '-ffp-contract=off' in build.STRICT_FP['eskmeans.hip']
    assert lib.abn_abi_version() == 20


def test_refusals_before_any_launch(lib):
    from abnet3_amd import _lib, eskmeans
    a = ctypes.c_void_p(0x10000)
    assert lib.abn_esk_max_span() == 8 == eskmeans.max_span()
    score = lambda T=100, D=40, n_utt=1, n_lm=5, frames=10, S=6, mf=50, K=8, p=a: lib.abn_esk_score(
        p, T, D, p, p, n_utt, n_lm, frames, S, mf, p, p, K, p, p, None)
    assert score(p=None) == _lib.E_ARG and b'null' in lib.abn_last_error()
    for kw in (dict(T=0), dict(D=0), dict(n_utt=0), dict(n_lm=1), dict(frames=0), dict(S=0), dict(mf=0), dict(K=0),
               dict(n_lm=(1 << 31) // 6, S=6)):
        assert score(**kw) == _lib.E_ARG, kw
    for kw in (dict(S=9), dict(frames=13), dict(D=513, frames=1), dict(K=lib.abn_kmeans_max_k() + 1), dict(frames=513, D=1)):
        assert score(**kw) == _lib.E_UNSUPPORTED, kw
        assert b'abn_esk_score' in lib.abn_last_error()
    seg = lambda n_utt=1, n_lm=5, S=6, p=a, opt=None: lib.abn_esk_segment(p, p, p, p, n_utt, n_lm, S, p, p, p, opt, opt, None)
    assert seg(p=None) == _lib.E_ARG
    for kw in (dict(n_utt=0), dict(n_lm=1), dict(S=0)):
        assert seg(**kw) == _lib.E_ARG, kw
    assert seg(S=9) == _lib.E_UNSUPPORTED and b'abn_esk_max_span' in lib.abn_last_error()


def test_python_refusals_need_no_device(lib):
    import torch
    from abnet3_amd import eskmeans
    with pytest.raises(ValueError, match='max_span'):
        eskmeans.candidate_scores(torch.zeros(4, 2), [0, 4], [0, 2], torch.zeros(1, 4), torch.zeros(1), frames=2, max_span=9)
    with pytest.raises(ValueError, match='float32 table'):
        eskmeans.candidate_scores(torch.zeros(4, 2, dtype=torch.float64), [0, 4], [0, 2], torch.zeros(1, 4), torch.zeros(1), frames=2)
    with pytest.raises(Exception, match='no CPU fallback'):
        eskmeans.candidate_scores(torch.zeros(4, 2), [0, 4], [0, 2], torch.zeros(1, 4), torch.zeros(1), frames=2)
