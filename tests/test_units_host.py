"""Penalised unit segmentation without a GPU: the restatement (tests/units_np.py) against brute force over every
labelling on half-integer grids, the new symbols in header and binding, the library's sizing queries and refusals (no
kernel is launched here), `segments`, the boundary scores on hand-made cases, and predict(penalty=None) taking the old
path."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import units_np  # noqa: E402
from conftest import ROOT  # noqa: E402

NAMES = ('abn_kmeans_viterbi', 'abn_kmeans_viterbi_ws_bytes', 'abn_kmeans_viterbi_max_len', 'abn_kmeans_viterbi_max_k')
PENALTIES = (0.0, 0.5, 1.0, 1.5, 3.0, 100.0)           # in score units: multiples of 1/2, exact in fp32


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def grid_cases():
    """Half-integer score grids with plenty of ties, T <= 6, K <= 3, some with BAD frames."""
    rng = np.random.default_rng(11)
    out = []
    for T, K in ((1, 1), (1, 3), (2, 2), (3, 3), (4, 2), (5, 3), (6, 2), (6, 3), (6, 3)):
        for rep in range(3):
            s = (rng.integers(-4, 5, size=(T, K)) / 2.0).astype(np.float32)
            good = np.ones(T, dtype=bool)
            if rep == 2:
                good = rng.random(T) > 0.35
            out.append((s, good))
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_restatement_attains_the_brute_force_optimum():
    for s, good in grid_cases():
        for p in PENALTIES:
            ids, obj, nsw = units_np.viterbi_one(s, good, p)
            best, arg = units_np.brute_force(s, good, p)
            assert (ids[~good] == -1).all() and (ids[good] >= 0).all()
            assert obj == best, (s, good, p)                                       # exact: the grid is half-integer
            assert units_np.J(s, ids, p) == best
            assert tuple(ids[good]) in arg
            assert nsw == units_np.switches(ids)


def test_zero_penalty_is_the_frame_wise_argmax_with_the_lowest_index_on_ties():
    for s, good in grid_cases():
        ids, obj, _ = units_np.viterbi_one(s, good, 0.0)
        assert np.array_equal(ids[good], np.argmax(s[good], axis=1)) if good.any() else (ids == -1).all()
        assert obj == float(s[good].max(axis=1).astype(np.float64).sum()) if good.any() else obj == 0.0
    s = np.array([[1, 1, 0], [0, 2, 2], [3, 3, 3]], dtype=np.float32)
    assert units_np.viterbi_one(s, np.ones(3, dtype=bool), 0.0)[0].tolist() == [0, 1, 0]


def test_switches_never_rise_with_the_penalty_and_a_huge_one_gives_the_best_column():
    for s, good in grid_cases():
        counts = [units_np.viterbi_one(s, good, p)[2] for p in PENALTIES]
        assert all(a >= b for a, b in zip(counts, counts[1:])), counts
        ids, obj, nsw = units_np.viterbi_one(s, good, 100.0)
        if good.any():
            col = s[good].astype(np.float64).sum(axis=0)
            assert nsw == 0 and (ids[good] == int(np.argmax(col))).all() and obj == col.max()


def test_bad_frames_pass_the_state_through():
    rng = np.random.default_rng(3)
    s = (rng.integers(-4, 5, size=(9, 3)) / 2.0).astype(np.float32)
    good = np.array([0, 1, 1, 0, 0, 1, 1, 0, 1], dtype=bool)
    for p in PENALTIES:
        ids, obj, nsw = units_np.viterbi_one(s, good, p)
        ids2, obj2, nsw2 = units_np.viterbi_one(s[good], np.ones(int(good.sum()), dtype=bool), p)
        assert (ids[~good] == -1).all() and np.array_equal(ids[good], ids2) and obj == obj2 and nsw == nsw2
    none = units_np.viterbi_one(s, np.zeros(9, dtype=bool), 1.0)
    assert (none[0] == -1).all() and none[1] == 0.0 and none[2] == 0
    empty = units_np.viterbi_one(s[:0], np.zeros(0, dtype=bool), 1.0)
    assert empty[0].shape == (0,) and empty[1] == 0.0 and empty[2] == 0


def test_tie_rules_by_hand():
    one = np.ones(3, dtype=bool)
    # W[1] = -1 = -p: the strict > does not stay, the path switches (both cost the same)
    s = np.array([[1, 0], [0, 0], [0, 1]], dtype=np.float32)
    ids, obj, nsw = units_np.viterbi_one(s, one, 1.0)
    assert obj == 1.0 and units_np.J(s, ids, 1.0) == 1.0
    # all equal: the lowest index everywhere, no switch
    ids, obj, nsw = units_np.viterbi_one(np.zeros((3, 4), dtype=np.float32), one, 0.5)
    assert ids.tolist() == [0, 0, 0] and nsw == 0 and obj == 0.0
    # corpus call: utterances in any order, rows outside keep their value
    s = (np.random.default_rng(0).integers(-3, 4, size=(10, 3)) / 2.0).astype(np.float32)
    good = np.ones(10, dtype=bool)
    a, oa, na = units_np.viterbi(s, good, [1, 6, 5], [4, 3, 0], 0.5)
    b, ob, nb = units_np.viterbi(s, good, [6, 5, 1], [3, 0, 4], 0.5)
    assert np.array_equal(a, b) and a[0] == -7 and a[5] == -7 and a[9] == -7
    assert oa.tolist() == [ob[2], ob[0], ob[1]] and na.tolist() == [nb[2], nb[0], nb[1]] and oa[2] == 0.0


def test_float64_optimum_agrees_with_the_restatement_on_exact_inputs():
    for s, good in grid_cases():
        for p in PENALTIES:
            assert units_np.optimum_f64(s.astype(np.float64), good, p) == units_np.viterbi_one(s, good, p)[1]


# ---- segments ------------------------------------------------------------------------------------------------------------
def test_segments_are_the_runs_without_the_bad_frames():
    from abnet3_amd.kmeans import segments, unit_sequences
    ids = {'a': np.array([3, 3, -1, 3, 1, 1, 1, -1, -1, 2], dtype=np.int32), 'b': np.zeros(0, dtype=np.int32),
           'c': np.array([-1, -1], dtype=np.int32), 'd': torch.tensor([5, 5, 5], dtype=torch.int32)}
    seg = segments(ids)
    assert [v.tolist() for v in seg['a']] == [[0, 3, 4, 9], [2, 4, 7, 10], [3, 3, 1, 2]]
    assert all(v.shape == (0,) and v.dtype == np.int64 for v in seg['b'] + seg['c'])
    assert [v.tolist() for v in seg['d']] == [[0], [3], [5]]
    for k in ids:
        ref = units_np.runs(np.asarray(ids[k]))
        assert all(np.array_equal(x, y) for x, y in zip(seg[k], ref))
    assert unit_sequences({'a': ids['a']})['a'].tolist() == [3, 1, 2]      # (collapse merges over a BAD frame, segments does not)


# ---- boundary scores -------------------------------------------------------------------------------------------------------
def _alignment():
    from abnet3_amd import tde
    files = ['f1'] * 4 + ['f2'] * 3
    onset = [0.0, 0.10, 0.25, 0.40, 0.0, 0.20, 0.30]
    offset = [0.10, 0.25, 0.40, 0.50, 0.20, 0.30, 0.45]
    return tde.make_alignment(files, onset, offset, ['SIL', 'a', 'b', 'SIL', 'c', 'SIL', 'SIL'])


def test_boundary_scores_by_hand():
    from abnet3_amd import tde
    al = _alignment()
    gold = tde.gold_boundaries(al)
    assert gold['f1'].tolist() == [0.10, 0.25, 0.40] and gold['f2'].tolist() == [0.20, 0.30]
    # f1: 0.11 hits 0.10, 0.18 misses, 0.26 hits 0.25, 0.40 is not found; f2: 0.31 hits 0.30, 0.20 is not found
    found = {'f1': [0.26, 0.11, 0.18], 'f2': [0.31]}
    s = tde.boundary_scores(found, al, tolerance=0.02)
    assert (s.n_found, s.n_gold, s.n_hit) == (4, 5, 3)
    assert s.precision == 0.75 and s.recall == 0.6
    assert s.f == pytest.approx(2 * 0.75 * 0.6 / 1.35, rel=1e-15)
    assert s.os == pytest.approx(0.6 / 0.75 - 1.0, rel=1e-15)
    r1 = np.sqrt(0.4 ** 2 + s.os ** 2)
    r2 = abs((-s.os + 0.6 - 1.0) / np.sqrt(2.0))
    assert s.r_value == pytest.approx(1.0 - (r1 + r2) / 2.0, rel=1e-15)
    ref = units_np.boundary_scores(found, {k: list(v) for k, v in gold.items()}, 0.02)
    assert all(getattr(s, k) == ref[k] for k in ref)
    # a perfect segmentation
    p = tde.boundary_scores({k: v for k, v in gold.items()}, al)
    assert p.precision == p.recall == p.f == p.r_value == 1.0 and p.os == 0.0


def test_boundary_scores_tolerance_edge_empty_sides_and_ignore():
    from abnet3_amd import tde
    al = tde.make_alignment(['f'] * 3, [0.0, 0.5, 1.0], [0.5, 1.0, 1.5], ['a', 'b', 'c'])
    # 0.5 + 0.25 and 1.0 - 0.25 are exact in binary: |f - g| == tolerance is a hit, a hair more is not
    assert tde.boundary_scores({'f': [0.75]}, al, tolerance=0.25).n_hit == 1
    assert tde.boundary_scores({'f': [np.nextafter(0.75, 1.0)]}, al, tolerance=0.25).n_hit == 1   # ... but then 1.0 is in reach
    assert tde.boundary_scores({'f': [0.75]}, al, tolerance=np.nextafter(0.25, 0.0)).n_hit == 0
    # one found boundary cannot hit two gold ones, nor two found ones the same gold one
    assert tde.boundary_scores({'f': [0.75]}, al, tolerance=0.3).n_hit == 1
    assert tde.boundary_scores({'f': [0.49, 0.51]}, al, tolerance=0.05).n_hit == 1
    e = tde.boundary_scores({}, al)
    assert (e.n_found, e.n_gold, e.n_hit) == (0, 2, 0) and e.precision == e.recall == e.f == e.os == 0.0
    assert e.r_value == pytest.approx(1.0 - (1.0 + 1.0 / np.sqrt(2.0)) / 2.0, rel=1e-15)
    single = tde.make_alignment(['f'], [0.0], [1.0], ['a'])
    g = tde.boundary_scores({'f': [0.3]}, single)
    assert (g.n_found, g.n_gold, g.n_hit) == (1, 0, 0) and g.precision == g.recall == 0.0
    with pytest.raises(ValueError, match='not in the alignment'):
        tde.boundary_scores({'nope': [0.1]}, al)
    # ignore: the onset between two ignored phones is no boundary
    gold = tde.gold_boundaries(_alignment(), ignore=('SIL',))
    assert gold['f1'].tolist() == [0.10, 0.25, 0.40] and gold['f2'].tolist() == [0.20]


def test_unit_boundaries_lie_midway_between_the_frames_of_a_switch():
    from abnet3_amd import tde
    times = {'a': 0.005 + 0.01 * np.arange(8)}
    b = tde.unit_boundaries({'a': np.array([2, 2, -1, 2, 4, 4, -1, 1])}, times)
    assert b['a'].tolist() == [0.5 * (times['a'][3] + times['a'][4]), 0.5 * (times['a'][5] + times['a'][7])]
    assert tde.unit_boundaries({'a': np.full(8, -1)}, times)['a'].shape == (0,)
    with pytest.raises(ValueError, match='8 times'):
        tde.unit_boundaries({'a': np.zeros(3, dtype=np.int32)}, times)


# ---- the library, no launch ------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_new_names(lib):
    from abnet3_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(abn_[a-z0-9_]+)\s*\(', text))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 20 and lib.abn_abi_version() == 20


def test_sizing_queries_and_refusals(lib):
    from abnet3_amd import kmeans
    ws = lib.abn_kmeans_viterbi_ws_bytes
    assert kmeans.viterbi_max_k() == lib.abn_kmeans_viterbi_max_k() >= 1024
    assert kmeans.viterbi_max_len() == lib.abn_kmeans_viterbi_max_len() >= 1 << 16
    up = lambda v: (v + 255) // 256 * 256

    def layout(n_utt, max_len, K):
        # per workgroup (one per utterance, 256 at most): 128 x (K rounded up to 128) fp32 scores, per frame one 64-bit
        # word of stay bits per 64 centroids (K rounded up to 256, 512, 1024, 2048, 4096) and an int32, 8 bytes of slack
        ks, kw = (K + 127) // 128 * 128, 4
        while kw * 64 < K:
            kw *= 2
        return min(n_utt, 256) * up(128 * ks * 4 + max_len * (8 * kw + 4) + 8)
    for n_utt, max_len, K, D in ((1, 1, 1, 1), (3, 300, 129, 40), (5000, 1000, 1024, 100), (256, 0, 300, 8), (257, 130, 4096, 512)):
        assert ws(n_utt, max_len, K, D) == layout(n_utt, max_len, K), (n_utt, max_len, K, D)
    # no T x K array: 1.14 M frames in utterances of up to 1000 frames, K = 1024
    assert ws(2000, 1000, 1024, 40) < 1140000 * 1024 * 4 // 4
    for args in ((0, 10, 4, 4), (1 << 31, 10, 4, 4), (1, -1, 4, 4), (1, lib.abn_kmeans_viterbi_max_len() + 1, 4, 4), (1, 10, 0, 4),
                 (1, 10, lib.abn_kmeans_viterbi_max_k() + 1, 4), (1, 10, 4, 0), (1, 10, 4, 513)):
        assert ws(*args) == -1, args
        assert b'abn_kmeans_viterbi_ws_bytes' in lib.abn_last_error()


def test_library_refuses_bad_arguments_before_any_launch(lib):
    from abnet3_amd import _lib
    p = ctypes.c_void_p(0x10000)
    big = 1 << 30
    call = lib.abn_kmeans_viterbi
    good = [p, 100, 4, p, p, 2, p, p, p, 8, 0.5, p, None, None, p, big, None]

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)
    for i in (0, 3, 4, 6, 7, 8, 11):                                   # x, off, len, shift, m, b, ids
        assert with_(**{'a%d' % i: None}) == _lib.E_ARG, i
        assert b'null pointer' in lib.abn_last_error()
    assert with_(a1=0) == _lib.E_ARG and with_(a1=1 << 31) == _lib.E_ARG                 # T
    assert with_(a2=0) == _lib.E_ARG and with_(a5=0) == _lib.E_ARG and with_(a9=0) == _lib.E_ARG     # D, n_utt, K
    assert with_(a2=513) == _lib.E_UNSUPPORTED and with_(a9=lib.abn_kmeans_viterbi_max_k() + 1) == _lib.E_UNSUPPORTED
    for pen in (-0.5, float('nan'), float('inf')):
        assert with_(a10=pen) == _lib.E_ARG
        assert b'penalty_score' in lib.abn_last_error()
    assert with_(a14=None) == _lib.E_WORKSPACE and with_(a15=1024) == _lib.E_WORKSPACE
    assert with_(a15=2 * (128 * 128 * 4 + 8)) == _lib.E_WORKSPACE                        # the slabs alone: no frame fits
    assert with_(a14=ctypes.c_void_p(0x10004)) == _lib.E_ARG


def test_python_layer_refuses_on_the_host(lib):
    from abnet3_amd import kmeans
    for bad in (-1.0, float('nan'), float('inf'), 1e39, 'x', None):
        with pytest.raises(ValueError, match='penalty'):
            kmeans.check_penalty('t', bad)
    assert kmeans.check_penalty('t', 0) == 0.0 and kmeans.check_penalty('t', np.float32(1.5)) == 1.5
    q = kmeans.KMeansQuantizer(2)
    with pytest.raises(ValueError, match='fit or load'):
        q.segment(torch.zeros(4, 3), 1.0)
    with pytest.raises(ValueError, match='penalty'):
        q.segment(torch.zeros(4, 3), -1.0)
    q.centroids_, q.counts_, q.shift_ = np.zeros((2, 3)), np.zeros(2), np.zeros(3, dtype=np.float32)
    with pytest.raises(ValueError, match='D = 4'):
        q.segment(torch.zeros(4, 4), 1.0)
    with pytest.raises(ValueError, match='float32'):
        q.segment(torch.zeros(4, 3, dtype=torch.float64), 1.0)
    with pytest.raises(ValueError, match='abn_kmeans_viterbi_max_len'):
        q.segment(torch.zeros(kmeans.viterbi_max_len() + 1, 3), 1.0)
    assert q.last_objective_ is None and q.last_n_switch_ is None
    # the refusal table of kmeans.viterbi's utterances (5 rows; the checks it shares with both HMM entries)
    from abnet3_amd import _utt
    spans = lambda off=(0, 3), lens=(3, 2), longest=kmeans.viterbi_max_len(): _utt.utterance_spans(
        'kmeans.viterbi', off, lens, 5, longest, 'abn_kmeans_viterbi_max_len')
    for kw, match in ((dict(lens=[3]), '2 offsets and 1 lengths'), (dict(lens=[3, 4]), 'outside the table\'s 5 rows'),
                      (dict(off=[-1, 3]), 'outside the table'), (dict(off=[0, 2]), 'kmeans.viterbi: utterances overlap'),
                      (dict(off=[2, 0], lens=[3, 3]), 'kmeans.viterbi: utterances overlap'),
                      (dict(longest=2), 'of 3 frames, the kernel takes up to 2 \\(abn_kmeans_viterbi_max_len\\)')):
        with pytest.raises(ValueError, match=match):
            spans(**kw)
    off_h, len_h, n_utt, longest = spans(off=torch.tensor([3, 0]), lens=[2, 3])          # touching, in any order: not an overlap
    assert off_h.tolist() == [3, 0] and len_h.tolist() == [2, 3] and off_h.dtype == len_h.dtype == np.int64 and (n_utt, longest) == (2, 3)
    assert spans(off=[], lens=[])[2:] == (0, 0) and _utt.starts([3, 0, 2]).tolist() == [0, 3, 3]
    ap = kmeans.parser()
    assert ap.parse_args(['transform', 'm.npz', 'f.npz', 'o.npz']).penalty is None
    assert ap.parse_args(['transform', 'm.npz', 'f.npz', 'o.npz', '--penalty', '2.5']).penalty == 2.5


def test_predict_without_a_penalty_takes_the_old_path(monkeypatch):
    from abnet3_amd import kmeans
    q = kmeans.KMeansQuantizer(2)
    calls = []
    monkeypatch.setattr(q, '_assign', lambda table, **kw: calls.append('assign') or torch.zeros(table.shape[0], dtype=torch.int32))
    monkeypatch.setattr(q, '_segment_ids', lambda table, rows, penalty: calls.append(('segment', penalty)) or
                        torch.ones(table.shape[0], dtype=torch.int32))
    monkeypatch.setattr(kmeans, 'viterbi', lambda *a, **k: pytest.fail('viterbi without a penalty'))
    t = torch.zeros(5, 3)
    assert q.predict(t).tolist() == [0] * 5 and q.predict(t, penalty=None).tolist() == [0] * 5
    assert calls == ['assign', 'assign']
    assert q.predict(t, penalty=0.0).tolist() == [1] * 5 and q.segment(t, 2.0).tolist() == [1] * 5
    assert calls[2:] == [('segment', 0.0), ('segment', 2.0)]
