"""KMeansQuantizer without a GPU: the float64 restatement (tests/kmeans_np.py) on hand-computed cases, the bitrate and
unit-sequence helpers, the save / load round trip, the command line's arguments, the new symbols in header and binding,
and the library's argument checks and workspace sizing (no kernel is launched here)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_np  # noqa: E402
from conftest import ROOT  # noqa: E402

NAMES = ('abn_kmeans_max_d', 'abn_kmeans_max_k', 'abn_kmeans_assign', 'abn_kmeans_ws_bytes', 'abn_kmeans_accumulate',
         'abn_kmeans_update', 'abn_dtw_cost_parallel_batched')


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


# ---- the restatement on cases worked out by hand -----------------------------------------------------------------------
def test_assignment_tie_goes_to_the_lowest_k_and_bad_rows_get_minus_one():
    # centred frames on a line; centroids at -1, +1 and a duplicate of +1: the frame at 0 is equally far from all three
    xc = np.array([[-1.0], [0.0], [1.0], [np.nan], [0.5]], dtype=np.float32)
    bad = np.array([False, False, False, True, False])
    m, b = kmeans_np.tables(np.array([[-1.0], [1.0], [1.0]]))
    assert np.array_equal(b, np.float32([-0.5, -0.5, -0.5]))
    ids, s, E = kmeans_np.assign(xc, bad, m, b)
    assert list(ids) == [0, 0, 1, -1, 1]
    assert np.allclose(s[0], [0.5, -1.5, -1.5]) and s[1, 0] == s[1, 1] == s[1, 2] == -0.5
    g = kmeans_np.gamma(2)
    assert np.allclose(E, g * np.array([1.5, 0.5, 1.5, 0.5, 1.0]))       # max_k (|xc m| + |b|); the BAD row counts as zeros


def test_statistics_update_and_empty_cluster_by_hand():
    xc = np.array([[0.0, 0.0], [2.0, 0.0], [10.0, 10.0], [np.inf, 0.0]], dtype=np.float32)
    bad = np.array([False, False, False, True])
    mu = np.array([[1.0, 0.0], [9.0, 9.0], [-50.0, -50.0]])              # nobody is nearest to the third
    ids, inertia, mu2, empty = kmeans_np.iteration(xc, bad, mu)
    assert list(ids) == [0, 0, 1, -1]
    m, _ = kmeans_np.tables(mu)
    N, S, d2 = kmeans_np.statistics(xc, ids, m, 3)
    assert list(N) == [2.0, 1.0, 0.0]
    assert np.array_equal(S, [[2.0, 0.0], [10.0, 10.0], [0.0, 0.0]])
    assert list(d2) == [1.0, 1.0, 2.0, 0.0] and inertia == 4.0 / 3.0
    assert np.array_equal(mu2, [[1.0, 0.0], [10.0, 10.0], [-50.0, -50.0]]) and empty == 1      # the empty one is kept
    assert np.allclose(kmeans_np.sum_bound(xc, ids, 3), [[kmeans_np.gamma(2) * 2.0, 0.0], [kmeans_np.gamma(1) * 10.0] * 2,
                                                         [0.0, 0.0]])


def test_prepare_centres_on_the_good_frames_and_marks_overflow():
    x = np.array([[1.0, 2.0], [3.0, 6.0], [np.nan, 0.0]], dtype=np.float32)
    xc, bad, shift = kmeans_np.prepare(x)
    assert np.array_equal(shift, np.float32([2.0, 4.0])) and list(bad) == [False, False, True]
    assert np.array_equal(xc[:2], np.float32([[-1.0, -2.0], [1.0, 2.0]]))
    x = np.zeros((8, 2), dtype=np.float32)
    x[7, 0] = 1e20                                   # finite, and so is the mean 1.25e19 -- its centred square is not
    xc, bad, shift = kmeans_np.prepare(x)
    assert shift[0] == np.float32(1.25e19) and list(bad) == [False] * 7 + [True]


def test_cosine_renormalises_and_ignores_scale():
    x = np.array([[3.0, 4.0], [30.0, 40.0], [0.0, 2.0], [0.0, 0.0]], dtype=np.float32)
    xc, bad, shift = kmeans_np.prepare(x, 'cosine')
    assert not shift.any() and list(bad) == [False, False, False, True]             # the all-zero row is BAD
    assert np.array_equal(xc[0], xc[1]) and np.allclose(xc[0], [0.6, 0.8])
    mu = np.array([[1.0, 0.0], [0.0, 1.0]])
    m, b = kmeans_np.tables(mu, 'cosine')
    assert not b.any()
    ids, _, _ = kmeans_np.assign(xc, bad, m, b)
    assert list(ids) == [1, 1, 1, -1]
    N, S, _ = kmeans_np.statistics(xc, ids, m, 2)
    mu2, empty = kmeans_np.update(N, S, mu, 'cosine')
    assert empty == 1 and np.array_equal(mu2[0], mu[0])
    mean = (2.0 * xc[0].astype(np.float64) + [0.0, 1.0]) / 3.0
    assert np.allclose(mu2[1], mean / np.linalg.norm(mean), rtol=0, atol=1e-15)
    assert abs(np.linalg.norm(mu2[1]) - 1.0) < 1e-15


def test_float64_inertia_does_not_increase():
    rng = np.random.default_rng(0)
    x = (rng.normal(size=(4, 3))[rng.integers(0, 4, 400)] * 5 + rng.normal(size=(400, 3))).astype(np.float32)
    xc, bad, _ = kmeans_np.prepare(x)
    mu = xc[:4].astype(np.float64)
    last = np.inf
    for _ in range(8):
        _, inertia, mu, _ = kmeans_np.iteration(xc, bad, mu)
        assert inertia <= last * (1 + 1e-12)
        last = inertia


# ---- helpers -------------------------------------------------------------------------------------------------------------
def test_unit_sequences_and_bitrate_known_answers():
    from abnet3_amd.kmeans import bitrate, unit_sequences
    ids = {'a': np.array([3, 3, 3, 5, 5, -1, 5, 3], dtype=np.int32), 'b': np.array([-1, -1], dtype=np.int32),
           'c': torch.tensor([7], dtype=torch.int32)}
    seq = unit_sequences(ids)
    assert list(seq) == ['a', 'b', 'c']
    assert list(seq['a']) == [3, 5, 3] and list(seq['b']) == [] and list(seq['c']) == [7]   # (the BAD frame is dropped first)
    assert list(unit_sequences(ids, collapse=False)['a']) == [3, 3, 3, 5, 5, 5, 3]
    # two symbols at equal frequency, 100 symbols in 1 s: 1 bit each
    assert bitrate({'x': np.arange(100) % 2}, 1.0) == pytest.approx(100.0, abs=1e-12)
    assert bitrate([np.zeros(50, dtype=int)], 2.0) == 0.0                                  # one symbol: no information
    assert bitrate({'x': np.arange(8), 'y': np.arange(8)}, 4.0) == pytest.approx(16 / 4.0 * 3.0)
    p = np.array([0.5, 0.25, 0.25])
    assert bitrate([np.array([0, 0, 1, 2])], 0.5) == pytest.approx(8.0 * -(p * np.log2(p)).sum())
    assert bitrate({}, 1.0) == 0.0
    with pytest.raises(ValueError):
        bitrate([np.arange(4)], 0.0)


def test_save_load_round_trip(tmp_path):
    from abnet3_amd.kmeans import KMeansQuantizer
    q = KMeansQuantizer(3, n_iter=7, tol=1e-3, metric='cosine', seed=5)
    rng = np.random.default_rng(0)
    q.centroids_ = rng.normal(size=(3, 4))
    q.counts_ = np.array([5.0, 0.0, 7.0])
    q.shift_ = rng.normal(size=4).astype(np.float32)
    q.inertias = [3.0, 2.5]
    q.n_bad_, q.n_empty_ = 2, 1
    path = str(tmp_path / 'km.npz')
    q.save(path)
    h = KMeansQuantizer.load(path)
    assert h.whoami() == q.whoami() and h.whoami()['class_name'] == 'KMeansQuantizer'
    assert h.whoami()['params'] == dict(n_clusters=3, n_iter=7, tol=1e-3, metric='cosine', seed=5)
    for k in ('centroids_', 'counts_', 'shift_'):
        assert np.array_equal(getattr(q, k), getattr(h, k)) and getattr(q, k).dtype == getattr(h, k).dtype, k
    assert h.inertias == q.inertias and (h.n_bad_, h.n_empty_) == (2, 1)
    with pytest.raises(ValueError):
        KMeansQuantizer(3).save(path)
    np.savez(str(tmp_path / 'other.npz'), weights=np.zeros(3))
    with pytest.raises(ValueError, match='not a KMeansQuantizer'):
        KMeansQuantizer.load(str(tmp_path / 'other.npz'))


def test_constructor_and_export():
    import abnet3_amd
    from abnet3_amd.kmeans import KMeansQuantizer
    assert abnet3_amd.KMeansQuantizer is KMeansQuantizer
    q = KMeansQuantizer(50)
    assert (q.n_iter, q.tol, q.metric, q.seed) == (20, 1e-4, 'euclidean', 0)
    with pytest.raises(ValueError):
        KMeansQuantizer(0)
    with pytest.raises(ValueError, match='metric'):
        KMeansQuantizer(4, metric='manhattan')
    with pytest.raises(ValueError, match='fit or load'):
        KMeansQuantizer(2).predict(torch.zeros(10, 4))


def test_abx_parallel_option_is_checked_on_the_host():
    from abnet3_amd.abx import ABXEvaluator, dtw_cost_batch
    with pytest.raises(ValueError, match='parallel'):
        dtw_cost_batch(None, None, None, None, None, None, parallel='clip')
    with pytest.raises(ValueError, match='only'):
        dtw_cost_batch(None, None, None, None, None, None, distance='kl', parallel='zero')
    with pytest.raises(ValueError, match='parallel'):
        ABXEvaluator(None, None, parallel='clip')


def test_command_line_arguments():
    from abnet3_amd import kmeans
    ap = kmeans.parser()
    a = ap.parse_args(['fit', 'f.npz', 'm.npz'])
    assert (a.cmd, a.features, a.model, a.n_clusters, a.n_iter, a.tol, a.metric, a.seed) == \
        ('fit', 'f.npz', 'm.npz', 50, 20, 1e-4, 'euclidean', 0)
    a = ap.parse_args(['fit', 'f.h5f', 'm.npz', '-k', '100', '--n-iter', '5', '--tol', '0', '--metric', 'cosine', '--seed', '3'])
    assert (a.n_clusters, a.n_iter, a.tol, a.metric, a.seed) == (100, 5, 0.0, 'cosine', 3)
    a = ap.parse_args(['transform', 'm.npz', 'f.npz', 'out.npz'])
    assert (a.cmd, a.model, a.features, a.out, a.quantize) == ('transform', 'm.npz', 'f.npz', 'out.npz', False)
    assert ap.parse_args(['transform', 'm.npz', 'f.npz', 'out.npz', '--quantize']).quantize
    for bad in (['fit', 'f.npz'], ['fit', 'f.npz', 'm.npz', '--metric', 'l1'], ['score', 'm.npz', 'f.npz'], []):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


# ---- the library, no launch ----------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_new_names(lib):
    from abnet3_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(abn_[a-z0-9_]+)\s*\(', text))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 20 and lib.abn_abi_version() == 20
    assert 'ABN_ABI_VERSION 20' in re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read())


def test_limits_and_value_errors(lib):
    from abnet3_amd import gmm, kmeans
    assert kmeans.max_k() == 4096 == gmm.max_k() and kmeans.max_d() == 512
    with pytest.raises(ValueError, match='T < K'):
        kmeans.KMeansQuantizer(8).fit(torch.zeros(3, 4))
    with pytest.raises(ValueError, match='abn_kmeans_max_d'):
        kmeans.KMeansQuantizer(2).fit(torch.zeros(10, 513))
    with pytest.raises(ValueError, match='abn_kmeans_max_k'):
        kmeans.KMeansQuantizer(4097).fit(torch.zeros(2 * 4097, 4))
    with pytest.raises(ValueError, match='float32'):
        kmeans.KMeansQuantizer(2).fit(torch.zeros(10, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match='float32'):
        kmeans.KMeansQuantizer(2).fit({'a': np.zeros((10, 4))})


def test_workspace_sizing_and_refusals(lib):
    ws = lib.abn_kmeans_ws_bytes
    up = lambda v: (v + 15) // 16 * 16

    def layout(ranges, K, D, tiles):
        # [ranges][K][D] fp32 sums, [ranges][K] int32 counts, [ranges][tiles][4 waves] float64 inertia partials, each
        # part starting on a multiple of 16 bytes
        return up(up(ranges * K * D * 4) + ranges * K * 4) + ranges * tiles * 4 * 8

    # centroids per workgroup: 128 halved while 128 D > 8192 floats of LDS, at least 16
    assert ws(300, 130, 39, 3) == layout(3, 130, 39, 2) == 60848 + 1568 + 192
    assert ws(300, 130, 39, 2) == layout(2, 130, 39, 2)
    assert ws(300, 130, 39, 9) == ws(300, 130, 39, 3)                     # 300 frames are three blocks of 128: three ranges at most
    assert ws(1000, 300, 280, 1) == layout(1, 300, 280, 19)               # D = 280: tiles of 16 centroids
    assert ws(1000, 300, 100, 1) == layout(1, 300, 100, 5)                # D = 100: tiles of 64
    assert ws(1, 1, 1, 0) == 16 + 16 + 32
    assert ws(1140000, 1024, 40, 0) == layout(255, 1024, 40, 8)           # by the grid: 8 tiles, 8907 blocks in ranges of 35
    assert ws(1000, 4096, 512, 0) > 0
    for T, K, D, r in ((1000, 0, 4, 0), (1000, 4097, 4, 0), (1000, 4, 513, 0), (1000, 4, 0, 0), (0, 4, 4, 0), (1000, 4, 4, -1),
                       (1000, 4, 4, 1025), (1 << 31, 4, 4, 0)):
        assert ws(T, K, D, r) == -1, (T, K, D, r)
        assert b'abn_kmeans_ws_bytes' in lib.abn_last_error()


def test_library_refuses_bad_arguments_before_any_launch(lib):
    from abnet3_amd import _lib
    p = ctypes.c_void_p(0x10000)
    assert lib.abn_kmeans_assign(None, 10, 4, p, p, p, 2, None, p, None, None, None) == _lib.E_ARG
    assert b'null' in lib.abn_last_error()
    assert lib.abn_kmeans_assign(p, 0, 4, p, p, p, 2, None, p, None, None, None) == _lib.E_ARG
    assert b'T = 0' in lib.abn_last_error()
    assert lib.abn_kmeans_assign(p, 10, 4, p, p, p, 2, p, p, None, None, None) == _lib.E_ARG        # prev_ids, no counter
    assert lib.abn_kmeans_assign(p, 10, 513, p, p, p, 2, None, p, None, None, None) == _lib.E_UNSUPPORTED
    assert b'abn_kmeans_max_d' in lib.abn_last_error()
    assert lib.abn_kmeans_assign(p, 10, 4, p, p, p, 4097, None, p, None, None, None) == _lib.E_UNSUPPORTED
    assert lib.abn_kmeans_accumulate(p, 10, 4, p, p, 2, None, 0, p, 1 << 20, None) == _lib.E_ARG
    assert lib.abn_kmeans_accumulate(p, 10, 4, p, p, 2, p, 0, p, 8, None) == _lib.E_WORKSPACE
    assert b'abn_kmeans_ws_bytes' in lib.abn_last_error()
    assert lib.abn_kmeans_accumulate(p, 10, 4, p, p, 2, p, 0, ctypes.c_void_p(0x10004), 1 << 20, None) == _lib.E_ARG
    assert lib.abn_kmeans_accumulate(p, 10, 4, p, p, 2, p, 1025, p, 1 << 20, None) == _lib.E_ARG
    assert lib.abn_kmeans_update(p, 1 << 20, p, 10, 2, 4, 0, 0, None, p, p, p, p, None) == _lib.E_ARG
    assert lib.abn_kmeans_update(p, 1 << 20, p, 10, 2, 4, 0, 0, p, p, None, p, p, None) == _lib.E_ARG   # mu, m, b go together
    assert lib.abn_kmeans_update(None, 0, p, 10, 2, 4, 0, 0, p, p, p, p, p, None) == _lib.E_WORKSPACE
