"""abnet3_amd/discovery.py without a GPU: segment enumeration, pair formation from given neighbour lists and the
written files read back through PairsDataLoader.load_pairs, against the brute-force restatement (tests/knn_np.py);
and the argument checks of abn_knn_topk / abn_segment_vectors, which answer before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_np  # noqa: E402


@pytest.mark.parametrize('lengths,shift', [((40, 60, 80), 5), ((40, 60), 5), ((7,), 1), ((10, 3), 4)])
def test_segment_enumeration(lengths, shift):
    from abnet3_amd.discovery import enumerate_segments
    n_frames = [0, 3, 39, 40, 41, 44, 45, 79, 80, 81, 200, 333]
    f, b, L = enumerate_segments(n_frames, lengths, shift)
    ref = knn_np.segments(n_frames, lengths, shift)
    assert list(zip(f.tolist(), b.tolist(), L.tolist())) == ref
    assert f.dtype == b.dtype == L.dtype == np.int32
    assert all(s + ln <= n_frames[fi] for fi, s, ln in ref)


def random_lists(rng, n, k, fill):
    """Neighbour lists like the kernel's: distinct j != i per row, sorted by descending similarity, a -1 / -inf tail."""
    idx = np.full((n, k), -1, dtype=np.int32)
    sim = np.full((n, k), -np.inf, dtype=np.float32)
    for i in range(n):
        m = int(rng.integers(0, k + 1)) if fill == 'ragged' else k
        js = rng.choice(np.delete(np.arange(n), i), size=min(m, n - 1), replace=False)
        s = np.sort(rng.uniform(-0.2, 1.0, len(js)).astype(np.float32))[::-1]
        idx[i, :len(js)], sim[i, :len(js)] = js, s
    return idx, sim


@pytest.mark.parametrize('mutual', [True, False])
@pytest.mark.parametrize('min_similarity,max_pairs', [(0.0, None), (0.5, None), (-1.0, 7), (0.0, 0)])
def test_pairs_from_lists(mutual, min_similarity, max_pairs):
    from abnet3_amd.discovery import pairs_from_lists
    rng = np.random.default_rng(5)
    for n, k, fill in ((30, 4, 'full'), (12, 10, 'full'), (40, 5, 'ragged'), (1, 3, 'ragged')):
        idx, sim = random_lists(rng, n, k, fill)
        sim[rng.random(sim.shape) < 0.2] = np.float32(0.75)          # exact ties: (a, b) decides
        sim = np.where(idx >= 0, sim, -np.inf).astype(np.float32)
        a, b, s = pairs_from_lists(idx, sim, min_similarity, mutual, max_pairs)
        ref = knn_np.pairs_from_lists(idx, sim, min_similarity, mutual, max_pairs)
        assert list(zip(a.tolist(), b.tolist(), s.tolist())) == ref
        assert (a < b).all()


def test_written_files_read_back(tmp_path):
    from abnet3_amd.dataloader import PairsDataLoader
    from abnet3_amd.discovery import enumerate_segments, pairs_from_lists, write_pairs
    rng = np.random.default_rng(2)
    names = ['spk_b', 'spk_a'.encode(), 'utt3']
    n_frames = [120, 95, 300]
    f, b, L = enumerate_segments(n_frames, (40, 60), 5)
    idx, sim = random_lists(rng, len(f), 6, 'full')
    a, c, s = pairs_from_lists(idx, sim, 0.0, False)
    pairs_path, map_path = write_pairs(str(tmp_path / 'out'), names, f, b, L, a, c, s)
    lines = open(pairs_path).read().splitlines()
    assert len(lines) == len(a) > 0
    for line, x, y, v in zip(lines, a, c, s):
        fields = line.split(' ')
        assert len(fields) == 7
        assert [int(t) for t in fields[:6]] == [f[x], f[y], b[x], b[x] + L[x], b[y], b[y] + L[y]]
        assert fields[6] == '%.11f' % (1.0 - float(v))
        assert int(fields[3]) <= n_frames[f[x]] and int(fields[5]) <= n_frames[f[y]]      # the end is exclusive
    assert open(map_path).read().splitlines() == ['0 spk_b', '1 spk_a', '2 utt3']
    dl = PairsDataLoader(pairs_path, None, map_path, ratio_split_train_test=0.5, split_method='files')
    dl.split_train_test = lambda pairs: (pairs, [])                  # every pair, in file order
    dl.load_pairs()
    name = ['spk_b', 'spk_a', 'utt3']
    assert dl.pairs['train'] == [[name[f[x]], b[x], b[x] + L[x], name[f[y]], b[y], b[y] + L[y]] for x, y in zip(a, c)]
    ids = PairsDataLoader(pairs_path, None, None)
    ids.load_pairs()
    assert ids.files <= {0, 1, 2}


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def test_knn_argument_checks(lib):
    """Refused before any launch (no GPU needed): the pointers below are never dereferenced."""
    from abnet3_amd import _lib
    p = ctypes.c_void_p(0x10000)
    call = lambda Q=p, nq=100, C=p, nc=100, d=400, k=10, idx=p, sim=p, ws=p, wsb=1 << 30: lib.abn_knn_topk(
        Q, nq, C, nc, d, None, None, k, idx, sim, ws, wsb, None)
    for k in (0, -1, 33, 1000):
        assert call(k=k) == _lib.E_UNSUPPORTED
        assert lib.abn_knn_ws_bytes(100, 100, k) == -1
    for d in (0, 2, 3, 5, 402, 4100, -4):
        assert call(d=d) == _lib.E_UNSUPPORTED
    assert b'd = -4' in lib.abn_last_error()
    for kw in (dict(Q=None), dict(C=None), dict(idx=None), dict(sim=None), dict(nq=0), dict(nc=0), dict(nq=-5),
               dict(Q=ctypes.c_void_p(0x10004))):
        assert call(**kw) == _lib.E_ARG, kw
    # a split needs its workspace
    need = lib.abn_knn_ws_bytes(100, 1000, 10)
    assert need == 100 * 8 * 10 * 8                                   # 8 candidate tiles, one range each
    assert call(nc=1000, ws=None, wsb=0) == _lib.E_WORKSPACE
    assert call(nc=1000, wsb=need - 1) == _lib.E_WORKSPACE
    assert lib.abn_knn_ws_bytes(100, 100, 10) == 0                    # one tile: nothing to merge


def test_knn_split_switch_sizes_the_workspace(lib, monkeypatch):
    monkeypatch.setenv('ABN_KNN_SPLIT', '1')
    assert lib.abn_knn_ws_bytes(5000, 5000, 10) == 0
    monkeypatch.setenv('ABN_KNN_SPLIT', '7')
    assert lib.abn_knn_ws_bytes(5000, 5000, 10) == 5000 * 7 * 10 * 8      # 40 tiles: 7 ranges of 6 (the last of 4)
    monkeypatch.setenv('ABN_KNN_SPLIT', 'auto')
    assert lib.abn_knn_ws_bytes(5000, 5000, 10) == 5000 * 10 * 10 * 8     # 40 query blocks -> 13 asked: 4 tiles each, 10 ranges


def test_segment_vectors_argument_checks(lib):
    from abnet3_amd import _lib
    p = ctypes.c_void_p(0x10000)
    call = lambda table=p, D=40, row0=p, ln=p, n=10, K=10, out=p, keep=p: lib.abn_segment_vectors(
        table, D, row0, ln, n, K, out, keep, None)
    for kw in (dict(D=0), dict(D=5000), dict(K=0), dict(K=2000), dict(D=4096, K=1024)):
        assert call(**kw) == _lib.E_UNSUPPORTED, kw
    for kw in (dict(table=None), dict(row0=None), dict(ln=None), dict(out=None), dict(keep=None), dict(n=-1)):
        assert call(**kw) == _lib.E_ARG, kw
    assert call(n=0) == 0                                             # nothing to do, nothing launched
