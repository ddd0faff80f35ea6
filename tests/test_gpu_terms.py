"""Term discovery on the MI355X: abn_dtw_local_batched / abn_dtw_local_kl_batched against the numpy restatement
(tests/terms_np.py) bit for bit -- score, length and the four bounds --, the refused, empty and blocked cases, the
exclusion band, the scalar-load path, the grid-stride loop, the Python surface, and TermDiscoverer end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import terms_np  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = terms_np.CAP
N1_EDGES = [1, 2, 63, 64, 65, 127, 128, 129, 200, 333]                     # both sides of the band edges
N2_EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 128, CAP - 1, CAP]               # the tile, round and cap edges
THETA = 0.5             # unrelated frames sit around 0.5 whatever D is: live paths everywhere; orthogonal quantised frames
                        # are at 0.5 exactly, similarity 0: ties with the dead cell


def dev(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def offsets(n):
    return np.concatenate(([0], np.cumsum(n)[:-1])).astype(np.int64)


def lengths(rng, P):
    """Side-1 and side-2 lengths of P pairs: every side-2 edge against the side-1 edges in two pairings, then small
    random pairs."""
    n1 = rng.integers(1, 201, P).astype(np.int32)
    n2 = rng.integers(1, 81, P).astype(np.int32)
    k = len(N2_EDGES)
    n2[:k] = N2_EDGES
    n1[:k] = (N1_EDGES + N1_EDGES[:1])[:k]
    n2[k:2 * k] = N2_EDGES[::-1]
    n1[k:2 * k] = (N1_EDGES + N1_EDGES[4:5])[:k]
    return n1, n2


def frames(rng, rows, D, quantised):
    if not quantised:
        return rng.standard_normal((rows, D)).astype(np.float32)
    f = rng.integers(-2, 3, (rows, D)).astype(np.float32)          # repeated frames: exact ties in H, |cos| rounded above 1
    f[1::2] = f[0:len(f) - 1:2]
    return f


def raw_local(t1, o1, n1, t2, o2, n2, theta, exclude=0, kl=False):
    """The entry point alone over device tables (cosine: [rows, D] tensors; kl: (P, L, bad)), outputs prefilled so that
    what the kernel leaves alone shows: (score, len, start1, start2, end1, end2)."""
    from abnet3_amd import _lib
    lib = _lib.load()
    P = len(n1)
    tab = [dev(o1, np.int64), dev(n1, np.int32), dev(o2, np.int64), dev(n2, np.int32)]
    score = torch.full((P,), 7.0, dtype=torch.float64, device='cuda')
    ints = [torch.full((P,), 7, dtype=torch.int32, device='cuda') for _ in range(5)]
    out = [float(np.float32(theta)), int(exclude), _lib.ptr(score)] + [_lib.ptr(x) for x in ints] + [_lib.stream()]
    if kl:
        D = t1[0].shape[1]
        _lib.check(lib.abn_dtw_local_kl_batched(_lib.ptr(t1[0]), _lib.ptr(t1[1]), t1[0].shape[0], _lib.ptr(t2[0]), _lib.ptr(t2[1]),
                                                t2[0].shape[0], *[_lib.ptr(x) for x in tab], P, D, _lib.ptr(t1[2]),
                                                _lib.ptr(t2[2]), *out), 'abn_dtw_local_kl_batched')
    else:
        _lib.check(lib.abn_dtw_local_batched(_lib.ptr(t1), t1.shape[0], _lib.ptr(t2), t2.shape[0], *[_lib.ptr(x) for x in tab],
                                             P, t1.shape[1], *out), 'abn_dtw_local_batched')
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in [score] + ints)


NAMES = ('score', 'path_len', 'start1', 'start2', 'end1', 'end2')


def assert_same(got, ref, what=''):
    """Length and the four bounds; the score as int64 bits."""
    for name, g, r in zip(NAMES[1:], got[1:], ref[1:]):
        assert np.array_equal(g, r), (what, name, np.flatnonzero(g != r)[:10], g[g != r][:10], r[g != r][:10])
    gb, rb = got[0].view(np.int64), ref[0].view(np.int64)
    assert np.array_equal(gb, rb), (what, 'score', np.flatnonzero(gb != rb)[:10])


@pytest.mark.parametrize('D', [1, 3, 40, 100, 257])
def test_local_kernel_matches_the_restatement(D):
    from abnet3_amd import _lib
    assert _lib.load().abn_dtw_local_max_n2() == CAP
    rng = np.random.default_rng(500 + D)
    for quantised in (False, True):
        n1, n2 = lengths(rng, 60)
        n1[-1], n1[-3] = 50, 40                                     # (room around the frames that get blocked)
        f1, f2 = frames(rng, int(n1.sum()), D, quantised), frames(rng, int(n2.sum()), D, quantised)
        o1, o2 = offsets(n1), offsets(n2)
        # blocked cells: a NaN frame and an infinite frame on side 1, a NaN frame on side 2, an all-zero frame on either side
        f1[o1[-1] + n1[-1] // 2] = np.nan
        f2[o2[-2] + n2[-2] // 2, D // 2] = np.nan
        f1[o1[-3], 0] = np.inf
        f1[o1[-4] + n1[-4] - 1] = 0.0
        f2[o2[-5]] = 0.0
        # empty sides; then the refused: a side 2 of cap + 1 frames (its rows exist), offsets outside either table, a
        # negative length
        n1[-6] = 0
        n2[-7] = 0
        assert len(f2) >= CAP + 1
        o1 = np.concatenate([o1, [0, len(f1) - 3, 0, -1, 0]])
        n1 = np.concatenate([n1, [4, 4, 5, 5, -2]]).astype(np.int32)
        o2 = np.concatenate([o2, [0, 0, len(f2) - 2, 0, 0]])
        n2 = np.concatenate([n2, [CAP + 1, 5, 3, 5, 5]]).astype(np.int32)
        got = raw_local(dev(f1), o1, n1, dev(f2), o2, n2, THETA)
        ref = terms_np.local_cosine_batch(f1, o1, n1, f2, o2, n2, THETA)
        assert_same(got, ref, 'quantised' if quantised else 'random')
        assert got[1][-5:].tolist() == [-1] * 5 and (got[0][-5:] == 0).all()               # refused: -1, 0 and the bounds -1
        assert all((g[-5:] == -1).all() for g in got[2:])
        assert got[1][-11] == 0 and got[1][-12] == 0 and got[5][-11] == -1 and got[0][-12] == 0     # empty sides
        live = got[1] > 0
        assert live.sum() >= 40
        assert (got[0][live] > 0).all() and (got[4][live] >= got[2][live]).all() and (got[5][live] >= got[3][live]).all()
        span1, span2 = got[4][live] - got[2][live] + 1, got[5][live] - got[3][live] + 1
        assert (np.maximum(span1, span2) <= got[1][live]).all() and (got[1][live] <= span1 + span2 - 1).all()


@pytest.mark.parametrize('n', [64, 65, 200])
def test_exclusion_on_self_pairs(n):
    rng = np.random.default_rng(600 + n)
    D = 40
    f = frames(rng, 3 * n + 20, D, False)
    f[n + 5:n + 5 + n // 4] = f[n + 5 + n // 2:n + 5 + n // 2 + n // 4]          # a repeat inside the second utterance
    o = np.array([0, n + 5, 2 * n + 9], np.int64)
    ln = np.full(3, n, np.int32)
    t = dev(f)
    got0 = raw_local(t, o, ln, t, o, ln, 0.05)
    assert_same(got0, terms_np.local_cosine_batch(f, o, ln, f, o, ln, 0.05))
    # without the exclusion the self-match is the whole diagonal
    assert got0[1].tolist() == [n] * 3 and got0[2].tolist() == [0] * 3 and got0[3].tolist() == [0] * 3
    assert got0[4].tolist() == [n - 1] * 3 and got0[5].tolist() == [n - 1] * 3
    for exclude in (1, 10, 64):
        for theta in (0.05, THETA):
            got = raw_local(t, o, ln, t, o, ln, theta, exclude=exclude)
            assert_same(got, terms_np.local_cosine_batch(f, o, ln, f, o, ln, theta, exclude=exclude), (exclude, theta))
            on_diagonal = (got[1] > 0) & (np.abs(got[4] - got[5]) < exclude)
            assert not on_diagonal.any()
    # the repeat inside the second utterance comes out instead, the image with the smaller end row
    got = raw_local(t, o, ln, t, o, ln, 0.05, exclude=10)
    assert (got[1][1], got[2][1], got[3][1], got[4][1], got[5][1]) == (n // 4, 0, n // 2, n // 4 - 1, n // 2 + n // 4 - 1)
    # a window of the same utterance as side 2: the band follows the table rows
    o2, l2 = o + 7, ln - 7
    got = raw_local(t, o, ln, t, o2, l2, THETA, exclude=10)
    assert_same(got, terms_np.local_cosine_batch(f, o, ln, f, o2, l2, THETA, exclude=10), 'window')


def test_a_planted_copy_crossing_a_band_edge():
    """Rows 60..70 of a 130-frame side 1 (the band edge at 64) against columns 58..68 of side 2 (the round edge at
    diagonal 128 = 64 + 64 lies inside it): exact bounds, the restatement's bits."""
    rng = np.random.default_rng(21)
    D = 40
    x, y = frames(rng, 130, D, False), frames(rng, 100, D, False)
    y[58:69] = x[60:71]
    got = raw_local(dev(x), [0], np.int32([130]), dev(y), [0], np.int32([100]), 0.05)
    ref = terms_np.local_cosine_batch(x, [0], [130], y, [0], [100], 0.05)
    assert_same(got, ref)
    assert [int(g[0]) for g in got[1:]] == [11, 60, 58, 70, 68]
    assert 10.9 * 0.05 < got[0][0] <= 11 * np.float64(np.float32(0.05))


@pytest.mark.parametrize('D,how', [(40, 'one float in'), (39, 'one row in')])
def test_unaligned_tables_take_the_scalar_path(D, how):
    rng = np.random.default_rng(22)
    n1, n2 = rng.integers(1, 150, 40).astype(np.int32), rng.integers(1, 70, 40).astype(np.int32)
    f1, f2 = frames(rng, int(n1.sum()) + 1, D, False), frames(rng, int(n2.sum()) + 1, D, False)
    o1, o2 = offsets(n1), offsets(n2)
    if how == 'one float in':           # D % 4 == 0, the table 4 bytes past an aligned allocation
        t1 = dev(np.concatenate([np.zeros(1, np.float32), f1.ravel()]))[1:].view(f1.shape)
        t2 = dev(f2)
        ref = terms_np.local_cosine_batch(f1, o1, n1, f2, o2, n2, THETA)
    else:                               # odd D, views that start one row in
        t1, t2 = dev(f1)[1:], dev(f2)[1:]
        ref = terms_np.local_cosine_batch(f1[1:], o1, n1, f2[1:], o2, n2, THETA)
    assert t1.data_ptr() % 16 != 0 and t1.is_contiguous()
    assert_same(raw_local(t1, o1, n1, t2, o2, n2, THETA), ref)
    if how == 'one float in':
        assert_same(raw_local(dev(f1), o1, n1, t2, o2, n2, THETA), ref)         # the vector loads: the same bits


def test_grid_stride_many_tiny_pairs():
    """More pairs than the grid has wavefronts: each wavefront works through several, its LDS state must not leak."""
    rng = np.random.default_rng(23)
    K = 300
    n1, n2 = rng.integers(1, 9, K).astype(np.int32), rng.integers(1, 5, K).astype(np.int32)
    f1, f2 = frames(rng, int(n1.sum()), 5, True), frames(rng, int(n2.sum()), 5, True)
    o1, o2 = offsets(n1), offsets(n2)
    f1[o1[7]] = np.nan
    f2[o2[9]] = np.nan
    ref = terms_np.local_cosine_batch(f1, o1, n1, f2, o2, n2, THETA)
    assert (ref[1] > 0).sum() > 100 and (ref[1] == 0).sum() > 5
    pick = rng.integers(0, K, 9000)
    assert len(pick) > 256 * 32
    got = raw_local(dev(f1), o1[pick], n1[pick], dev(f2), o2[pick], n2[pick], THETA)
    for g, r in zip(got, ref):
        assert g.tobytes() == r[pick].tobytes()


@pytest.mark.parametrize('D', [3, 40, 100])
def test_kl_local_kernel_matches_the_restatement(D):
    from abnet3_amd.abx import kl_tables
    rng = np.random.default_rng(700 + D)
    n1, n2 = lengths(rng, 40)
    n1[-1] = 50
    o1, o2 = offsets(n1), offsets(n2)
    f1 = rng.dirichlet(np.full(D, 0.5), int(n1.sum())).astype(np.float32)
    f2 = rng.dirichlet(np.full(D, 0.5), int(n2.sum())).astype(np.float32)
    f2[o2[3] + 5:o2[3] + 25] = f1[o1[3] + 10:o1[3] + 30]                  # a planted copy (pair 3: 64 x 32 frames)
    f1[o1[-1] + n1[-1] // 2, 0] = -0.25                                  # a BAD row on side 1 ...
    f2[o2[-2], D // 2] = np.nan                                          # ... and on side 2
    f1[o1[-3], 1] = 0.0                                                  # a zero is floored: kept
    n1[-4] = 0
    o1, n1 = np.concatenate([o1, [-1]]), np.concatenate([n1, [3]]).astype(np.int32)
    o2, n2 = np.concatenate([o2, [0]]), np.concatenate([n2, [3]]).astype(np.int32)
    t1, t2 = kl_tables(dev(f1)), kl_tables(dev(f2))
    host = lambda t: tuple(x.cpu().numpy() for x in t)
    # the Dirichlet rows' mutual KL distances: theta at their lower quartile keeps live paths everywhere
    theta = float(np.quantile(terms_np.kl_cells([a[:200] for a in host(t1)], [a[:200] for a in host(t2)]), 0.25))
    got = raw_local(t1, o1, n1, t2, o2, n2, theta, kl=True)
    ref = terms_np.local_kl_batch(host(t1), o1, n1, host(t2), o2, n2, theta)          # the device's own P and L
    assert_same(got, ref)
    assert got[1][-1] == -1 and got[1][-5] == 0 and (got[1] > 0).sum() >= 30
    # the planted copy at mean distance 0, under a theta nothing else pays for
    small = 1e-5
    got = raw_local(t1, o1[3:4], n1[3:4], t2, o2[3:4], n2[3:4], small, kl=True)
    assert_same(got, terms_np.local_kl_batch(host(t1), o1[3:4], n1[3:4], host(t2), o2[3:4], n2[3:4], small))
    assert [int(g[0]) for g in got[1:]] == [20, 10, 5, 29, 24]
    assert got[0][0] == 20 * np.float64(np.float32(small))


def test_python_surface_checks():
    from abnet3_amd.abx import kl_tables
    from abnet3_amd.terms import local_dtw_batch, max_n2
    cap = max_n2()
    assert cap == CAP
    rng = np.random.default_rng(24)
    x, y = dev(frames(rng, 300, 24, False)), dev(frames(rng, cap + 1, 24, False))
    xo, xn, yo, yn = [0, 100, 0], [300, 40, 10], [0, 1, 5], [cap, 7, 0]
    out = local_dtw_batch(x, xo, xn, y, yo, yn, THETA)
    ref = terms_np.local_cosine_batch(x.cpu().numpy(), xo, xn, y.cpu().numpy(), yo, yn, THETA)
    assert len(out) == 6 and out[0].dtype == torch.float64 and all(t.dtype == torch.int32 for t in out[1:])
    assert all(t.is_cuda and t.shape == (3,) for t in out)
    assert_same(tuple(t.cpu().numpy() for t in out), ref)
    with pytest.raises(ValueError, match=str(cap)):
        local_dtw_batch(x, [0], [10], y, [0], [cap + 1], THETA)
    with pytest.raises(ValueError, match='outside'):
        local_dtw_batch(x, [295], [10], y, [0], [5], THETA)
    with pytest.raises(ValueError, match='widths'):
        local_dtw_batch(x, [0], [10], y[:, :20].contiguous(), [0], [5], THETA)
    with pytest.raises(ValueError, match='float32'):
        local_dtw_batch(x.double(), [0], [10], y, [0], [5], THETA)
    with pytest.raises(ValueError, match='same table'):
        local_dtw_batch(x, [0], [10], y, [0], [5], THETA, exclude=3)
    with pytest.raises(ValueError, match='same table'):
        local_dtw_batch(x, [0], [10], x.clone(), [0], [5], THETA, exclude=3)
    with pytest.raises(ValueError, match='theta'):
        local_dtw_batch(x, [0], [10], y, [0], [5], float('inf'))
    with pytest.raises(ValueError, match='kl_tables'):
        local_dtw_batch((x, x, x), [0], [10], (y, y, y), [0], [5], THETA, distance='kl')
    empty = local_dtw_batch(x, [], [], y, [], [], THETA)
    assert len(empty) == 6 and all(t.numel() == 0 for t in empty)
    same = local_dtw_batch(x, [0], [300], x, [0], [300], 0.05, exclude=5)
    assert same[1].item() == 0 or abs(same[4].item() - same[5].item()) >= 5
    post = rng.dirichlet(np.ones(12), 60).astype(np.float32)
    post[40:46] = post[20:26]
    t = kl_tables(dev(post))
    sc, ln, s1, s2, e1, e2 = local_dtw_batch(t, [0], [60], t, [0], [60], 1e-4, exclude=6, distance='kl')
    assert (sc.item(), ln.item(), s1.item(), s2.item(), e1.item(), e2.item()) == (6 * np.float64(np.float32(1e-4)), 6, 20, 40, 25, 45)
    with pytest.raises(ValueError, match='same table'):
        local_dtw_batch(t, [0], [60], kl_tables(dev(post)), [0], [60], 1e-4, exclude=6, distance='kl')


@pytest.fixture(scope='module')
def planted():
    feats, times, words = terms_np.planted_corpus()
    names = sorted(feats)
    return feats, times, words, names, terms_np.discover(names, feats, 0.05)


def written(td, out_dir):
    return [open(p, 'rb').read() for p in td.write(str(out_dir))]


def test_discoverer_end_to_end(planted, tmp_path):
    from abnet3_amd.sampler import SamplerClusterSiamese
    from abnet3_amd.terms import TermDiscoverer
    feats, times, words, names, (matches, clusters) = planted
    td = TermDiscoverer(feats, times, theta=0.05)
    got_m, got_c = td.discover()
    assert td.names == names and max(len(v) for v in feats.values()) > td.window == CAP
    assert [tuple(m)[:6] + (m.path_len,) for m in got_m] == [m[:6] + (m[7],) for m in matches]
    assert np.array([m.score for m in got_m]).tobytes() == np.array([m[6] for m in matches]).tobytes()
    assert np.array([m.distance for m in got_m]).tobytes() == np.array([m[8] for m in matches]).tobytes()
    assert got_c == clusters
    # every planted word is one cluster holding all its occurrences, with exact bounds
    assert got_c == sorted(sorted((names.index(k), lo, hi) for k, lo, hi in occ) for occ in words.values())
    files = written(td, tmp_path / 'a')
    assert files[0].decode() == terms_np.classes_text(names, times, clusters)
    assert files[1].decode() == terms_np.pairs_text(matches) and files[2].decode() == terms_np.map_text(names)
    assert written(TermDiscoverer(feats, times, theta=0.05, chunk_pairs=5), tmp_path / 'b') == files
    parsed = SamplerClusterSiamese().parse_input_file(str(tmp_path / 'a' / 'terms.classes'))
    assert [[(f, names[g]) for (f, _on, _off), (g, _lo, _hi) in zip(c, want)] for c, want in zip(parsed, clusters)] == \
        [[(names[g], names[g]) for g, _lo, _hi in want] for want in clusters]
    for c, want in zip(parsed, clusters):
        for (f, on, off), (g, lo, hi) in zip(c, want):
            assert td.corpus.token(f, on, off) == (td.corpus.offset[names[g]] + lo, hi - lo + 1)
    # a given pair list: side 1 whole, side 2 windowed
    m2, _ = TermDiscoverer(feats, times, theta=0.05).discover(pairs=[('utt1', 'utt2'), ('utt4', 'utt3')])
    ref2, _ = terms_np.discover(names, feats, 0.05, pairs=[(1, 2), (4, 3)])
    assert [tuple(m) for m in m2] == ref2 and len(m2) == 2


def test_discoverer_over_posteriorgrams(planted, tmp_path):
    from abnet3_amd.terms import TermDiscoverer
    feats, times, words, names, _ = planted
    post = {}
    for k, v in feats.items():                                      # a row softmax: copies stay copies
        e = np.exp(v - v.max(axis=1, keepdims=True))
        post[k] = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    td = TermDiscoverer(post, times, distance='kl', theta=0.05)
    got_m, got_c = td.discover()
    t = tuple(x.cpu().numpy() for x in td.tables)
    tables = {k: [a[td.corpus.offset[k]:td.corpus.offset[k] + td.corpus.length[k]] for a in t] for k in names}
    matches, clusters = terms_np.discover(names, post, 0.05, cells='kl', tables=tables)
    assert [tuple(m) for m in got_m] == matches and got_c == clusters
    assert got_c == sorted(sorted((names.index(k), lo, hi) for k, lo, hi in occ) for occ in words.values())
    assert all(m.distance == 0.0 for m in got_m)
    files = written(td, tmp_path / 'kl')
    assert files[0].decode() == terms_np.classes_text(names, times, clusters) and files[1].decode() == terms_np.pairs_text(matches)
    assert written(TermDiscoverer(post, times, distance='kl', theta=0.05, chunk_pairs=5), tmp_path / 'kl5') == files
