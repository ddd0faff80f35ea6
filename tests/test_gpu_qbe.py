"""Query-by-example search on the MI355X: abn_dtw_search_batched / abn_dtw_search_kl_batched against the numpy
restatement (tests/qbe_np.py) bit for bit -- result, bounds and the whole profile --, the refused, empty and blocked
cases, the scalar-load path, the grid-stride loop, and QbeSearcher end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abx_kl_np  # noqa: E402
import qbe_np  # noqa: E402

pytestmark = pytest.mark.gpu

U_EDGES = [1, 2, 63, 64, 65, 127, 128, 129, 200, 333]              # both sides of the band edges
Q_EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 128, 255, 256]            # the round, tile and cap edges


def dev(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def offsets(n):
    return np.concatenate(([0], np.cumsum(n)[:-1])).astype(np.int64)


def lengths(rng, P):
    """Utterance and query lengths of P pairs: every query edge against the utterance edges in two pairings, then small
    random pairs."""
    un = rng.integers(1, 201, P).astype(np.int32)
    qn = rng.integers(1, 81, P).astype(np.int32)
    k = len(Q_EDGES)
    qn[:k] = Q_EDGES
    un[:k] = (U_EDGES + U_EDGES[:1])[:k]
    qn[k:2 * k] = Q_EDGES[::-1]
    un[k:2 * k] = (U_EDGES + U_EDGES[4:5])[:k]
    return un, qn


def frames(rng, rows, D, quantised):
    if not quantised:
        return rng.standard_normal((rows, D)).astype(np.float32)
    f = rng.integers(-2, 3, (rows, D)).astype(np.float32)          # repeated frames: exact ties, |cos| rounded above 1
    f[1::2] = f[0:len(f) - 1:2]
    return f


def raw_search(tu, uo, un, tq, qo, qn, kl=False, profile=True):
    """The entry point alone over device tables (cosine: [rows, D] tensors; kl: (P, L, bad)), outputs prefilled so that
    what the kernel leaves alone shows: (cost, len, start, end, (prof cost, len, start))."""
    from abnet3_amd import _lib
    lib = _lib.load()
    P = len(un)
    tab = [dev(uo, np.int64), dev(un, np.int32), dev(qo, np.int64), dev(qn, np.int32)]
    cost = torch.full((P,), 7.0, dtype=torch.float64, device='cuda')
    plen, start, end = (torch.full((P,), 7, dtype=torch.int32, device='cuda') for _ in range(3))
    poff = np.concatenate(([0], np.cumsum(np.maximum(np.asarray(un, np.int64), 0))))
    rows = int(poff[-1])
    pc, pl, ps = dev(np.full(rows, np.nan)), dev(np.full(rows, -7, np.int32)), dev(np.full(rows, -7, np.int32))
    d_poff = dev(poff[:-1], np.int64)
    out = [_lib.ptr(cost), _lib.ptr(plen), _lib.ptr(start), _lib.ptr(end)]
    out += [_lib.ptr(d_poff), rows, _lib.ptr(pc), _lib.ptr(pl), _lib.ptr(ps)] if profile else [None, 0, None, None, None]
    out.append(_lib.stream())
    if kl:
        D = tu[0].shape[1]
        _lib.check(lib.abn_dtw_search_kl_batched(_lib.ptr(tu[0]), _lib.ptr(tu[1]), tu[0].shape[0], _lib.ptr(tq[0]), _lib.ptr(tq[1]),
                                                 tq[0].shape[0], *[_lib.ptr(x) for x in tab], P, D, _lib.ptr(tu[2]),
                                                 _lib.ptr(tq[2]), *out), 'abn_dtw_search_kl_batched')
    else:
        _lib.check(lib.abn_dtw_search_batched(_lib.ptr(tu), tu.shape[0], _lib.ptr(tq), tq.shape[0], *[_lib.ptr(x) for x in tab],
                                              P, tu.shape[1], *out), 'abn_dtw_search_batched')
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (cost, plen, start, end)) + (tuple(x.cpu().numpy() for x in (pc, pl, ps)),)


def assert_same(got, ref, what=''):
    """Cost as int64 bits; length, start, end; the whole profile (cost bits, length, start)."""
    for name, g, r in zip(('path_len', 'start', 'end'), got[1:4], ref[1:4]):
        assert np.array_equal(g, r), (what, name, np.flatnonzero(g != r)[:10])
    assert np.array_equal(got[0].view(np.int64), ref[0].view(np.int64)), (what, 'cost', np.flatnonzero(got[0] != ref[0])[:10])
    for name, g, r in zip(('profile len', 'profile start'), got[4][1:], ref[4][1:]):
        assert np.array_equal(g, r), (what, name, np.flatnonzero(g != r)[:10])
    gb, rb = got[4][0].view(np.int64), ref[4][0].view(np.int64)
    assert np.array_equal(gb, rb), (what, 'profile cost', np.flatnonzero(gb != rb)[:10])


@pytest.mark.parametrize('D', [1, 3, 40, 100, 257])
def test_search_kernel_matches_the_restatement(D):
    from abnet3_amd import _lib
    cap = _lib.load().abn_dtw_search_max_query()
    assert cap == qbe_np.CAP
    rng = np.random.default_rng(300 + D)
    for quantised in (False, True):
        un, qn = lengths(rng, 60)
        un[-1], un[-3] = 50, 40                                     # (room around the frames that get blocked)
        fu, fq = frames(rng, int(un.sum()), D, quantised), frames(rng, int(qn.sum()), D, quantised)
        uo, qo = offsets(un), offsets(qn)
        # blocked cells: a NaN frame inside an utterance (routed around), a NaN frame in a query (no detection), an
        # infinite frame, an all-zero frame on either side (distance 1: kept)
        fu[uo[-1] + un[-1] // 2] = np.nan
        fq[qo[-2] + qn[-2] // 2, D // 2] = np.nan
        # (that query's utterance gets no all-zero frame: the reference's zero-frame rule comes before the division, so
        # a zero frame is at distance 1 from a NaN frame too and would carry a path through the NaN query frame)
        fu[uo[-2] + np.flatnonzero(~fu[uo[-2]:uo[-2] + un[-2]].any(axis=1)), 0] = 1.0
        fu[uo[-3], 0] = np.inf
        fu[uo[-4] + un[-4] - 1] = 0.0
        fq[qo[-5]] = 0.0
        # empty sides; then the refused: a query of cap + 1 frames (its rows exist), offsets outside the tables, a
        # negative length
        un[-6] = 0
        qn[-7] = 0
        assert len(fq) >= cap + 1
        uo = np.concatenate([uo, [0, len(fu) - 3, 0, -1, 0]])
        un = np.concatenate([un, [4, 4, 5, 5, -2]]).astype(np.int32)
        qo = np.concatenate([qo, [0, 0, len(fq) - 2, 0, 0]])
        qn = np.concatenate([qn, [cap + 1, 5, 3, 5, 5]]).astype(np.int32)
        got = raw_search(dev(fu), uo, un, dev(fq), qo, qn)
        ref = qbe_np.search_cosine_batch(fq, qo, qn, fu, uo, un, cap=cap)
        assert_same(got, ref, 'quantised' if quantised else 'random')
        assert got[1][-5:].tolist() == [-1] * 5 and (got[0][-5:] == 0).all() and (got[2][-5:] == -1).all()
        assert got[1][-11] == 0 and got[1][-12] == 0 and got[3][-11] == -1                  # empty sides
        assert got[1][-7] == 0 and got[2][-7] == -1 and got[0][-7] == 0                     # the NaN query frame
        assert got[1][-6] >= qn[-6] and got[1][-8] >= qn[-8]                                # NaN / inf utterance frames
        if not quantised:
            keep = np.ones(len(un), bool)
            keep[[-12, -11, -7, -5, -4, -3, -2, -1]] = False
            assert (got[1][keep] >= qn[keep]).all() and (got[3][keep] >= got[2][keep]).all() and (got[2][keep] >= 0).all()
        # without the profile: the same results
        bare = raw_search(dev(fu), uo, un, dev(fq), qo, qn, profile=False)
        for g, b in zip(got[:4], bare[:4]):
            assert g.tobytes() == b.tobytes()
        assert np.isnan(bare[4][0]).all() and (bare[4][1] == -7).all()


def test_a_planted_query_is_found_at_cost_zero_with_exact_bounds():
    """Frames whose cosine with themselves rounds above 1 -- a NaN cell, for which ABX drops the pair: the search takes
    the cell as 0, so the query's own stretch costs exactly 0 with a diagonal path.  Fails on a kernel that keeps the
    drop rule."""
    from oracle import dtw_oracle as O
    rng = np.random.default_rng(8)
    pool = rng.integers(-3, 4, (1500, 7)).astype(np.float32)
    self_d = np.array([O.cosine_distance(f[None], f[None], check=False)[0][0, 0] for f in pool])
    keep = np.flatnonzero(np.isnan(self_d) | (self_d == 0))
    assert np.isnan(self_d[keep]).sum() >= 20
    fu = pool[keep[:230]]
    assert len(fu) == 230
    spans = [(0, 1), (5, 9), (60, 70), (100, 140), (200, 230), (63, 66)]
    for a, b in spans[2:]:
        assert np.isnan(self_d[keep[a:b]]).any()
    qo = np.array([a for a, _ in spans], np.int64)
    qn = np.array([b - a for a, b in spans], np.int32)
    uo, un = np.zeros(len(spans), np.int64), np.full(len(spans), 230, np.int32)
    got = raw_search(dev(fu), uo, un, dev(fu), qo, qn)
    assert_same(got, qbe_np.search_cosine_batch(fu, qo, qn, fu, uo, un))
    assert (got[0] == 0).all() and np.array_equal(got[1], qn)
    assert np.array_equal(got[2], qo) and np.array_equal(got[3], qo + qn - 1)


@pytest.mark.parametrize('D,how', [(40, 'one float in'), (39, 'one row in')])
def test_unaligned_tables_take_the_scalar_path(D, how):
    rng = np.random.default_rng(12)
    un, qn = rng.integers(1, 150, 40).astype(np.int32), rng.integers(1, 70, 40).astype(np.int32)
    fu, fq = frames(rng, int(un.sum()) + 1, D, False), frames(rng, int(qn.sum()) + 1, D, False)
    uo, qo = offsets(un), offsets(qn)
    if how == 'one float in':           # D % 4 == 0, the table 4 bytes past an aligned allocation
        tu = dev(np.concatenate([np.zeros(1, np.float32), fu.ravel()]))[1:].view(fu.shape)
        tq = dev(fq)
        ref = qbe_np.search_cosine_batch(fq, qo, qn, fu, uo, un)
    else:                               # odd D, views that start one row in
        tu, tq = dev(fu)[1:], dev(fq)[1:]
        ref = qbe_np.search_cosine_batch(fq[1:], qo, qn, fu[1:], uo, un)
    assert tu.data_ptr() % 16 != 0 and tu.is_contiguous()
    assert_same(raw_search(tu, uo, un, tq, qo, qn), ref)
    if how == 'one float in':
        assert_same(raw_search(dev(fu), uo, un, tq, qo, qn), ref)         # the vector loads: the same bits


def test_grid_stride_many_tiny_pairs():
    """More pairs than the grid has wavefronts: each wavefront works through several, its LDS state must not leak."""
    rng = np.random.default_rng(13)
    K = 300
    un, qn = rng.integers(1, 9, K).astype(np.int32), rng.integers(1, 5, K).astype(np.int32)
    fu, fq = frames(rng, int(un.sum()), 5, True), frames(rng, int(qn.sum()), 5, True)
    uo, qo = offsets(un), offsets(qn)
    fu[uo[7]] = np.nan
    fq[qo[9]] = np.nan
    ref = qbe_np.search_cosine_batch(fq, qo, qn, fu, uo, un)
    pick = rng.integers(0, K, 9000)
    assert len(pick) > 256 * 32
    got = raw_search(dev(fu), uo[pick], un[pick], dev(fq), qo[pick], qn[pick])
    for g, r in zip(got[:4], ref[:4]):
        assert g.tobytes() == r[pick].tobytes()
    poff = offsets(un[pick])
    for k in (0, 1, 4000, 8191, 8192, 8999):
        sl, rs = slice(poff[k], poff[k] + un[pick[k]]), slice(ref[5][pick[k]], ref[5][pick[k]] + un[pick[k]])
        for g, r in zip(got[4], ref[4]):
            assert g[sl].tobytes() == r[rs].tobytes()


@pytest.mark.parametrize('D', [3, 40, 100])
def test_kl_search_kernel_matches_the_restatement(D):
    from abnet3_amd.abx import kl_tables
    rng = np.random.default_rng(400 + D)
    un, qn = lengths(rng, 40)
    un[-1] = 50
    uo, qo = offsets(un), offsets(qn)
    fu = rng.dirichlet(np.full(D, 0.5), int(un.sum())).astype(np.float32)
    fq = rng.dirichlet(np.full(D, 0.5), int(qn.sum())).astype(np.float32)
    fq[qo[3]:qo[3] + qn[3]] = fu[uo[3] + 10:uo[3] + 10 + qn[3]]           # a query cut from its utterance (32 of its 64 frames)
    fu[uo[-1] + un[-1] // 2, 0] = -0.25                                  # a BAD row in an utterance ...
    fq[qo[-2], D // 2] = np.nan                                          # ... and in a query
    fu[uo[-3], 1] = 0.0                                                  # a zero is floored: kept
    un[-4] = 0
    uo, un = np.concatenate([uo, [-1]]), np.concatenate([un, [3]]).astype(np.int32)
    qo, qn = np.concatenate([qo, [0]]), np.concatenate([qn, [3]]).astype(np.int32)
    tu, tq = kl_tables(dev(fu)), kl_tables(dev(fq))
    host = lambda t: tuple(x.cpu().numpy() for x in t)
    got = raw_search(tu, uo, un, tq, qo, qn, kl=True)
    ref = qbe_np.search_kl_batch(host(tq), qo, qn, host(tu), uo, un)        # the device's own P and L
    assert_same(got, ref)
    assert (got[0][3], got[1][3], got[2][3], got[3][3]) == (0.0, qn[3], 10, 10 + qn[3] - 1)
    assert got[1][-1] == -1 and got[1][-5] == 0 and got[1][-3] == 0 and got[1][-2] >= qn[-2]
    assert np.isinf(got[4][0][offsets(un[:-1])[-1] + un[-2] // 2])


def test_python_surface_checks_and_profile():
    from abnet3_amd.abx import kl_tables
    from abnet3_amd.qbe import max_query, subsequence_dtw_batch
    cap = max_query()
    rng = np.random.default_rng(14)
    fu, fq = dev(frames(rng, 300, 24, False)), dev(frames(rng, cap + 1, 24, False))
    qo, qn, uo, un = [0, 1, 5], [cap, 7, 0], [0, 100, 0], [300, 40, 10]
    out = subsequence_dtw_batch(fq, qo, qn, fu, uo, un, profile=True)
    ref = qbe_np.search_cosine_batch(fq.cpu().numpy(), qo, qn, fu.cpu().numpy(), uo, un)
    assert out[0].dtype == torch.float64 and all(t.dtype == torch.int32 for t in out[1:4]) and out[0].is_cuda
    prof = out[4]
    assert prof.offset.tolist() == [0, 300, 340] and prof.cost.numel() == 350
    assert_same(tuple(t.cpu().numpy() for t in out[:4]) + (tuple(t.cpu().numpy() for t in prof[:3]),), ref)
    assert len(subsequence_dtw_batch(fq, qo, qn, fu, uo, un)) == 4
    with pytest.raises(ValueError, match=str(cap)):
        subsequence_dtw_batch(fq, [0], [cap + 1], fu, [0], [10])
    with pytest.raises(ValueError, match='outside'):
        subsequence_dtw_batch(fq, [0], [5], fu, [295], [10])
    with pytest.raises(ValueError, match='widths'):
        subsequence_dtw_batch(fq[:, :20].contiguous(), [0], [5], fu, [0], [10])
    with pytest.raises(ValueError, match='kl_tables'):
        subsequence_dtw_batch((fq, fq, fq), [0], [5], (fu, fu, fu), [0], [10], distance='kl')
    empty = subsequence_dtw_batch(fq, [], [], fu, [], [], profile=True)
    assert empty[0].numel() == 0 and empty[4].cost.numel() == 0
    t = kl_tables(dev(rng.dirichlet(np.ones(12), 60).astype(np.float32)))
    c, ln, s, e = subsequence_dtw_batch(t, [20], [6], t, [0], [60], distance='kl')
    assert (c.item(), ln.item(), s.item(), e.item()) == (0.0, 6, 20, 25)


@pytest.fixture(scope='module')
def planted():
    feats, times, queries, relevant, _ = qbe_np.planted_corpus()
    return feats, times, queries, relevant, qbe_np.search_corpus(feats, times, queries)


@pytest.mark.parametrize('chunk', [1 << 18, 5])
def test_searcher_end_to_end(planted, chunk):
    from abnet3_amd.qbe import QbeSearcher, mean_average_precision, precision_at_n
    feats, times, queries, relevant, (score, start, end) = planted
    res = QbeSearcher(feats, times, chunk_pairs=chunk).search(queries)
    assert res.utterances == list(feats) and res.queries == queries and res.score.shape == (3, 6)
    assert res.score.tobytes() == score.tobytes()
    assert np.array_equal(res.start_frame, start) and np.array_equal(res.end_frame, end)
    for q in range(3):
        for u, k in enumerate(feats):
            assert res.start_time[q, u] == times[k][start[q, u]] and res.end_time[q, u] == times[k][end[q, u]]
    assert mean_average_precision(res.score, relevant) == 1.0 and precision_at_n(res.score, relevant) == 1.0
    assert res.ranking(0)[0] == 0


def test_searcher_subsets_query_corpus_and_kl(planted):
    from abnet3_amd.dataloader import DeviceCorpus
    from abnet3_amd.qbe import QbeSearcher
    feats, times, queries, _relevant, (score, start, end) = planted
    corpus = DeviceCorpus(feats, times)
    s = QbeSearcher(corpus)
    sub = s.search(queries[1:], utterances=['utt4', 'utt1'])
    assert sub.score.tobytes() == score[1:][:, [4, 1]].tobytes() and np.array_equal(sub.end_frame, end[1:][:, [4, 1]])
    # queries from a corpus of their own; one that matches no frame: no detection, NaN times
    qfeats = {'q': feats['utt2'][10:].copy()}
    qtimes = {'q': np.arange(len(qfeats['q'])) * 0.01}
    own = s.search([('q', 0.045, 0.125), ('q', 5.0, 6.0)], query_corpus=qfeats, query_times=qtimes)
    ref = qbe_np.search(qbe_np.cosine_cells(feats['utt2'], qfeats['q'][5:13]))
    assert (own.score[0, 2], own.start_frame[0, 2], own.end_frame[0, 2]) == (ref[0] / ref[1], ref[2], ref[3])
    assert np.isinf(own.score[1]).all() and (own.start_frame[1] == -1).all() and np.isnan(own.start_time[1]).all()
    with pytest.raises(ValueError, match='frames'):
        s.search([('long', 0.0, 99.0)], query_corpus={'long': np.ones((300, 20), np.float32)}, query_times={'long': np.arange(300) * 0.01})
    # posteriorgrams: the KL route over the searcher's own tables
    post = {k: np.exp(v) / np.exp(v).sum(axis=1, keepdims=True) for k, v in feats.items()}
    post = {k: v.astype(np.float32) for k, v in post.items()}
    ks = QbeSearcher(post, times, distance='kl')
    kr = ks.search(queries)
    t = tuple(x.cpu().numpy() for x in ks.tables)
    for q, (f, on, off) in enumerate(queries):
        r, n = ks.corpus.token(f, on, off)
        for u, k in enumerate(post):
            o, ln = ks.corpus.offset[k], ks.corpus.length[k]
            c, pl, st, en, _ = qbe_np.search(qbe_np.kl_cells([a[o:o + ln] for a in t], [a[r:r + n] for a in t]))
            assert (kr.score[q, u], kr.start_frame[q, u], kr.end_frame[q, u]) == (c / pl, st, en)
    assert [int(kr.ranking(q)[0]) for q in range(3)] == [0, 1, 2] and (np.diag(kr.score) == 0).all()
