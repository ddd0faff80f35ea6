"""ABX over the symmetrised Kullback-Leibler frame distance on the MI355X: abn_kl_tables and abn_dtw_cost_kl_batched
against the numpy restatement (tests/abx_kl_np.py), ABXEvaluator(distance='kl') end to end, and the seam from a
softmax network's embed_table to the evaluator."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abx_kl_np  # noqa: E402
from test_gpu_abx import EDGES, GRID, assert_a_drop_does_not_leak, synthetic_set  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def host(t):
    return tuple(x.cpu().numpy() for x in t)


def softmax_rows(z):
    z = z.astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def posteriorgrams(feats, scale):
    return {k: softmax_rows(np.float32(scale) * v) for k, v in feats.items()}


def test_tables_match_the_restatement():
    from abnet3_amd.abx import kl_tables
    rng = np.random.default_rng(1)
    x = np.concatenate([softmax_rows(rng.standard_normal((3000, 100))),
                        softmax_rows(20.0 * rng.standard_normal((3000, 100))),       # saturated: zeros and near-ones
                        rng.random((2000, 100)).astype(np.float32)])                 # (rows need not sum to one)
    x[10, 5] = 0.0
    x[11, 7] = 5e-7                                                                   # floor / 2
    x[12, 3] = np.nan
    x[13, 99] = np.inf
    x[14, 0] = -1e-3
    x[15, 64] = -np.inf
    P, L, bad = host(kl_tables(dev(x), floor=1e-6))
    rP, rL, rbad = abx_kl_np.tables(x, floor=1e-6)
    assert bad.dtype == np.uint8 and np.array_equal(bad.astype(bool), rbad)
    assert np.flatnonzero(bad).tolist() == [12, 13, 14, 15]
    ok = ~rbad
    assert np.array_equal(P[ok].view(np.int32), rP[ok].view(np.int32))
    assert P[10, 5] == np.float32(1e-6) and P[11, 7] == np.float32(1e-6)
    # the device's double log need not be correctly rounded: an entry may land on the other side of a float32
    # rounding boundary, never further, and only in a share of at most 1e-4 of the entries
    du = np.abs(L[ok].view(np.int32).astype(np.int64) - rL[ok].view(np.int32).astype(np.int64))
    print('L: %d of %d entries differ, max %d unit(s)' % ((du != 0).sum(), du.size, du.max()))
    assert du.max() <= 1
    assert (du != 0).mean() <= 1e-4
    # another floor; a table with a frame width that is no multiple of the wavefront
    y = x[:500, :37].copy()
    P2, L2, bad2 = host(kl_tables(dev(y), floor=1e-3))
    rP2, rL2, rbad2 = abx_kl_np.tables(y, floor=1e-3)
    assert np.array_equal(bad2.astype(bool), rbad2)
    assert np.array_equal(P2[~rbad2].view(np.int32), rP2[~rbad2].view(np.int32))
    assert np.abs(L2[~rbad2].view(np.int32).astype(np.int64) - rL2[~rbad2].view(np.int32).astype(np.int64)).max() <= 1
    with pytest.raises(ValueError):
        kl_tables(dev(y), floor=0.0)


def kl_pair_table(rng, P, D, quantised, lo=1, hi=200):
    """test_gpu_abx.pair_table for probability rows."""
    n1 = rng.integers(lo, hi + 1, P).astype(np.int32)
    n2 = rng.integers(lo, hi + 1, P).astype(np.int32)
    if hi >= 200:                       # both sides of every band / round edge
        k = len(EDGES)
        n1[:k] = EDGES
        n2[:k] = EDGES[::-1]
        n1[k:2 * k] = EDGES
        n2[k:2 * k] = EDGES
    r1, r2 = int(n1.sum()), int(n2.sum())
    if quantised:      # few distinct frames, with exact zeros, repeated: many exact ties and many d == 0
        protos = softmax_rows(4.0 * rng.integers(-2, 3, (5, D)))
        protos[:, ::3] = 0.0
        f1 = protos[rng.integers(0, 5, r1)]
        f2 = protos[rng.integers(0, 5, r2)]
        f1[1::2] = f1[0:len(f1) - 1:2]
        f2[2::3] = f2[1:len(f2) - 1:3][:len(f2[2::3])]
    else:
        f1 = softmax_rows(2.0 * rng.standard_normal((r1, D)))
        f2 = softmax_rows(2.0 * rng.standard_normal((r2, D)))
    o1 = np.concatenate(([0], np.cumsum(n1)[:-1])).astype(np.int64)
    o2 = np.concatenate(([0], np.cumsum(n2)[:-1])).astype(np.int64)
    return f1, o1, n1, f2, o2, n2


def raw_kl_cost(t1, o1, n1, t2, o2, n2):
    """abn_dtw_cost_kl_batched alone on device tables t = (P, L, bad)."""
    from abnet3_amd import _lib
    lib = _lib.load()
    tab = [dev(o1, np.int64), dev(n1, np.int32), dev(o2, np.int64), dev(n2, np.int32)]
    P = len(n1)
    cost = torch.full((P,), 7.0, dtype=torch.float64, device='cuda')
    plen = torch.full((P,), 7, dtype=torch.int32, device='cuda')
    _lib.check(lib.abn_dtw_cost_kl_batched(_lib.ptr(t1[0]), _lib.ptr(t1[1]), t1[0].shape[0], _lib.ptr(t2[0]), _lib.ptr(t2[1]),
                                           t2[0].shape[0], *[_lib.ptr(x) for x in tab], P, t1[0].shape[1], _lib.ptr(t1[2]),
                                           _lib.ptr(t2[2]), _lib.ptr(cost), _lib.ptr(plen), _lib.stream()),
               'abn_dtw_cost_kl_batched')
    return cost.cpu().numpy(), plen.cpu().numpy()


@pytest.mark.parametrize('D', [1, 3, 39, 40, 100, 128, 257])
def test_kl_cost_kernel_matches_the_restatement(D):
    from abnet3_amd import _lib
    from abnet3_amd.abx import kl_tables
    cap = _lib.load().abn_dtw_cost_max_n2()
    rng = np.random.default_rng(200 + D)
    for quantised in (False, True):
        f1, o1, n1, f2, o2, n2 = kl_pair_table(rng, 120 if D <= 128 else 60, D, quantised)
        # an empty token on either side; a BAD row (its pair is dropped); a zero entry (floored: kept)
        n1[-1] = 0
        n2[-2] = 0
        f1[o1[-3] + n1[-3] // 2, D // 2] = np.nan
        f2[o2[-4], 0] = -0.5
        f1[o1[-5] + n1[-5] - 1, 0] = 0.0
        t1, t2 = kl_tables(dev(f1)), kl_tables(dev(f2))
        # a pair beyond the cap (its rows exist) and two pairs outside the tables: refused
        o1 = np.concatenate([o1, [0, len(f1) - 3, 0]])
        n1 = np.concatenate([n1, [4, 4, 5]]).astype(np.int32)
        o2 = np.concatenate([o2, [0, 0, -1]])
        n2 = np.concatenate([n2, [cap + 1, 5, 5]]).astype(np.int32)
        assert len(f2) >= cap + 1
        got_c, got_l = raw_kl_cost(t1, o1, n1, t2, o2, n2)
        ref_c, ref_l = abx_kl_np.dtw_cost_batch(host(t1), o1, n1, host(t2), o2, n2, cap=cap)     # the device's own P and L
        assert np.array_equal(got_l, ref_l), np.flatnonzero(got_l != ref_l)[:10]
        assert np.array_equal(got_c.view(np.int64), ref_c.view(np.int64)), np.flatnonzero(got_c != ref_c)[:10]
        assert got_l[-3:].tolist() == [-1, -1, -1] and (got_c[-3:] == 0).all()           # refused
        assert got_l[-7:-3].tolist() == [0, 0, 0, 0] and (got_c[-7:-3] == 0).all()         # BAD rows, empty tokens
        assert (got_l[:-7] > 0).all() and (got_c >= 0).all()


def test_kl_cost_kernel_identical_tokens_cost_exactly_zero():
    from abnet3_amd.abx import kl_tables
    rng = np.random.default_rng(5)
    f1, o1, n1, _f2, _o2, _n2 = kl_pair_table(rng, 60, 40, False, lo=1, hi=90)
    t = kl_tables(dev(f1))
    c, ln = raw_kl_cost(t, o1, n1, t, o1, n1)
    assert (c == 0).all() and np.array_equal(ln, n1)                  # the diagonal, by the tie-break


def test_kl_cost_kernel_unaligned_tables_take_the_scalar_path():
    """D % 4 == 0 but tables that are not 16-byte aligned: the scalar loads, the same bits."""
    from abnet3_amd.abx import kl_tables
    rng = np.random.default_rng(3)
    f1, o1, n1, f2, o2, n2 = kl_pair_table(rng, 100, 40, False, lo=1, hi=90)
    t1, t2 = kl_tables(dev(f1)), kl_tables(dev(f2))
    shifted = []
    for which, t in enumerate(t1[:2]):          # P 4 bytes, L 8 bytes past an aligned allocation
        base = torch.cat([torch.zeros(which + 1, device='cuda'), t.reshape(-1)])
        shifted.append(base[which + 1:].view(t.shape))
        assert shifted[-1].data_ptr() % 16 != 0
    got_c, got_l = raw_kl_cost((shifted[0], shifted[1], t1[2]), o1, n1, t2, o2, n2)
    al_c, al_l = raw_kl_cost(t1, o1, n1, t2, o2, n2)
    ref_c, ref_l = abx_kl_np.dtw_cost_batch(host(t1), o1, n1, host(t2), o2, n2)
    assert np.array_equal(got_l, ref_l) and np.array_equal(al_l, ref_l)
    assert np.array_equal(got_c.view(np.int64), ref_c.view(np.int64))
    assert np.array_equal(al_c.view(np.int64), ref_c.view(np.int64))


def test_kl_cost_kernel_grid_stride_many_tiny_pairs():
    """More pairs than the grid has wavefronts: each wavefront works through several; a pair dropped for a BAD row
    must not take the next one with it."""
    from abnet3_amd.abx import kl_tables
    rng = np.random.default_rng(13)
    f1, o1, n1, f2, o2, n2 = kl_pair_table(rng, 300, 5, True, lo=1, hi=8)
    f1[o1[7], 0] = -0.25                                             # a BAD row: this pair is dropped
    t1, t2 = kl_tables(dev(f1)), kl_tables(dev(f2))
    ref_c, ref_l = abx_kl_np.dtw_cost_batch(host(t1), o1, n1, host(t2), o2, n2)      # the device's own P and L
    assert ref_l[7] == 0 and (np.delete(ref_l, 7) > 0).all()
    pick = rng.integers(0, 300, 9000)
    assert len(pick) > GRID
    got_c, got_l = raw_kl_cost(t1, o1[pick], n1[pick], t2, o2[pick], n2[pick])
    assert np.array_equal(got_l, ref_l[pick]), np.flatnonzero(got_l != ref_l[pick])[:10]
    assert np.array_equal(got_c.view(np.int64), ref_c[pick].view(np.int64)), np.flatnonzero(got_c != ref_c[pick])[:10]
    assert_a_drop_does_not_leak(pick, 7, ref_l, got_l)


def test_kl_cost_beyond_the_cap_raises():
    from abnet3_amd import _lib
    from abnet3_amd.abx import dtw_cost_batch, kl_tables
    cap = _lib.load().abn_dtw_cost_max_n2()
    rng = np.random.default_rng(7)
    t1 = kl_tables(dev(softmax_rows(rng.standard_normal((30, 24)))))
    t2 = kl_tables(dev(softmax_rows(rng.standard_normal((cap + 1, 24)))))
    c, ln = dtw_cost_batch(t1, [0, 5], [20, 25], t2, [0, 1], [cap, cap], distance='kl')      # the cap itself is fine
    assert (ln.cpu().numpy() > 0).all()
    with pytest.raises(ValueError, match=str(cap)):
        dtw_cost_batch(t1, [0, 5], [20, 25], t2, [0, 0], [cap, cap + 1], distance='kl')


def restatement_error(ev, items, mode):
    """The restatement's ABX error over the evaluator's own device tables and tokens."""
    P, L, bad = host(ev.tables)
    assert not bad.any()
    tok = [(P[r:r + n], L[r:r + n]) for r, n in zip(ev.row, ev.n)]
    return abx_kl_np.abx_error(items, tok, mode)


@pytest.mark.parametrize('mode', ['within', 'across'])
def test_kl_evaluator_end_to_end(mode):
    from abnet3_amd.abx import ABXEvaluator
    # seed, noise and scale of the middle case: the restatement's error is 21.7 % (within) and 30.9 % (across)
    items, feats, times = synthetic_set(np.random.default_rng(31), noise=3.0)
    post = posteriorgrams(feats, 1.0)
    ev = ABXEvaluator(items, post, times, distance='kl')
    r = ev.run(mode)
    assert r.distance == 'kl' and r.n_items == len(items) and not r.dropped and r.n_triplets > 0
    ref = restatement_error(ev, items, mode)
    print('%s: restatement %.6f, device %.6f' % (mode, ref, r.error))
    assert 5.0 < ref < 40.0
    assert abs(r.error - ref) <= 1e-12
    again = ABXEvaluator(items, post, times, distance='kl').run(mode)
    assert np.float64(again.error).tobytes() == np.float64(r.error).tobytes()
    assert again.cells == r.cells
    assert ev.run(mode).cells == r.cells                               # the tables are built once and reused
    items2, feats2, times2 = synthetic_set(np.random.default_rng(32), noise=0.01)
    assert ABXEvaluator(items2, posteriorgrams(feats2, 1.0), times2, distance='kl').run(mode).error == 0.0
    items3, feats3, times3 = synthetic_set(np.random.default_rng(33), n_items=90, separable=False)
    chance = ABXEvaluator(items3, posteriorgrams(feats3, 1.0), times3, distance='kl').run(mode).error
    assert 30.0 < chance < 70.0, chance
    assert ABXEvaluator(items, post, times).run(mode).distance == 'cosine'


def test_kl_evaluator_raises_on_a_bad_frame():
    from abnet3_amd.abx import ABXEvaluator
    items, feats, times = synthetic_set(np.random.default_rng(41))
    post = posteriorgrams(feats, 1.0)
    post[items.files[0]][0, 0] = 0.0                                   # a zero is floored
    assert np.isfinite(ABXEvaluator(items, post, times, distance='kl').run('within').error)
    for v in (np.nan, -0.25):
        post[items.files[0]][0, 0] = v
        with pytest.raises(ValueError, match='dropped'):
            ABXEvaluator(items, post, times, distance='kl').run('within')


def test_softmax_embed_table_to_kl_evaluator():
    from abnet3_amd.abx import ABXEvaluator
    from abnet3_amd.dataloader import DeviceCorpus
    from abnet3_amd.embedder import EmbedderSiamese
    from abnet3_amd.model import SiameseNetwork
    torch.manual_seed(0)
    items, feats, times = synthetic_set(np.random.default_rng(51), D=40)
    net = SiameseNetwork(input_dim=40, num_hidden_layers=1, hidden_dim=64, output_dim=30, p_dropout=0.0,
                         activation_layer='sigmoid', last_non_linearity='softmax', output_path='/tmp/abx_kl_embed_test')
    names = list(feats)
    table = torch.from_numpy(np.concatenate([feats[k] for k in names])).cuda()
    emb = EmbedderSiamese(network=net).embed_table(table)
    assert torch.allclose(emb.sum(dim=1), torch.ones(len(emb), device='cuda'), atol=1e-4)
    corpus = DeviceCorpus.from_table(emb.contiguous(), names, [len(feats[k]) for k in names], times)
    ev = ABXEvaluator(items, corpus, distance='kl')
    for mode in ('within', 'across'):
        r = ev.run(mode)
        assert np.isfinite(r.error) and 0.0 <= r.error <= 100.0 and r.n_triplets > 0
