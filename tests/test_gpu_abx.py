"""ABX evaluation on the MI355X: abn_dtw_cost_batched against abn_dtw_batched and the C oracle (bit for bit),
abn_abx_score against the brute-force restatement (tests/abx_np.py), and ABXEvaluator end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abx_np  # noqa: E402
from test_abx_host import random_items, score_rows_np  # noqa: E402

pytestmark = pytest.mark.gpu

EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]


def pair_table(rng, P, D, quantised, lo=1, hi=200):
    n1 = rng.integers(lo, hi + 1, P).astype(np.int32)
    n2 = rng.integers(lo, hi + 1, P).astype(np.int32)
    if hi >= 200:                       # both sides of every band / round edge
        k = len(EDGES)
        n1[:k] = EDGES
        n2[:k] = EDGES[::-1]
        n1[k:2 * k] = EDGES
        n2[k:2 * k] = EDGES
    if quantised:      # quantised features with repeated frames: many exactly equal costs, the tie-break decides
        f1 = rng.integers(-2, 3, (int(n1.sum()), D)).astype(np.float32)
        f2 = rng.integers(-2, 3, (int(n2.sum()), D)).astype(np.float32)
        f1[1::2] = f1[0:len(f1) - 1:2]
        f2[2::3] = f2[1:len(f2) - 1:3][:len(f2[2::3])]
    else:
        f1 = rng.standard_normal((int(n1.sum()), D)).astype(np.float32)
        f2 = rng.standard_normal((int(n2.sum()), D)).astype(np.float32)
    o1 = np.concatenate(([0], np.cumsum(n1)[:-1])).astype(np.int64)
    o2 = np.concatenate(([0], np.cumsum(n2)[:-1])).astype(np.int64)
    return f1, o1, n1, f2, o2, n2


def raw_cost(f1, o1, n1, f2, o2, n2):
    """abn_dtw_cost_batched alone (no fallback for long tokens)."""
    from abnet3_amd import _lib
    lib = _lib.load()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t1, t2 = dev(f1), dev(f2)
    tab = [dev(np.asarray(o1, np.int64)), dev(np.asarray(n1, np.int32)), dev(np.asarray(o2, np.int64)),
           dev(np.asarray(n2, np.int32))]
    P = len(n1)
    cost = torch.full((P,), 7.0, dtype=torch.float64, device='cuda')
    plen = torch.full((P,), 7, dtype=torch.int32, device='cuda')
    _lib.check(lib.abn_dtw_cost_batched(_lib.ptr(t1), t1.shape[0], _lib.ptr(t2), t2.shape[0], *[_lib.ptr(x) for x in tab],
                                        P, f1.shape[1], _lib.ptr(cost), _lib.ptr(plen), _lib.stream()),
               'abn_dtw_cost_batched')
    return cost.cpu().numpy(), plen.cpu().numpy()


def batched(f1, o1, n1, f2, o2, n2):
    from abnet3_amd.utils import dtw_align_batch
    r = dtw_align_batch(torch.from_numpy(f1).cuda(), o1, n1, torch.from_numpy(f2).cuda(), o2, n2)
    return r.total_cost.cpu().numpy(), r.path_len.cpu().numpy()


@pytest.mark.parametrize('D', [1, 3, 39, 40, 100, 128, 257])
def test_cost_kernel_matches_dtw_batched(D):
    rng = np.random.default_rng(100 + D)
    for quantised in (False, True):
        f1, o1, n1, f2, o2, n2 = pair_table(rng, 300 if D <= 128 else 150, D, quantised)
        # an empty token on either side; a NaN frame (its pair is dropped); an all-zero frame (distance 1: kept)
        n1[-1] = 0
        n2[-2] = 0
        f1[o1[-3]] = np.nan
        f1[o1[-4] + n1[-4] - 1] = 0.0
        got_c, got_l = raw_cost(f1, o1, n1, f2, o2, n2)
        ref_c, ref_l = batched(f1, o1, n1, f2, o2, n2)
        assert np.array_equal(got_l, ref_l), np.flatnonzero(got_l != ref_l)[:10]
        assert np.array_equal(got_c.view(np.int64), ref_c.view(np.int64)), np.flatnonzero(got_c != ref_c)[:10]
        assert got_l[-1] == 0 and got_l[-2] == 0 and got_l[-3] == 0
        if not quantised:              # (quantised frames repeat: a cosine of identical frames may round above 1)
            assert (got_l[:-3] > 0).all()


def test_cost_kernel_unaligned_rows_take_the_scalar_path():
    """D % 4 == 0 but a feature table that is not 16-byte aligned: the scalar dot chain, the same bits."""
    rng = np.random.default_rng(3)
    f1, o1, n1, f2, o2, n2 = pair_table(rng, 200, 40, False, lo=1, hi=90)
    from abnet3_amd import _lib
    lib = _lib.load()
    base = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), f1.ravel()])).cuda()
    t1 = base[1:].view(f1.shape)                                     # 4 bytes past an aligned allocation
    t2 = torch.from_numpy(f2).cuda()
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    tab = [dev(o1, np.int64), dev(n1, np.int32), dev(o2, np.int64), dev(n2, np.int32)]
    P = len(n1)
    cost = torch.empty(P, dtype=torch.float64, device='cuda')
    plen = torch.empty(P, dtype=torch.int32, device='cuda')
    _lib.check(lib.abn_dtw_cost_batched(_lib.ptr(t1), t1.shape[0], _lib.ptr(t2), t2.shape[0], *[_lib.ptr(x) for x in tab],
                                        P, 40, _lib.ptr(cost), _lib.ptr(plen), _lib.stream()), 'abn_dtw_cost_batched')
    ref_c, ref_l = batched(f1, o1, n1, f2, o2, n2)
    assert np.array_equal(plen.cpu().numpy(), ref_l)
    assert np.array_equal(cost.cpu().numpy().view(np.int64), ref_c.view(np.int64))


GRID = 256 * 32                     # the most wavefronts a launch of the cost kernel has


def assert_a_drop_does_not_leak(pick, dropped, ref_l, got_l):
    """The pairs drawn next to an occurrence of the dropped pair -- in front of and behind it in the table, and GRID
    places apart, where its own wavefront takes them -- are not dropped (those the reference keeps; there are some)."""
    at = np.flatnonzero(pick == dropped)
    for step in (1, GRID):
        for nb in (at[at >= step] - step, at[at + step < len(pick)] + step):
            nb = nb[ref_l[pick[nb]] > 0]
            assert len(nb), step
            assert (got_l[nb] > 0).all(), (step, nb[got_l[nb] <= 0][:10])


def test_cost_kernel_grid_stride_many_tiny_pairs():
    """More pairs than the grid has wavefronts: each wavefront works through several; the drop flag and its LDS rows
    must not leak from one pair into the next."""
    rng = np.random.default_rng(13)
    f1, o1, n1, f2, o2, n2 = pair_table(rng, 300, 5, True, lo=1, hi=8)
    f1[o1[7]] = np.nan                                               # this pair is dropped
    ref_c, ref_l = batched(f1, o1, n1, f2, o2, n2)
    assert ref_l[7] == 0
    pick = rng.integers(0, 300, 9000)
    assert len(pick) > GRID
    got_c, got_l = raw_cost(f1, o1[pick], n1[pick], f2, o2[pick], n2[pick])
    assert np.array_equal(got_l, ref_l[pick]), np.flatnonzero(got_l != ref_l[pick])[:10]
    assert np.array_equal(got_c.view(np.int64), ref_c[pick].view(np.int64)), np.flatnonzero(got_c != ref_c[pick])[:10]
    assert_a_drop_does_not_leak(pick, 7, ref_l, got_l)


def test_cost_beyond_the_cap_goes_to_dtw_batched():
    from abnet3_amd import _lib
    from abnet3_amd.abx import dtw_cost_batch
    cap = _lib.load().abn_dtw_cost_max_n2()
    rng = np.random.default_rng(7)
    n1 = np.array([20, 700, 5, 64, 300], dtype=np.int32)
    n2 = np.array([cap, cap + 1, 3 * cap, 65, 40], dtype=np.int32)
    f1 = rng.standard_normal((int(n1.sum()), 24)).astype(np.float32)
    f2 = rng.standard_normal((int(n2.sum()), 24)).astype(np.float32)
    o1 = np.concatenate(([0], np.cumsum(n1)[:-1]))
    o2 = np.concatenate(([0], np.cumsum(n2)[:-1]))
    raw_c, raw_l = raw_cost(f1, o1, n1, f2, o2, n2)
    assert list(raw_l[[1, 2]]) == [-1, -1] and (raw_l[[0, 3, 4]] > 0).all()      # refused by the kernel ...
    c, ln = dtw_cost_batch(torch.from_numpy(f1).cuda(), o1, n1, torch.from_numpy(f2).cuda(), o2, n2)
    ref_c, ref_l = batched(f1, o1, n1, f2, o2, n2)
    assert np.array_equal(ln.cpu().numpy(), ref_l)                                 # ... and computed all the same
    assert np.array_equal(c.cpu().numpy().view(np.int64), ref_c.view(np.int64))


def test_cost_kernel_matches_the_oracle():
    from oracle import dtw_oracle as O
    rng = np.random.default_rng(11)
    f1, o1, n1, f2, o2, n2 = pair_table(rng, 300, 100, False, lo=3, hi=70)
    got_c, got_l = raw_cost(f1, o1, n1, f2, o2, n2)
    for p in range(len(n1)):
        d = O.cosine_distance(f1[o1[p]:o1[p] + n1[p]], f2[o2[p]:o2[p] + n2[p]])
        assert got_c[p] == O.dtw_cost(d), p
        assert got_l[p] == len(O.dtw_path(d)[0]), p


@pytest.mark.parametrize('mode', ['within', 'across'])
def test_score_kernel_matches_brute_force(mode):
    from abnet3_amd.abx import enumerate_cells, abx_score
    rng = np.random.default_rng(21)
    phones, contexts, speakers = random_items(rng, 60, n_phones=3, n_ctx=2, n_spk=3)
    plan = enumerate_cells(phones, contexts, speakers, mode)
    pairs = list(zip(plan.P.tolist(), plan.Q.tolist()))
    trips = abx_np.triplets(phones, contexts, speakers, mode)
    for dist in (rng.integers(0, 5, len(pairs)).astype(np.float64),     # many ties
                 np.full(len(pairs), 0.25),                              # every triplet a tie
                 rng.random(len(pairs))):
        s2, cnt = abx_score(torch.from_numpy(dist).cuda(), plan)
        ref = abx_np.cell_scores(trips, dict(zip(pairs, dist)))
        assert {k: (int(a), int(b)) for k, a, b in zip(plan.cells, s2, cnt)} == ref
        h2, hc = score_rows_np(plan, dist)
        assert np.array_equal(s2, h2) and np.array_equal(cnt, hc)


def synthetic_set(rng, n_items=48, D=20, n_phones=4, separable=True, noise=0.05):
    """Items of 3..12 frames, one utterance per speaker with its items end to end, 10 ms frames."""
    from abnet3_amd.abx import Items
    protos = rng.standard_normal((n_phones, 4, D)).astype(np.float32)
    phones, contexts, speakers = random_items(rng, n_items, n_phones=n_phones, n_ctx=2, n_spk=3)
    cols, feats, times = [], {}, {}
    for s in sorted(set(speakers)):
        rows, t = [], 0
        for i in [i for i in range(n_items) if speakers[i] == s]:
            n = int(rng.integers(3, 13))
            if separable:
                k = int(phones[i][1:])
                src = np.linspace(0, 3, n)
                lo = np.minimum(np.floor(src).astype(int), 2)
                w = (src - lo)[:, None].astype(np.float32)
                f = protos[k, lo] * (1 - w) + protos[k, lo + 1] * w + noise * rng.standard_normal((n, D)).astype(np.float32)
            else:
                f = rng.standard_normal((n, D)).astype(np.float32)
            rows.append(f)
            cols.append((s, (t + 0.5) * 0.01, (t + n - 0.5) * 0.01, phones[i], contexts[i][0], contexts[i][1], s))
            t += n
        feats[s] = np.concatenate(rows).astype(np.float32)
        times[s] = (np.arange(t) + 0.5) * 0.01
    return Items(*zip(*cols)), feats, times


def oracle_error(items, feats, times, mode):
    from abnet3_amd.utils import Features_Accessor
    acc = Features_Accessor(times, dict(feats))
    tok = [acc.get(items.files[i], items.onsets[i], items.offsets[i]) for i in range(len(items))]
    trips = abx_np.triplets(items.phones, items.contexts, items.speakers, mode)
    d = {pq: abx_np.dtw_distance(tok[pq[0]], tok[pq[1]]) for pq in abx_np.needed_pairs(trips)}
    return abx_np.error(abx_np.cell_scores(trips, d))


@pytest.mark.parametrize('mode', ['within', 'across'])
def test_evaluator_end_to_end(mode):
    from abnet3_amd.abx import ABXEvaluator
    items, feats, times = synthetic_set(np.random.default_rng(31), noise=3.0)
    r = ABXEvaluator(items, feats, times).run(mode)
    assert r.n_items == len(items) and not r.dropped and r.n_triplets > 0
    ref = oracle_error(items, feats, times, mode)
    assert 5.0 < ref < 40.0
    assert abs(r.error - ref) <= 1e-12
    again = ABXEvaluator(items, feats, times).run(mode)
    assert np.float64(again.error).tobytes() == np.float64(r.error).tobytes()
    assert again.cells == r.cells
    assert ABXEvaluator(*synthetic_set(np.random.default_rng(32), noise=0.01)).run(mode).error == 0.0
    chance = ABXEvaluator(*synthetic_set(np.random.default_rng(33), n_items=90, separable=False)).run(mode).error
    assert 30.0 < chance < 70.0, chance


def test_evaluator_drops_and_raises():
    from abnet3_amd.abx import ABXEvaluator, Items
    items, feats, times = synthetic_set(np.random.default_rng(41))
    # an item outside every frame is dropped and reported
    extra = Items(items.files + [items.files[0]], list(items.onsets) + [99.0], list(items.offsets) + [99.5],
                  items.phones + ['p0'], [c[0] for c in items.contexts] + ['c0'],
                  [c[1] for c in items.contexts] + ['n0'], items.speakers + [items.speakers[0]])
    r = ABXEvaluator(extra, feats, times).run('within')
    assert [d[0] for d in r.dropped] == [len(items)] and r.n_items == len(items)
    # an all-zero frame is at distance 1 from the others (kept, as in abn_dtw_batched); a non-finite frame drops the
    # pairs of its item: ValueError naming it
    f = {k: v.copy() for k, v in feats.items()}
    f[items.files[0]][0] = 0.0
    assert np.isfinite(ABXEvaluator(items, f, times).run('within').error)
    f[items.files[0]][0] = np.nan
    with pytest.raises(ValueError, match='dropped'):
        ABXEvaluator(items, f, times).run('within')


def test_embed_table_to_evaluator():
    from abnet3_amd.abx import ABXEvaluator
    from abnet3_amd.dataloader import DeviceCorpus
    from abnet3_amd.embedder import EmbedderSiamese
    from abnet3_amd.model import SiameseNetwork
    torch.manual_seed(0)
    items, feats, times = synthetic_set(np.random.default_rng(51), D=40)
    net = SiameseNetwork(input_dim=40, num_hidden_layers=1, hidden_dim=64, output_dim=30, p_dropout=0.0,
                         activation_layer='sigmoid', output_path='/tmp/abx_embed_test')
    names = list(feats)
    table = torch.from_numpy(np.concatenate([feats[k] for k in names])).cuda()
    emb = EmbedderSiamese(network=net).embed_table(table)
    corpus = DeviceCorpus.from_table(emb.contiguous(), names, [len(feats[k]) for k in names], times)
    ev = ABXEvaluator(items, corpus)
    for mode in ('within', 'across'):
        r = ev.run(mode)
        assert np.isfinite(r.error) and 0.0 <= r.error <= 100.0 and r.n_triplets > 0
