"""ABX evaluation, host side (no GPU): the item-file reader, the cell / needed-pair enumeration against a brute-force
restatement (tests/abx_np.py), the aggregation order, and the command line without h5features."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abx_np  # noqa: E402


def score_rows_np(plan, dist):
    """What abn_abx_score computes, restated on the host: per cell, (2 x score sum, triplet count)."""
    s2 = np.zeros(len(plan.cells), dtype=np.int64)
    cnt = np.zeros(len(plan.cells), dtype=np.int64)
    for ao, al, bo, bl, c in zip(plan.a_off, plan.a_len, plan.b_off, plan.b_len, plan.row_cell):
        da, db = dist[ao:ao + al][:, None], dist[bo:bo + bl][None, :]
        s2[c] += int(2 * (da < db).sum() + (da == db).sum())
        cnt[c] += al * bl
    return s2, cnt


def random_items(rng, n, n_phones=4, n_ctx=2, n_spk=3):
    phones = ['p%d' % v for v in rng.integers(0, n_phones, n)]
    contexts = [('c%d' % v, 'n%d' % w) for v, w in zip(rng.integers(0, n_ctx, n), rng.integers(0, 2, n))]
    speakers = ['s%d' % v for v in rng.integers(0, n_spk, n)]
    return phones, contexts, speakers


def test_read_item_file(tmp_path):
    from abnet3_amd.abx import read_item_file
    p = tmp_path / 'items.item'
    p.write_text('#file onset offset #phone prev-phone next-phone speaker\n'
                 'utt_a 0.0125 0.1875 ae  b t s01\n'
                 'utt_b\t1.5\t1.75\tiy\t\tSIL  k   s02\n'
                 '\n'
                 'utt_a 2 2.0625e0 ae b t s01\n')
    it = read_item_file(str(p))
    assert len(it) == 3
    assert it.files == ['utt_a', 'utt_b', 'utt_a']
    assert it.onsets.dtype == np.float64 and list(it.onsets) == [0.0125, 1.5, 2.0]
    assert list(it.offsets) == [0.1875, 1.75, 2.0625]
    assert it.phones == ['ae', 'iy', 'ae']
    assert it.contexts == [('b', 't'), ('SIL', 'k'), ('b', 't')]
    assert it.speakers == ['s01', 's02', 's01']
    bad = tmp_path / 'bad.item'
    bad.write_text('#file onset offset #phone prev-phone next-phone speaker\nutt 0.1 0.2 a b c\n')
    with pytest.raises(ValueError):
        read_item_file(str(bad))


@pytest.mark.parametrize('mode', ['within', 'across'])
@pytest.mark.parametrize('seed', range(6))
def test_enumeration_matches_brute_force(mode, seed):
    from abnet3_amd.abx import enumerate_cells
    rng = np.random.default_rng(seed)
    phones, contexts, speakers = random_items(rng, int(rng.integers(8, 30)))
    plan = enumerate_cells(phones, contexts, speakers, mode)
    trips = abx_np.triplets(phones, contexts, speakers, mode)
    # every needed ordered pair exactly once, and nothing else
    pairs = list(zip(plan.P.tolist(), plan.Q.tolist()))
    assert len(pairs) == len(set(pairs))
    assert set(pairs) == abx_np.needed_pairs(trips)
    # the same cells with the same triplet counts and, on random distances with ties, the same scores
    dist = rng.integers(0, 4, len(pairs)).astype(np.float64)
    d = dict(zip(pairs, dist))
    ref = abx_np.cell_scores(trips, d)
    s2, cnt = score_rows_np(plan, dist)
    assert len(plan.cells) == len(set(plan.cells))
    got = {k: (int(a), int(b)) for k, a, b in zip(plan.cells, s2, cnt)}
    assert got == ref
    if ref:
        from abnet3_amd.abx import aggregate
        assert abs(aggregate(plan.cells, s2, cnt)[0] - abx_np.error(ref)) < 1e-12


def test_aggregation_order_is_pinned():
    """Cells are averaged over contexts, then speaker keys, then phone pairs -- not weighted by triplets."""
    from abnet3_amd.abx import enumerate_cells, aggregate
    # context c1: items 0, 1 phone a, item 2 phone b; context c2: items 3, 4 phone a, items 5, 6, 7 phone b
    phones = ['a', 'a', 'b', 'a', 'a', 'b', 'b', 'b']
    contexts = [('x', 'y')] * 3 + [('x', 'z')] * 5
    speakers = ['s'] * 8
    plan = enumerate_cells(phones, contexts, speakers, 'within')
    d = {}
    for p, q in zip(plan.P.tolist(), plan.Q.tolist()):
        same = phones[p] == phones[q]
        if contexts[q] == ('x', 'y'):
            d[(p, q)] = 0.1 if same else 1.0          # (a, b, c1): every triplet right
        elif phones[q] == 'a':
            d[(p, q)] = 2.0 if same else 1.0          # (a, b, c2): every triplet wrong
        else:
            d[(p, q)] = 0.5 if same else 1.0          # (b, a, c2): every triplet right
    dist = np.array([d[pq] for pq in zip(plan.P.tolist(), plan.Q.tolist())])
    s2, cnt = score_rows_np(plan, dist)
    counts = dict(zip(plan.cells, cnt.tolist()))
    assert counts == {('a', 'b', ('x', 'y'), 's'): 2, ('a', 'b', ('x', 'z'), 's'): 6, ('b', 'a', ('x', 'z'), 's'): 12}
    err, by_pair, _ = aggregate(plan.cells, s2, cnt)
    assert by_pair == {('a', 'b'): 0.5, ('b', 'a'): 1.0}
    assert err == 25.0                                  # triplet-weighted: 100 (1 - 14 / 20) = 30
    # speaker keys are averaged before phone pairs
    cells = [('a', 'b', 'c1', ('s1', 's2')), ('a', 'b', 'c2', ('s1', 's2')), ('a', 'b', 'c1', ('s2', 's1')),
             ('b', 'a', 'c1', ('s1', 's2'))]
    err, by_pair, cell_score = aggregate(cells, [2, 0, 6, 1], [1, 1, 3, 1])
    assert cell_score == [1.0, 0.0, 1.0, 0.5]
    assert by_pair == {('a', 'b'): 0.75, ('b', 'a'): 0.5}
    assert err == 37.5


def test_command_line_without_h5features(tmp_path, monkeypatch):
    from abnet3_amd import abx
    monkeypatch.setitem(sys.modules, 'h5features', None)          # import h5features -> ImportError
    items = tmp_path / 'i.item'
    items.write_text('#file onset offset #phone prev-phone next-phone speaker\nu 0 1 a b c s\n')
    with pytest.raises(ImportError, match='h5features'):
        abx.main([str(tmp_path / 'emb.h5f'), str(items), '--mode', 'within'])
