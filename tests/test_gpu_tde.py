"""Term scoring on the MI355X: abn_edit_distance_batched against the restated Levenshtein DP (tests/tde_np.py) for exact
equality -- the word edges of the bit-vector recurrence, alphabets, refusals, mixed lengths in one wavefront, the
grid-stride loop, aliased tables --, edit_distance_batch's sort and un-sort, and TermEvaluator end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tde_np  # noqa: E402

pytestmark = pytest.mark.gpu

SHORT = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256]
INT32_MAX = 2 ** 31 - 1


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def offsets(n):
    return (np.cumsum(n) - n).astype(np.int64)


def tables(seqs):
    """(flat int32 table allocated exactly, offsets, lengths) of a list of sequences."""
    n = np.array([len(s) for s in seqs], dtype=np.int32)
    flat = np.concatenate([np.asarray(s, dtype=np.int64) for s in seqs] + [np.zeros(0, np.int64)]).astype(np.int32)
    return flat, offsets(n), n


def raw_edit(t1, o1, n1, t2, o2, n2, max_short):
    """The entry point alone over device tables, the output prefilled with 7 so that what the kernel leaves alone shows."""
    from abnet3_amd import _lib
    lib = _lib.load()
    P = len(n1)
    tab = [dev(o1, np.int64), dev(n1, np.int32), dev(o2, np.int64), dev(n2, np.int32)]
    dist = torch.full((P + 1,), 7, dtype=torch.int32, device='cuda')
    _lib.check(lib.abn_edit_distance_batched(_lib.ptr(t1), t1.numel(), _lib.ptr(t2), t2.numel(), *[_lib.ptr(x) for x in tab], P,
                                             max_short, _lib.ptr(dist), _lib.stream()), 'abn_edit_distance_batched')
    torch.cuda.synchronize()
    out = dist.cpu().numpy()
    assert out[P] == 7                                              # nothing past the last pair
    return out[:P]


def check_pairs(seqs1, seqs2, max_short, what=''):
    """Both orders of the arguments against the restatement; returns the distances."""
    f1, o1, n1 = tables(seqs1)
    f2, o2, n2 = tables(seqs2)
    ref = tde_np.edit_batch(f1, o1, n1, f2, o2, n2, max_short, distance=tde_np.levenshtein_rows)
    t1, t2 = dev(f1, np.int32), dev(f2, np.int32)
    got = raw_edit(t1, o1, n1, t2, o2, n2, max_short)
    assert np.array_equal(got, ref), (what, np.flatnonzero(got != ref)[:10], got[got != ref][:10], ref[got != ref][:10])
    swapped = raw_edit(t2, o2, n2, t1, o1, n1, max_short)
    assert np.array_equal(swapped, ref), (what, 'swapped', np.flatnonzero(swapped != ref)[:10])
    return got


@pytest.mark.parametrize('max_short', [32, 64, 256])
def test_length_edges(max_short):
    """Every short-side edge against a long side of the same length, one more, 300 and 1000; the rows that fit 64 with
    max_short = 64 (the one-word instance), those that fit 32 also with 32 (32-bit words), all others with 256."""
    rng = np.random.default_rng(max_short)
    lo = {32: -1, 64: -1, 256: 64}[max_short]
    seqs1, seqs2 = [], []
    for s in SHORT:
        if lo < s <= max_short:
            for n in (s, s + 1, 300, 1000):
                seqs1.append(rng.integers(0, 4, s))
                seqs2.append(rng.integers(0, 4, n))
    assert len(seqs1) >= 4 * 4
    got = check_pairs(seqs1, seqs2, max_short)
    assert (got >= 0).all()
    if lo < 0:
        assert got[:4].tolist() == [0, 1, 300, 1000]               # the empty side: the other side's length


def alphabet_cases(rng, draw):
    lens = [(5, 9), (31, 40), (32, 32), (64, 64), (64, 200), (65, 130), (128, 129), (129, 129), (200, 256), (256, 300), (0, 7), (1, 1)]
    seqs1 = [draw(a) for a, _ in lens]
    seqs2 = [draw(b) for _, b in lens]
    for n in (64, 65, 128, 129, 256):
        x = draw(n + 1)
        seqs1 += [x[:n], x[:n], x[:n]]
        seqs2 += [x[:n].copy(), x[1:n + 1], x[1:n]]                  # identical; shifted by one (same length; one shorter)
    return seqs1, seqs2


@pytest.mark.parametrize('alphabet', [1, 2, 40, 4096, 'extremes'])
def test_alphabets(alphabet):
    rng = np.random.default_rng(77)
    if alphabet == 'extremes':
        pool = np.array([INT32_MAX, -INT32_MAX - 1, -1, 0, 1, INT32_MAX - 1, -7], dtype=np.int64)
        draw = lambda n: pool[rng.integers(0, len(pool), n)]
    else:
        draw = lambda n: rng.integers(0, alphabet, n)
    seqs1, seqs2 = alphabet_cases(rng, draw)
    got = check_pairs(seqs1, seqs2, 256, alphabet)
    if alphabet == 1:
        assert got.tolist() == [abs(len(a) - len(b)) for a, b in zip(seqs1, seqs2)]
    assert got[12::3].tolist() == [0] * 5                           # identical sequences
    if alphabet in (40, 4096):
        assert got[13::3].max() <= 2 and got[14::3].max() <= 1      # the shift costs at most a deletion and an insertion
    # disjoint alphabets: the longer length
    far1 = [np.asarray(s) % 1000 for s in seqs1]
    far2 = [np.asarray(s) % 1000 + 1000 for s in seqs2]
    got = check_pairs(far1, far2, 256, 'disjoint')
    assert got.tolist() == [max(len(a), len(b)) for a, b in zip(far1, far2)]


@pytest.mark.parametrize('max_short', [20, 32, 64, 100, 256])
def test_refusals_between_good_pairs(max_short):
    """min(n1, n2) = max_short + 1, a negative length, off + n past the rows, offsets far outside the table: -1, the
    neighbours right, and nothing read -- the tables are allocated exactly, without guard rows."""
    rng = np.random.default_rng(5)
    rows = 2 * max_short + 2
    f1, f2 = rng.integers(0, 3, rows).astype(np.int32), rng.integers(0, 3, rows + 1).astype(np.int32)
    good = (0, max_short, 1, max_short + 1)                        # (off1, n1, off2, n2): the short side at the cap
    far = 2 ** 40
    bad = [(0, max_short + 1, 0, max_short + 1), (0, max_short + 2, 0, max_short + 1), (0, -1, 0, 3), (0, 3, 0, -5),
           (rows - 3, 4, 0, 3), (0, 3, rows - 1, 3), (rows, 1, 0, 1), (far, 3, 0, 3), (0, 3, -far, 3), (-1, 3, 0, 3),
           (2 ** 62, INT32_MAX, 0, 3), (0, 3, 2 ** 63 - 1, 1), (far, 0, 0, 3)]
    rows_ = []
    for b in bad:
        rows_ += [good, b]
    rows_ += [good, (rows, 0, rows + 1, 0), (rows - 3, 3, rows - 2, 3)]          # legal: empty at the very end, flush with the end
    o1, n1, o2, n2 = (np.array(c) for c in zip(*rows_))
    ref = tde_np.edit_batch(f1, o1, n1, f2, o2, n2, max_short, distance=tde_np.levenshtein_rows)
    assert (ref[1:2 * len(bad):2] == -1).all() and (ref[0:2 * len(bad):2] == ref[0]).all() and ref[0] >= 0 and ref[-2] == 0
    t1, t2 = dev(f1, np.int32), dev(f2, np.int32)
    assert np.array_equal(raw_edit(t1, o1, n1, t2, o2, n2, max_short), ref)
    assert np.array_equal(raw_edit(t2, o2, n2, t1, o1, n1, max_short), ref)


def test_mixed_lengths_in_one_wavefront_unsorted():
    """256 pairs with lengths drawn from 0 .. 256 in random order through the raw entry: no sorting."""
    rng = np.random.default_rng(6)
    n1, n2 = rng.integers(0, 257, 256), rng.integers(0, 257, 256)
    n1[:8] = [0, 256, 0, 256, 64, 65, 1, 0]
    n2[:8] = [0, 256, 256, 0, 65, 64, 0, 1]
    seqs1 = [rng.integers(0, 3, n) for n in n1]
    seqs2 = [rng.integers(0, 3, n) for n in n2]
    got = check_pairs(seqs1, seqs2, 256)
    assert got[0] == 0 and got[2] == 256 and got[3] == 256 and (got >= 0).all()


def test_grid_stride_many_short_pairs():
    """More pairs than one pass of the grid holds: a lane works through several pairs, its LDS slots and its state must
    not leak from one to the next."""
    from abnet3_amd import _lib
    rng = np.random.default_rng(7)
    K = 400
    seqs1 = [rng.integers(0, 3, n) for n in rng.integers(0, 9, K)]
    seqs2 = [rng.integers(0, 3, n) for n in rng.integers(0, 9, K)]
    f1, o1, n1 = tables(seqs1)
    f2, o2, n2 = tables(seqs2)
    ref = tde_np.edit_batch(f1, o1, n1, f2, o2, n2, 8)
    n_pick = _lib.EDIT_GRID_PAIRS * 2 + 1001
    pick = rng.integers(0, K, n_pick)
    assert len(pick) > 2 * _lib.EDIT_GRID_BLOCKS * _lib.EDIT_BLOCK_PAIRS
    got = raw_edit(dev(f1, np.int32), o1[pick], n1[pick], dev(f2, np.int32), o2[pick], n2[pick], 8)
    assert np.array_equal(got, ref[pick])


def test_one_table_with_aliasing_offsets_and_no_pairs():
    from abnet3_amd import _lib
    rng = np.random.default_rng(8)
    f = rng.integers(0, 5, 500).astype(np.int32)
    o1, n1 = rng.integers(0, 300, 80), rng.integers(0, 120, 80)
    o2, n2 = rng.integers(0, 300, 80), rng.integers(0, 200, 80)
    o2[:10], n2[:10] = o1[:10], n1[:10]                             # a stretch against itself
    o2[10:20] = o1[10:20] + 1                                       # against itself one further
    t = dev(f, np.int32)
    ref = tde_np.edit_batch(f, o1, n1, f, o2, n2, 256, distance=tde_np.levenshtein_rows)
    got = raw_edit(t, o1, n1, t, o2, n2, 256)
    assert np.array_equal(got, ref) and got[:10].tolist() == [0] * 10
    empty = np.zeros(0, np.int64)
    assert len(raw_edit(t, empty, empty, t, empty, empty, 64)) == 0
    assert _lib.load().abn_edit_distance_batched(_lib.ptr(t), 500, _lib.ptr(t), 500, None, None, None, None, 0, 64, None, None) == 0


def test_edit_distance_batch_sorts_and_unsorts():
    from abnet3_amd.tde import edit_distance_batch
    rng = np.random.default_rng(9)
    f1, f2 = rng.integers(0, 4, 3000).astype(np.int32), rng.integers(0, 4, 4000).astype(np.int32)
    P = 1000
    n1, n2 = rng.integers(0, 61, P).astype(np.int32), rng.integers(0, 61, P).astype(np.int32)
    o1, o2 = rng.integers(0, 3000 - 60, P), rng.integers(0, 4000 - 60, P)
    t1, t2 = dev(f1, np.int32), dev(f2, np.int32)
    raw = raw_edit(t1, o1, n1, t2, o2, n2, 64)
    assert (raw >= 0).all() and len(set(raw.tolist())) > 20
    # host arrays (max_short derived from them), device tensors (the cap), a given max_short
    for got in (edit_distance_batch(f1, o1, n1, f2, o2, n2),
                edit_distance_batch(t1, dev(o1, np.int64), dev(n1, np.int32), t2, dev(o2, np.int64), dev(n2, np.int32)),
                edit_distance_batch(t1, o1, n1, t2, o2, n2, max_short=64)):
        assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), raw)
    # refused pairs come back as -1, nothing is raised
    n1b = n1.copy()
    n1b[5], n2[5] = 70, 70
    got = edit_distance_batch(t1, o1, n1b, t2, o2, n2, max_short=64).cpu().numpy()
    assert got[5] == -1 and np.array_equal(np.delete(got, 5), np.delete(raw, 5))
    one = edit_distance_batch(t1, [0, 10], [20, 5], t1, [0, 10], [20, 5])
    assert one.tolist() == [0, 0]
    assert edit_distance_batch(t1, [], [], t2, [], []).numel() == 0
    with pytest.raises(ValueError, match='max_short'):
        edit_distance_batch(t1, o1, n1, t2, o2, n2, max_short=257)
    with pytest.raises(ValueError, match='int32'):
        edit_distance_batch(t1.long(), o1, n1, t2, o2, n2)


def test_evaluator_end_to_end(tmp_path):
    """The synthetic corpus of tests/test_tde_host.py: ned and coverage equal the restatement's with ==, every count and
    per-pair array too; the .classes route and the command line give the same."""
    from abnet3_amd import tde, terms
    lines, clusters, ignore = tde_np.synthetic()
    ref = tde_np.evaluate(clusters, *tde_np.parse_alignment(lines), ignore=ignore)
    (tmp_path / 'phones.txt').write_text('\n'.join(lines) + '\n')
    ev = tde.TermEvaluator(str(tmp_path / 'phones.txt'), ignore=ignore)
    got = ev.evaluate(clusters)
    assert got.ned == ref['ned'] and got.coverage == ref['coverage']
    assert (got.n_clusters, got.n_tokens, got.n_pairs, got.n_skipped) == (ref['n_clusters'], ref['n_tokens'], ref['n_pairs'], ref['n_skipped'])
    for name in ('dist', 'max_len', 'token1', 'token2'):
        assert np.array_equal(getattr(got, name), ref[name]), name
    assert got.dist.dtype == np.int32 and len(got.dist) == got.n_pairs - got.n_skipped
    with open(tmp_path / 'x.classes', 'w') as fh:
        for k, c in enumerate(clusters):
            fh.write('Class %d\n' % k + ''.join('%s %r %r\n' % t for t in c) + '\n')
    again = ev.evaluate(str(tmp_path / 'x.classes'))
    assert again.ned == ref['ned'] and again.coverage == ref['coverage'] and np.array_equal(again.dist, ref['dist'])
    assert tde.summary(got) == 'NED %.4f coverage %.4f (60 clusters, %d tokens, %d pairs, %d skipped)' % (
        ref['ned'], ref['coverage'], ref['n_tokens'], ref['n_pairs'], ref['n_skipped'])
    empty = ev.evaluate([])
    assert np.isnan(empty.ned) and empty.coverage == 0.0 and empty.n_pairs == 0 and len(empty.dist) == 0


def test_discoverer_to_evaluator_round_trip():
    import terms_np
    from abnet3_amd.tde import TermEvaluator, make_alignment
    from abnet3_amd.terms import TermDiscoverer
    feats, times, words = terms_np.planted_corpus()
    files, on, off, sym = [], [], [], []
    for name, v in feats.items():                                  # 80 ms phones over each utterance, five symbols in turn
        for k in range(len(v) // 8):
            files.append(name), on.append(k * 0.08), off.append((k + 1) * 0.08), sym.append('p%d' % (k % 5))
    td = TermDiscoverer(feats, times, theta=0.05)
    td.discover()
    assert len(td.clusters) >= 2
    s = TermEvaluator(make_alignment(files, on, off, sym)).evaluate(td.clusters, td.names, td.corpus.times)
    assert 0 <= s.ned <= 1 and 0 < s.coverage <= 1
    assert s.n_clusters == len(td.clusters) and s.n_tokens == sum(len(c) for c in td.clusters) and s.n_pairs > 0
