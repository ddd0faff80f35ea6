"""The pair-free histogram kernel (csrc/edit_hist.hip, abns_edit_cluster_hist) and the full term scores on an MI355X: hist,
n_pairs and n_skipped EQUAL the restatement (tests/tde_full_np.py) at both edges of the three instantiations and on cluster
sizes around the wavefront; the same bits from two calls, under any order of the tokens and the clusters, for any grid and
on dirty memory; 2 449 965 000 pairs of one cluster against the closed form; no allocation that grows with the pairs;
evaluate_full against evaluate and against the restatement; ESKMeans.term_scores on a small fitted model.

Needs an MI355X: -m gpu."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tde_full_np as full_np  # noqa: E402
import tde_np  # noqa: E402
from dirty_memory import dirty  # noqa: E402

pytestmark = pytest.mark.gpu

COLUMNS = ('table', 'tok_off', 'tok_n', 'tok_file', 'tok_on', 'tok_end', 'cl_first')
SIZES = [1, 2, 3, 63, 64, 65, 129]
# name -> (cluster sizes, transcription lengths, alphabet): the three instantiations (M <= 32, <= 64, <= 256) at both edges;
# the quadratic reference keeps the clusters of long tokens small
TABLES = {
    'short-2': (SIZES + [1] * 70 + [0, 0, 2, 2] + [1] * 70 + [5], [0, 1, 2, 7, 31, 32], 2),
    'short-40': ([0] + SIZES[::-1] + [1] * 30, [0, 1, 3, 12, 31, 32], 40),
    'one-word-2': ([1, 0, 2, 3, 65, 64, 1, 1, 9], [0, 1, 32, 33, 63, 64], 2),
    'one-word-40': ([3, 63, 1, 2, 1, 40], [0, 1, 33, 63, 64], 40),
    'four-words-2': ([1, 2, 3, 0, 14, 1, 9], [0, 1, 64, 65, 255, 256], 2),
    'four-words-40': ([12, 1, 3, 2, 10], [0, 1, 65, 255, 256], 40),
    'none': ([], [1], 2),
    'singles': ([1] * 200 + [0] * 5, [0, 3], 2),
}
_TABLE, _REF = {}, {}


def table_of(name):
    if name not in _TABLE:
        sizes, lengths, alphabet = TABLES[name]
        _TABLE[name] = full_np.token_table(np.random.default_rng(sum(map(ord, name))), sizes, lengths, alphabet)
    return _TABLE[name]


def reference(name):
    """The restated (hist, n_pairs, n_skipped) of a table: computed once, shared by the tests, never written to."""
    if name not in _REF:
        hist, n_pairs, n_skipped = full_np.table_histogram(table_of(name))
        hist.setflags(write=False)
        _REF[name] = (hist, n_pairs, n_skipped)
    return _REF[name]


def run(t, with_groups=True, **change):
    from abnet3_amd import tde
    a = dict(t)
    a.update(change)
    return tde.cluster_histogram(*[a[k] for k in COLUMNS], groups=a['groups'] if with_groups else None)


def assert_equal(got, want, what=''):
    assert got[0].dtype == np.int64 and got[0].shape == want[0].shape, (what, got[0].shape, want[0].shape)
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5])
    assert got[1:] == want[1:], (what, got[1:], want[1:])


@pytest.mark.parametrize('name', sorted(TABLES))
def test_counts_equal_the_restatement(name):
    t, want = table_of(name), reference(name)
    got = run(t)
    assert_equal(got, want, name)
    assert_equal(run(t), got, name + ': a second call')
    M = max(1, int(t['tok_n'].max())) if len(t['tok_n']) else 1
    assert got[0].shape == (2, M + 1, M + 1) and got[0].sum() == got[1] - got[2]
    if name.startswith(('short', 'one-word')):                                # the larger tables exercise every branch
        sizes = np.diff(t['cl_first'])
        assert got[1] < int((sizes * (sizes - 1) // 2).sum()) and got[2] > 0 and got[0][0].sum() > 0 and got[0][1].sum() > 0
        assert got[0][:, 0, :].sum() > 0 and (got[0].sum(axis=(0, 1)) > 0)[[1, M]].all()
    one = run(t, with_groups=False)                                                # no speakers: everything is "within"
    assert np.array_equal(one[0][0], want[0][0] + want[0][1]) and not one[0][1].any() and one[1:] == want[1:]


@pytest.mark.parametrize('name', ['short-2', 'one-word-40', 'four-words-2'])
def test_the_same_bits_for_any_order_any_grid_and_on_dirty_memory(name, monkeypatch):
    t, want = table_of(name), reference(name)
    rng = np.random.default_rng(7)
    first = t['cl_first']
    for _ in range(2):
        cl = rng.permutation(len(first) - 1)
        order = np.concatenate([first[c] + rng.permutation(first[c + 1] - first[c]) for c in cl]).astype(np.int64)
        moved = {k: t[k][order] for k in ('tok_off', 'tok_n', 'tok_file', 'tok_on', 'tok_end', 'groups')}
        moved['cl_first'] = np.concatenate([[0], np.cumsum(np.diff(first)[cl])]).astype(np.int64)
        assert_equal(run(t, **moved), want, name + ': permuted')
    for blocks in ('1', '3', '64', '65536'):
        monkeypatch.setenv('ABN_EDIT_HIST_BLOCKS', blocks)                    # read at every call
        assert_equal(run(t), want, '%s: %s workgroups' % (name, blocks))
    monkeypatch.delenv('ABN_EDIT_HIST_BLOCKS')
    for byte in (0xFF, 0xC2):                                                 # hist, counts and the workspace come from torch.empty
        with dirty(byte) as count:
            got = run(t)
        assert int(count) >= 3
        assert_equal(got, want, '%s: memory of 0x%02X' % (name, byte))


def test_device_columns_are_taken_as_they_are_and_bad_tokens_fail_the_call():
    from abnet3_amd import _lib, tde
    t, want = table_of('short-40'), reference('short-40')
    on_device = {k: torch.from_numpy(t[k]).cuda() for k in COLUMNS[:-1] + ('groups',)}
    assert_equal(run(t, **on_device), want, 'device columns')
    assert_equal(run(t, cl_first=torch.from_numpy(t['cl_first']).cuda()), want, 'cl_first from the device')
    long = t['tok_n'].copy()
    long[3] = 257
    with pytest.raises(ValueError, match='257'):
        run(t, tok_n=long)
    # the C entry itself: a token that leaves the table, or one longer than M, fails the call and leaves hist and counts alone
    lib = _lib.load()
    M = int(t['tok_n'].max())
    for column, at, value in (('tok_off', 5, len(t['table'])), ('tok_off', 0, -1), ('tok_n', 2, M + 1), ('tok_n', 7, -1)):
        cols = dict(on_device)
        bad = t[column].copy()
        bad[at] = value
        cols[column] = torch.from_numpy(bad).cuda()
        hist = torch.full((2, M + 1, M + 1), -7, dtype=torch.int64, device='cuda')
        counts = torch.full((2,), -7, dtype=torch.int64, device='cuda')
        n_ws = lib.abns_edit_cluster_hist_ws_bytes(len(bad), len(t['cl_first']) - 1, 0)
        ws = torch.empty(n_ws, dtype=torch.uint8, device='cuda')
        rc = lib.abns_edit_cluster_hist(_lib.ptr(cols['table']), cols['table'].numel(), *[_lib.ptr(cols[k]) for k in COLUMNS[1:6]],
                                        _lib.ptr(cols['groups']), len(bad), t['cl_first'].ctypes.data, len(t['cl_first']) - 1, M,
                                        _lib.ptr(hist), _lib.ptr(counts), _lib.ptr(ws), n_ws, _lib.stream())
        torch.cuda.synchronize()
        assert rc == _lib.E_ARG and b'token' in lib.abn_last_error(), (column, at)
        assert (hist == -7).all() and (counts == -7).all()
    with pytest.raises(_lib.HipLibraryError, match='token'):
        run(t, tok_off=t['tok_off'] + 1)                                      # the last token now ends one past the table


def test_past_two_to_the_31_pairs_against_the_closed_form():
    """One cluster of 70 000 one-symbol tokens over two symbols: C(70000, 2) = 2 449 965 000 pairs, more than a 32-bit
    counter or a 32-bit pair index holds."""
    n, n_a = 70000, 30011
    rng = np.random.default_rng(31)
    sym = np.zeros(n, dtype=np.int32)
    sym[rng.permutation(n)[:n - n_a]] = 1
    n_b = n - n_a
    k = np.arange(n)
    hist, n_pairs, n_skipped = run(dict(table=sym, tok_off=k.astype(np.int64), tok_n=np.ones(n, dtype=np.int32), tok_file=(k % 7).astype(np.int32),
                                        tok_on=k.astype(np.float64), tok_end=k + 0.5, cl_first=np.array([0, n], dtype=np.int64), groups=None),
                                   with_groups=False)
    assert n * (n - 1) // 2 == 2449965000 > 2 ** 31
    assert n_pairs == 2449965000 and n_skipped == 0 and hist.shape == (2, 2, 2)
    assert hist[0][0][1] == n_a * (n_a - 1) // 2 + n_b * (n_b - 1) // 2 and hist[0][1][1] == n_a * n_b
    assert hist.sum() == n_pairs and not hist[1].any()


def test_no_allocation_grows_with_the_pairs():
    """One cluster of 2 000 tokens of 1 - 8 symbols: 1 999 000 pairs.  The inputs are about 0.14 MB and hist under 2 KB; a work
    list of one 16-byte item per 64 pairs would be 0.53 MB; the pair table's four columns alone are 24 B x P = 48 MB."""
    t = full_np.token_table(np.random.default_rng(5), [2000], list(range(1, 9)), 40)
    run(t)                                                                    # (the library and its kernels are loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    hist, n_pairs, n_skipped = run(t)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print('peak device memory over cluster_histogram, uploads included: %d bytes for %d pairs' % (peak, n_pairs))
    assert n_pairs > 1900000 and hist.sum() == n_pairs
    assert peak <= 4 << 20


def test_evaluate_full_against_evaluate_and_the_restatement(tmp_path, capsys):
    from abnet3_amd import tde
    lines, clusters, ignore = tde_np.synthetic()
    word_lines, clusters = full_np.synthetic_words(lines, clusters)
    files, symbols = tde_np.parse_alignment(lines)
    speakers = full_np.speakers_of(files)
    (tmp_path / 'phones.txt').write_text('\n'.join(lines) + '\n')
    (tmp_path / 'words.txt').write_text('\n'.join(word_lines) + '\n')
    (tmp_path / 'spk.txt').write_text(''.join('%s %s\n' % kv for kv in speakers.items()))
    with open(tmp_path / 'x.classes', 'w') as fh:
        for k, c in enumerate(clusters):
            fh.write('Class %d\n' % k + ''.join('%s %r %r\n' % t for t in c) + '\n')
    ev = tde.TermEvaluator(str(tmp_path / 'phones.txt'), ignore=ignore)
    old = ev.evaluate(str(tmp_path / 'x.classes'))
    got = ev.evaluate_full(str(tmp_path / 'x.classes'), words=str(tmp_path / 'words.txt'), speakers=speakers)
    assert (got.n_pairs, got.n_skipped, got.coverage, got.n_clusters, got.n_tokens) == (old.n_pairs, old.n_skipped, old.coverage,
                                                                                      old.n_clusters, old.n_tokens)
    assert got.hist.sum() == len(old.dist) and abs(got.ned - old.ned) <= 1e-13 * old.ned
    ref = full_np.evaluate_full(clusters, files, symbols, ignore, tde_np.parse_alignment(word_lines)[0], None, speakers)
    for name in got._fields:
        a, b = getattr(got, name), ref[name]
        assert np.array_equal(a, b) if name == 'hist' else (tuple(a) == tuple(b) if isinstance(a, tuple) else a == b), name
    # within / across from evaluate's per-pair arrays
    flat = [t for c in clusters for t in c]
    spk = np.array([speakers[t[0]] for t in flat])
    within = spk[old.token1] == spk[old.token2]
    for part, mask in ((got.ned_within, within), (got.ned_across, ~within)):
        mean = tde.ned(old.dist[mask], old.max_len[mask])
        assert abs(part - mean) <= 1e-13 * mean
    assert tde.main([str(tmp_path / 'x.classes'), str(tmp_path / 'phones.txt'), '--full', '--words', str(tmp_path / 'words.txt'),
                     '--speakers', str(tmp_path / 'spk.txt'), '--ignore'] + list(ignore)) == 0
    assert capsys.readouterr().out.strip() == tde.full_summary(got)
    assert tde.main([str(tmp_path / 'x.classes'), str(tmp_path / 'phones.txt'), '--ignore'] + list(ignore)) == 0
    assert capsys.readouterr().out.strip() == tde.summary(old)                # without --full: today's line
    empty = ev.evaluate_full([])
    assert math.isnan(empty.ned) and empty.n_pairs == 0 and empty.hist.shape == (2, 2, 2) and empty.grouping == (0.0, 0.0, 0.0)


def test_term_scores_of_a_fitted_eskmeans_and_of_a_discoverer():
    """Planted words as in tests/test_gpu_esk.py: five templates, every word one phone of the alignment and one word of the
    word alignment -- the segmentation recovers them, so every score is perfect."""
    import esk_np
    import terms_np
    from abnet3_amd import eskmeans, tde
    from abnet3_amd.terms import TermDiscoverer
    rng = np.random.default_rng(12)
    D, frames, lens = 8, 10, (10, 13, 16, 18, 20)
    templates = [rng.standard_normal((n, D)).astype(np.float32) for n in lens]
    feats, times, lms, files, on, off, sym = {}, {}, {}, [], [], [], []
    for u in range(4):
        name = 's%d_utt%d' % (u % 2, u)
        words = list(rng.permutation(5)) + list(rng.integers(0, 5, size=2))
        x = np.concatenate([templates[w] for w in words])
        feats[name] = (x + 0.01 * rng.standard_normal(x.shape)).astype(np.float32)
        times[name] = 0.0125 + 0.01 * np.arange(len(x))
        bounds = np.concatenate(([0], np.cumsum([lens[w] for w in words])))
        lms[name] = np.unique(np.concatenate((bounds, (bounds[:-1] + bounds[1:]) // 2))).astype(np.int64)
        for a, e, w in zip(bounds[:-1], bounds[1:], words):
            files.append(name), on.append(times[name][a] - 0.005), off.append(times[name][e - 1] + 0.005), sym.append('w%d' % w)
    init = np.stack([esk_np.vector(t, 0, len(t), frames)[0] for t in templates]).astype(np.float64)
    q = eskmeans.ESKMeans(5, frames=frames, max_span=6, n_iter=5).fit(feats, lms, init=init, times=times)
    align = tde.make_alignment(files, on, off, sym)
    s = q.term_scores(tde.TermEvaluator(align), words=align, speakers=lambda f: f.split('_')[0])
    assert isinstance(s, tde.FullTermScores) and s.n_tokens == 28 and s.n_clusters == 5 and s.n_gold == 28 and s.n_empty == 0
    assert s.ned == 0.0 and s.ned_within == 0.0 and s.ned_across == 0.0 and s.coverage == 1.0
    assert s.token == (1.0, 1.0, 1.0) and s.type == (1.0, 1.0, 1.0) and s.boundary == (1.0, 1.0, 1.0) and s.grouping == (1.0, 1.0, 1.0)
    assert s.n_pairs == s.n_same == s.hist.sum() and s.hist[0].sum() > 0 and s.hist[1].sum() > 0
    feats2, times2, _ = terms_np.planted_corpus()
    td = TermDiscoverer(feats2, times2, theta=0.05)
    td.discover()
    pf, po, pe, ps = [], [], [], []
    for name, v in feats2.items():                                            # 80 ms phones, five symbols in turn
        for k in range(len(v) // 8):
            pf.append(name), po.append(k * 0.08), pe.append((k + 1) * 0.08), ps.append('p%d' % (k % 5))
    ev = tde.TermEvaluator(tde.make_alignment(pf, po, pe, ps))
    s2, old = td.term_scores(ev), ev.evaluate(td.clusters, td.names, td.corpus.times)
    assert (s2.n_pairs, s2.n_skipped, s2.coverage, s2.n_tokens) == (old.n_pairs, old.n_skipped, old.coverage, old.n_tokens)
    assert s2.token is None and abs(s2.ned - old.ned) <= 1e-13 * old.ned
