"""The host side of abnet3_amd/tde.py without a GPU: the parsers, the inclusion rule at its edges, pair enumeration, NED
and coverage on a hand-computed example and against the restatement (tests/tde_np.py), the argument errors of
abn_edit_distance_batched (which launch nothing) and its header / binding entries."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tde_np  # noqa: E402
from conftest import ROOT  # noqa: E402


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


# ---- the restatement itself, against distances known by hand

def test_restated_distance_on_known_pairs():
    lev = tde_np.levenshtein
    assert lev('kitten', 'sitting') == 3 and lev('sitting', 'kitten') == 3
    assert lev('flaw', 'lawn') == 2 and lev('abc', 'abc') == 0
    assert lev('abc', 'xyzuv') == 5 and lev('xyzuv', 'abc') == 5                 # disjoint alphabets: the longer length
    assert lev('', '') == 0 and lev('', 'abcd') == 4 and lev('abcd', '') == 4
    sym = np.array([1, 2, 3, 1, 2, 4, 9], dtype=np.int32)
    got = tde_np.edit_batch(sym, [0, 0, 0, 5, 0], [3, 3, 0, 2, 3], sym, [3, 3, 3, 6, 0], [3, 5, 2, 1, -1], 2)
    rng = np.random.default_rng(3)
    for alphabet in (1, 2, 5):
        for _ in range(40):
            a, b = (rng.integers(0, alphabet, rng.integers(0, 30)).tolist() for _ in range(2))
            assert tde_np.levenshtein_rows(a, b) == lev(a, b) == lev(b, a)
    assert got.tolist() == [-1, -1, 2, 1, -1]            # min length 3 > 2; outside; empty side; (4, 9) against (9); negative


# ---- parsers

ALIGNMENT = """f2 0.50 0.60 b
f1 0.10 0.20 a
f1 0.00 0.10 SIL

f1 0.20 0.35 c
f2 0.00 0.50 a
"""


def test_read_alignment(tmp_path):
    from abnet3_amd import tde
    path = tmp_path / 'phones.txt'
    path.write_text(ALIGNMENT)
    a = tde.read_alignment(str(path))
    assert a.names == ['f1', 'f2'] and a.symbols == {'SIL': 0, 'a': 1, 'b': 2, 'c': 3}
    assert a.first.tolist() == [0, 3, 5]
    on, off, ids = a.file('f1')
    assert on.tolist() == [0.0, 0.1, 0.2] and off.tolist() == [0.1, 0.2, 0.35] and ids.tolist() == [0, 1, 3]
    on, off, ids = a.file('f2')
    assert on.tolist() == [0.0, 0.5] and off.tolist() == [0.5, 0.6] and ids.tolist() == [1, 2] and ids.dtype == np.int32
    files, symbols = tde_np.parse_alignment(ALIGNMENT.splitlines())
    assert symbols == a.symbols and sorted(files) == a.names
    (tmp_path / 'bad.txt').write_text('f1 0.0 0.1\n')
    with pytest.raises(ValueError, match='bad.txt:1'):
        tde.read_alignment(str(tmp_path / 'bad.txt'))
    (tmp_path / 'nested.txt').write_text('f1 0.0 0.5 a\nf1 0.1 0.2 b\n')
    with pytest.raises(ValueError, match='inside'):
        tde.read_alignment(str(tmp_path / 'nested.txt'))


def test_read_classes_literal_and_as_write_classes_writes_it(tmp_path):
    from abnet3_amd import tde, terms
    path = tmp_path / 'lit.classes'
    path.write_text('Class 0\nf1 0.1 0.25\nf2 1.5 2.0\n\nClass 1\nf1 0.3 0.4\nf1 0.5 0.75\nf3 0 1\n\n')
    assert tde.read_classes(str(path)) == [[('f1', 0.1, 0.25), ('f2', 1.5, 2.0)], [('f1', 0.3, 0.4), ('f1', 0.5, 0.75), ('f3', 0.0, 1.0)]]
    names = [b'utt_a', 'utt_b']
    times = {b'utt_a': np.arange(50) * 0.01 + 0.0125, 'utt_b': np.arange(80) * 0.01 + 0.0125}
    clusters = [[(0, 3, 20), (1, 10, 33)], [(0, 30, 49), (1, 0, 18), (1, 40, 79)]]
    out = terms.write_classes(str(tmp_path / 'w.classes'), names, times, clusters)
    got = tde.read_classes(out)
    assert got == tde.tokens_of(clusters, names, times)
    assert got[0][0] == ('utt_a', float(times[b'utt_a'][3]), float(times[b'utt_a'][20])) and got[1][2][0] == 'utt_b'
    (tmp_path / 'bad.classes').write_text('f1 0.1 0.2\n')
    with pytest.raises(ValueError, match='bad.classes:1'):
        tde.read_classes(str(tmp_path / 'bad.classes'))


# ---- the inclusion rule

def rule_alignment():
    """One file: SIL [0, 0.25), a [0.25, 0.5), b [0.5, 0.53125) (1/32 s: half of it is under 30 ms), c [0.53125, 1.0),
    NSN [1.0, 1.5), d [1.5, 2.0).  Binary fractions: every overlap below is exact."""
    from abnet3_amd import tde
    return tde.make_alignment(['f'] * 6, [0.0, 0.25, 0.5, 0.53125, 1.0, 1.5], [0.25, 0.5, 0.53125, 1.0, 1.5, 2.0],
                              ['SIL', 'a', 'b', 'c', 'NSN', 'd'])


def test_transcription_rule_at_its_edges():
    from abnet3_amd import tde
    a = rule_alignment()
    ids = a.symbols
    assert ids == {'NSN': 0, 'SIL': 1, 'a': 2, 'b': 3, 'c': 4, 'd': 5}

    def phones(on, off, ignore=()):
        table, tok_off, tok_n = tde.transcribe([('f', on, off)], a, ignore)
        assert tok_off.tolist() == [0] and tok_n.tolist() == [len(table)] and table.dtype == np.int32
        return table.tolist()
    # exactly 30 ms of a long phone: in; one ulp less: out
    assert phones(0.0, 0.03) == [ids['SIL']]
    assert phones(0.0, np.nextafter(0.03, 0)) == []
    # exactly half of the 1/32 s phone (1/64 s < 30 ms): in; less than half: out
    assert phones(0.5, 0.515625) == [ids['b']]
    assert phones(0.5, 0.515624) == []
    assert phones(0.515625, 0.53125) == [ids['b']]
    # a phone straddling the token's start: 0.125 s of `a` (>= 30 ms), then b whole, then 2/64 s of c (>= 30 ms)
    assert phones(0.375, 0.5625) == [ids['a'], ids['b'], ids['c']]
    assert phones(0.49, 0.54) == [ids['b']]               # 10 ms of a (of 250), b whole, under 9 ms of c
    # a token covering nothing: before the file, in a gap of overlap zero, beyond its end
    assert phones(-1.0, 0.0) == [] and phones(0.5, 0.5) == [] and phones(2.0, 3.0) == []
    # ignore
    assert phones(0.0, 2.0) == [ids[s] for s in ('SIL', 'a', 'b', 'c', 'NSN', 'd')]
    assert phones(0.0, 2.0, ignore=('SIL', 'NSN', 'nowhere')) == [ids[s] for s in ('a', 'b', 'c', 'd')]
    # several tokens: the flat table
    table, tok_off, tok_n = tde.transcribe([('f', 0.25, 1.0), ('f', 2.0, 3.0), ('f', 1.4, 2.0)], a, ignore=('NSN',))
    assert table.tolist() == [ids['a'], ids['b'], ids['c'], ids['d']] and tok_off.tolist() == [0, 3, 3] and tok_n.tolist() == [3, 0, 1]
    assert tok_off.dtype == np.int64 and tok_n.dtype == np.int32
    with pytest.raises(ValueError, match='elsewhere'):
        tde.transcribe([('f', 0.0, 1.0), ('elsewhere', 0.0, 1.0)], a)
    # the restatement agrees, edge by edge
    files = {'f': list(zip(a.onset.tolist(), a.offset.tolist(), ['SIL', 'a', 'b', 'c', 'NSN', 'd']))}
    for on, off in [(0.0, 0.03), (0.0, np.nextafter(0.03, 0)), (0.5, 0.515625), (0.5, 0.515624), (0.375, 0.5625), (0.49, 0.54)]:
        assert tde_np.transcribe([('f', on, off)], files, ids)[0][0] == phones(on, off)


# ---- pairs

def test_pair_enumeration_order_and_the_overlap_exclusion():
    from abnet3_amd import tde
    clusters = [[('f1', 0.0, 1.0), ('f2', 0.0, 1.0), ('f1', 0.5, 1.5), ('f1', 1.0, 2.0)],       # tokens 0 .. 3
                [('f3', 0.0, 1.0)],                                                               # 4: no pair
                [('f2', 0.0, 1.0), ('f2', 0.25, 0.5)],                                            # 5, 6: overlap, no pair
                [('f9', 3.0, 4.0), ('f8', 3.0, 4.0), ('f9', 0.0, 1.0)]]                           # 7 .. 9
    t1, t2 = tde.cluster_pairs(clusters)
    assert list(zip(t1.tolist(), t2.tolist())) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (5, 6), (7, 8), (7, 9), (8, 9)]
    t1, t2 = tde.pair_table(clusters)
    # (0, 2) and (2, 3) share f1 and overlap; (0, 3) touch at 1.0: kept; (5, 6) overlap
    want = [(0, 1), (0, 3), (1, 2), (1, 3), (7, 8), (7, 9), (8, 9)]
    assert list(zip(t1.tolist(), t2.tolist())) == want and t1.dtype == np.int64
    assert tde_np.pairs(clusters) == want
    assert tde.pair_table([])[0].tolist() == [] and tde.pair_table([[('f', 0.0, 1.0)]])[1].tolist() == []


# ---- NED and coverage

def hand_example():
    """Two files of 1/8 s phones.  f1: a b c d e f g h SIL a b c; f2: a b x d SIL SIL e f g h."""
    s1, s2 = 'a b c d e f g h SIL a b c'.split(), 'a b x d SIL SIL e f g h'.split()
    lines = ['f1 %r %r %s' % (k / 8, (k + 1) / 8, s) for k, s in enumerate(s1)] + ['f2 %r %r %s' % (k / 8, (k + 1) / 8, s) for k, s in enumerate(s2)]
    clusters = [[('f1', 0.0, 0.5), ('f2', 0.0, 0.5), ('f1', 1.125, 1.5)],        # abcd, abxd, abc: 1/4, 1/4, 1/4
                [('f1', 0.5, 1.0), ('f2', 0.75, 1.25)],                          # efgh, efgh: 0
                [('f2', 0.5, 0.75), ('f1', 1.0, 1.125), ('f1', 0.875, 1.25)]]    # SIL SIL -> '', SIL -> '', h SIL a -> 'ha'
    return lines, clusters


def test_ned_and_coverage_by_hand(tmp_path):
    from abnet3_amd import tde
    lines, clusters = hand_example()
    (tmp_path / 'phones.txt').write_text('\n'.join(lines[::-1]) + '\n')
    ev = tde.TermEvaluator(str(tmp_path / 'phones.txt'), ignore=['SIL'])
    classes, flat, (table, tok_off, tok_n), (t1, t2), n_pairs, n_skipped, coverage = ev.prepare(clusters)
    assert tok_n.tolist() == [4, 4, 3, 4, 4, 0, 0, 2] and len(flat) == 8
    # cluster 2: (5, 6) both empty: skipped; (6, 7) share f1 and overlap: left out; (5, 7) scored
    assert n_pairs == 6 and n_skipped == 1
    assert list(zip(t1.tolist(), t2.tolist())) == [(0, 1), (0, 2), (1, 2), (3, 4), (5, 7)]
    sym = ev.alignment.symbols
    assert table[:4].tolist() == [sym[c] for c in 'abcd'] and table[tok_off[7]:].tolist() == [sym['h'], sym['a']]
    # f1: a b c d e f g h a b c all inside a token (11 of 11); f2: a b x d e f g h (8 of 8)
    assert coverage == 19 / 19
    # the distances, from the restatement (no GPU here): abcd/abxd 1, abcd/abc 1, abxd/abc 2, efgh/efgh 0, ''/ha 2
    dist = tde_np.edit_batch(table, tok_off[t1], tok_n[t1], table, tok_off[t2], tok_n[t2], 256)
    assert dist.tolist() == [1, 1, 2, 0, 2]
    max_len = np.maximum(tok_n[t1], tok_n[t2])
    assert max_len.tolist() == [4, 4, 4, 4, 2]
    assert tde.ned(dist, max_len) == np.mean(np.array([0.25, 0.25, 0.5, 0.0, 1.0]))
    assert math.isnan(tde.ned(dist[:0], max_len[:0]))
    ref = tde_np.evaluate(clusters, *tde_np.parse_alignment(lines), ignore=('SIL',))
    assert ref['ned'] == tde.ned(dist, max_len) and ref['coverage'] == coverage
    assert (ref['n_clusters'], ref['n_tokens'], ref['n_pairs'], ref['n_skipped']) == (3, 8, 6, 1)
    assert ref['dist'].tolist() == dist.tolist() and ref['token1'].tolist() == t1.tolist() and ref['token2'].tolist() == t2.tolist()
    # fewer tokens: coverage drops
    assert ev.prepare(clusters[1:2])[-1] == 8 / 19
    # frame tokens with names and times, as TermDiscoverer holds them
    names, times = ['f1', 'f2'], {'f1': np.arange(150) * 0.01 + 0.005, 'f2': np.arange(125) * 0.01 + 0.005}
    got = ev.prepare([[(0, 0, 49), (1, 0, 49)]], names, times)
    assert got[1] == [('f1', 0.005, float(times['f1'][49])), ('f2', 0.005, float(times['f2'][49]))] and got[2][2].tolist() == [4, 4]
    with pytest.raises(ValueError, match='times'):
        ev.prepare([[(0, 0, 49), (1, 0, 49)]], names)
    with pytest.raises(ValueError, match='f7'):
        ev.prepare([[('f1', 0.0, 0.5), ('f7', 0.0, 0.5)]])


def test_host_half_matches_the_restatement_on_the_synthetic_corpus():
    """The input of the GPU end-to-end test: transcriptions, pair table, counts and coverage equal the restatement's, and
    it does not degenerate -- under 10 % of the pairs are skipped, some pairs are excluded, some tokens are empty."""
    from abnet3_amd import tde
    lines, clusters, ignore = tde_np.synthetic()
    files, symbols = tde_np.parse_alignment(lines)
    assert len(files) == 20 and all(50 <= len(v) <= 200 for v in files.values()) and len(symbols) == 40
    ref = tde_np.evaluate(clusters, files, symbols, ignore)
    assert ref['n_skipped'] < 0.1 * ref['n_pairs'] and ref['n_skipped'] > 0
    assert ref['n_pairs'] < sum(len(c) * (len(c) - 1) // 2 for c in clusters)           # the exclusion acts
    assert 0 < ref['ned'] <= 1 and 0 < ref['coverage'] < 1
    a = tde.make_alignment(*zip(*[(ln.split()[0], float(ln.split()[1]), float(ln.split()[2]), ln.split()[3]) for ln in lines]))
    assert a.symbols == symbols
    ev = tde.TermEvaluator(a, ignore=ignore)
    classes, flat, (table, tok_off, tok_n), (t1, t2), n_pairs, n_skipped, coverage = ev.prepare(clusters)
    trans, _ = tde_np.transcribe(flat, files, symbols, ignore)
    assert [table[o:o + n].tolist() for o, n in zip(tok_off, tok_n)] == trans
    assert (n_pairs, n_skipped, coverage) == (ref['n_pairs'], ref['n_skipped'], ref['coverage'])
    assert t1.tolist() == ref['token1'].tolist() and t2.tolist() == ref['token2'].tolist()


# ---- the C entry: what launches nothing

def test_edit_entry_argument_errors(lib):
    from abnet3_amd import _lib
    assert lib.abn_edit_max_short() == _lib.EDIT_MAX_SHORT == 256
    p = ctypes.c_void_p(0x1000)
    args = lambda **kw: [kw.get(k, d) for k, d in (('sym1', p), ('rows1', 10), ('sym2', p), ('rows2', 10), ('off1', p), ('n1', p),
                                                     ('off2', p), ('n2', p), ('npairs', 4), ('max_short', 64), ('dist', p),
                                                     ('stream', None))]
    for name in ('sym1', 'sym2', 'off1', 'n1', 'off2', 'n2', 'dist'):
        assert lib.abn_edit_distance_batched(*args(**{name: None})) == _lib.E_ARG, name
        assert b'null' in lib.abn_last_error()
    for bad in (0, 257, -1):
        assert lib.abn_edit_distance_batched(*args(max_short=bad)) == _lib.E_ARG
        assert b'max_short' in lib.abn_last_error() and b'256' in lib.abn_last_error()
    assert lib.abn_edit_distance_batched(*args(npairs=-1)) == _lib.E_ARG
    assert lib.abn_edit_distance_batched(*args(npairs=0)) == 0                       # returns at once: nothing is launched
    assert lib.abn_edit_distance_batched(*args(npairs=0, sym1=None, dist=None)) == 0
    assert lib.abn_edit_distance_batched(*args(npairs=0, max_short=0)) == _lib.E_ARG


def test_header_and_binding_entries():
    from abnet3_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read()
    assert re.search(r'#define ABN_EDIT_MAX_SHORT (\d+)', text).group(1) == str(_lib.EDIT_MAX_SHORT)
    assert int(re.search(r'#define ABN_EDIT_GRID_BLOCKS (\d+)', text).group(1)) == _lib.EDIT_GRID_BLOCKS
    assert int(re.search(r'#define ABN_EDIT_BLOCK_PAIRS (\d+)', text).group(1)) == _lib.EDIT_BLOCK_PAIRS
    assert _lib.EDIT_GRID_PAIRS == _lib.EDIT_GRID_BLOCKS * _lib.EDIT_BLOCK_PAIRS
    assert re.search(r'int64_t abn_edit_max_short\(void\);', text)
    assert re.search(r'int abn_edit_distance_batched\(const int32_t\* sym1, int64_t rows1, const int32_t\* sym2, int64_t rows2,\s*'
                     r'const int64_t\* off1, const int32_t\* n1, const int64_t\* off2, const int32_t\* n2,\s*'
                     r'int64_t npairs, int64_t max_short, int32_t\* dist, void\* stream\);', text)
    assert re.search(r'#define ABN_ABI_VERSION 20\b', text) and _lib.ABI_VERSION == 20
    res, argtypes = _lib.SYMBOLS['abn_edit_distance_batched']
    assert res is ctypes.c_int and len(argtypes) == 12
    assert [argtypes[k] for k in (1, 3, 8, 9)] == [ctypes.c_int64] * 4
    assert all(argtypes[k] is ctypes.c_void_p for k in (0, 2, 4, 5, 6, 7, 10, 11))
    assert _lib.SYMBOLS['abn_edit_max_short'] == (ctypes.c_int64, [])
    import abnet3_amd
    from abnet3_amd import tde
    assert abnet3_amd.TermEvaluator is tde.TermEvaluator and abnet3_amd.edit_distance_batch is tde.edit_distance_batch


def test_command_line_refuses_without_files():
    from abnet3_amd import tde
    with pytest.raises(SystemExit):
        tde.main([])
