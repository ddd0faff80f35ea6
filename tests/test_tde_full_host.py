"""The host side of the full term scores (abnet3_amd/tde.py: evaluate_full) without a GPU: the worked example number for
number, the module against the restatement (tests/tde_full_np.py) on synthetic corpora with a word alignment and speakers --
the histogram of the launch replaced by the restated one, everything else the module's --, |S| by counting against the double
loop, the edge cases of snapping, the abns_ ledger of include/abnet3_hip_next.h and the refusals of abns_edit_cluster_hist
that need no launch."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tde_full_np as full_np  # noqa: E402
import tde_np  # noqa: E402
from conftest import ROOT  # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'abnet3_hip_next.h')
NAMES = {'abns_edit_hist_max_len', 'abns_edit_cluster_hist_ws_bytes', 'abns_edit_cluster_hist'}


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def alignment_of(lines):
    from abnet3_amd import tde
    parts = [line.split() for line in lines if line.strip()]
    return tde.make_alignment([p[0] for p in parts], [float(p[1]) for p in parts], [float(p[2]) for p in parts], [p[3] for p in parts])


def module_scores(lines, clusters, ignore, word_lines=None, speakers=None, ignore_words=None):
    """evaluate_full with the launch replaced by the restated histogram of the MODULE's transcriptions: (scores, prepared)."""
    from abnet3_amd import tde
    ev = tde.TermEvaluator(alignment_of(lines), ignore=ignore)
    prepared = ev.prepare_full(clusters, speakers=speakers)
    s = prepared[1]
    trans = [s.table[o:o + n].tolist() for o, n in zip(s.tok_off, s.tok_n)]
    hist, n_pairs, n_skipped = full_np.histogram(prepared[0], trans, prepared[6])
    words = None if word_lines is None else alignment_of(word_lines)
    return ev.finish_full(prepared, hist, n_pairs, n_skipped, words, ignore_words), prepared


def same(a, b):
    return a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b))


def assert_scores_equal(got, ref):
    for name in got._fields:
        if name == 'hist':
            assert got.hist.dtype == np.int64 and np.array_equal(got.hist, ref['hist'])
        elif name in ('token', 'type', 'boundary', 'grouping'):
            assert (getattr(got, name) is None) == (ref[name] is None), name
            assert getattr(got, name) is None or tuple(getattr(got, name)) == tuple(ref[name]), (name, getattr(got, name), ref[name])
        else:
            assert same(getattr(got, name), ref[name]), (name, getattr(got, name), ref[name])


# ---- the worked example -------------------------------------------------------------------------------------------------
PHONES = ['f 0.0 0.1 a', 'f 0.1 0.2 b', 'f 0.2 0.3 SIL', 'f 0.3 0.4 c', 'f 0.4 0.5 a', 'f 0.5 0.6 b']
WORDS = ['f 0 0.2 x', 'f 0.3 0.4 y', 'f 0.4 0.6 x']
CLUSTERS = [[('f', 0.0, 0.2), ('f', 0.4, 0.6)], [('f', 0.29, 0.5)]]


def test_the_worked_example_number_for_number():
    from abnet3_amd import tde
    got, prepared = module_scores(PHONES, CLUSTERS, ('SIL',), WORDS)
    s = prepared[1]
    a = alignment_of(PHONES)
    ids = a.symbols
    assert s.lo.tolist() == [0, 4, 3] and s.hi.tolist() == [1, 5, 4] and s.file.tolist() == [0, 0, 0]     # the third token: rows 3 .. 4, "c a"
    assert s.table.tolist() == [ids['a'], ids['b'], ids['a'], ids['b'], ids['c'], ids['a']]
    assert got.token[:2] == (2 / 3, 2 / 3) and got.token == full_np.prf(2, 3, 3) and abs(got.token[2] - 2 / 3) < 1e-15
    assert got.type == (1 / 2, 1 / 2, 1 / 2)
    assert got.boundary[:2] == (5 / 6, 5 / 5) and got.boundary[2] == 2 * (5 / 6) / (5 / 6 + 1)
    assert got.grouping == (1.0, 1.0, 1.0)
    assert got.hist.shape == (2, 3, 3) and got.hist[0][0][2] == 1 and got.hist.sum() == 1
    assert got.ned == 0.0 and got.ned_within == 0.0 and math.isnan(got.ned_across)
    assert (got.n_pairs, got.n_skipped, got.n_same) == (1, 0, 1)
    assert (got.n_clusters, got.n_tokens, got.n_empty, got.n_gold, got.n_gold_empty) == (2, 3, 0, 3, 0)
    assert got.coverage == 1.0
    files, symbols = tde_np.parse_alignment(PHONES)
    assert_scores_equal(got, full_np.evaluate_full(CLUSTERS, files, symbols, ('SIL',), tde_np.parse_alignment(WORDS)[0]))
    gold = tde.gold_words(alignment_of(WORDS), a, ('SIL',))
    assert gold.spans == {(0, 0, 1), (0, 3, 3), (0, 4, 5)} and gold.boundaries == {(0, 0), (0, 2), (0, 3), (0, 4), (0, 6)}
    assert gold.lexicon == {(ids['a'], ids['b']), (ids['c'],)}
    line = tde.full_summary(got)
    assert line.startswith('NED 0.0000 (within 0.0000, across nan) coverage 1.0000 token P 0.6667 R 0.6667 F 0.6667 type P 0.5000')
    assert line.endswith('(2 clusters, 3 tokens, 0 empty, 3 gold words, 0 empty, 1 pairs, 0 skipped, 1 same-type pairs)')


# ---- against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_the_module_equals_the_restatement_on_synthetic_corpora(seed):
    lines, clusters, ignore = tde_np.synthetic(seed=seed, n_files=8 if seed else 20, n_clusters=25 if seed else 60)
    word_lines, clusters = full_np.synthetic_words(lines, clusters, seed)
    files, symbols = tde_np.parse_alignment(lines)
    word_files = tde_np.parse_alignment(word_lines)[0]
    speakers = full_np.speakers_of(files)
    ref = full_np.evaluate_full(clusters, files, symbols, ignore, word_files, None, speakers)
    got, prepared = module_scores(lines, clusters, ignore, word_lines, speakers)
    s = prepared[1]
    flat = [t for c in clusters for t in c]
    # the module's snapping is the restatement's, token for token (file numbers are the sorted names' places)
    names = sorted(files)
    for k, t in enumerate(flat):
        span, seq = full_np.snap(t, files, symbols, ignore)
        assert s.table[s.tok_off[k]:s.tok_off[k] + s.tok_n[k]].tolist() == seq
        assert (span is None and (s.file[k], s.lo[k], s.hi[k]) == (-1, -1, -1)) or span == (names[s.file[k]], s.lo[k], s.hi[k])
    assert_scores_equal(got, ref)
    # the corpus exercises what it is for
    assert ref['n_empty'] > 0 and ref['n_gold_empty'] > 0 and ref['n_skipped'] >= 0 and ref['n_same'] > 0
    assert 0 < ref['token'][0] < 1 and 0 < ref['type'][1] < 1 and 0 < ref['boundary'][0] < 1 and 0 < ref['grouping'][0] < 1
    assert ref['hist'][0].sum() > 0 and ref['hist'][1].sum() > 0 and 0 < ref['ned_within'] <= 1 and 0 < ref['ned_across'] <= 1
    # without words the three triples are None and the rest stays; without speakers everything is "within"
    bare, _ = module_scores(lines, clusters, ignore)
    assert_scores_equal(bare, full_np.evaluate_full(clusters, files, symbols, ignore))
    assert bare.token is None and bare.type is None and bare.boundary is None and bare.grouping == got.grouping
    assert bare.ned == got.ned == bare.ned_within and math.isnan(bare.ned_across) and bare.hist[1].sum() == 0
    assert np.array_equal(bare.hist[0], got.hist[0] + got.hist[1])
    # ignore_words: another set of ignored words than `ignore`
    other, _ = module_scores(lines, clusters, ignore, word_lines, speakers, ignore_words=('w3', 'w4'))
    assert_scores_equal(other, full_np.evaluate_full(clusters, files, symbols, ignore, word_files, ('w3', 'w4'), speakers))
    assert other.n_gold != got.n_gold


def test_ned_from_the_histogram_against_the_mean_over_pairs():
    """evaluate().ned is np.mean of float64 quotients (pairwise summation: error <= (log2 n + 2) 2^-53 relative, 4.7e-15 for
    n < 2^40); ned_from_hist is the exactly rounded rational: the two differ by at most 1e-13 ned."""
    from abnet3_amd import tde
    for seed in (0, 1):
        lines, clusters, ignore = tde_np.synthetic(seed=seed)
        files, symbols = tde_np.parse_alignment(lines)
        ref = tde_np.evaluate(clusters, files, symbols, ignore)
        trans = tde_np.transcribe([t for c in clusters for t in c], files, symbols, ignore)[0]
        hist, n_pairs, n_skipped = full_np.histogram(clusters, trans)
        assert (n_pairs, n_skipped) == (ref['n_pairs'], ref['n_skipped']) and hist.sum() == len(ref['dist'])
        mean = tde.ned(ref['dist'], ref['max_len'])
        assert mean == ref['ned'] and abs(tde.ned_from_hist(hist) - mean) <= 1e-13 * mean
        assert tde.ned_from_hist(hist) == full_np.ned_of(hist)
    assert math.isnan(tde.ned_from_hist(np.zeros((2, 2, 2), dtype=np.int64)))
    one = np.zeros((2, 4, 4), dtype=np.int64)
    one[0][1][3], one[1][2][3] = 2, 1
    assert tde.ned_from_hist(one) == float(np.float64(4) / np.float64(9)) and tde.ned_from_hist(one[1:2]) == 2 / 3


def test_the_batched_restatement_of_the_distance_and_the_table_histogram():
    """tests/test_gpu_tde_full.py takes its reference from table_histogram: here against the plain loops."""
    rng = np.random.default_rng(1)
    for la, lb in ((0, 3), (3, 0), (5, 5), (7, 2), (1, 9), (0, 0)):
        A, B = rng.integers(0, 3, (20, la)), rng.integers(0, 3, (20, lb))
        assert full_np.levenshtein_many(A, B).tolist() == [tde_np.levenshtein(a.tolist(), b.tolist()) for a, b in zip(A, B)]
    t = full_np.token_table(rng, [1, 4, 0, 7, 2], [0, 1, 2, 5], 3, p_overlap=0.5)
    seqs = [t['table'][o:o + n].tolist() for o, n in zip(t['tok_off'], t['tok_n'])]
    clusters = [[(int(t['tok_file'][k]), float(t['tok_on'][k]), float(t['tok_end'][k])) for k in range(a, b)]
                for a, b in zip(t['cl_first'][:-1], t['cl_first'][1:])]
    hist, n_pairs, n_skipped = full_np.histogram(clusters, seqs, t['groups'].tolist())
    got = full_np.table_histogram(t)
    assert np.array_equal(got[0], hist) and got[1:] == (n_pairs, n_skipped) and 0 < n_skipped and n_pairs < 1 + 6 + 21
    assert t['cl_first'].tolist() == [0, 1, 5, 5, 12, 14] and t['tok_off'].dtype == np.int64 and t['tok_on'].dtype == np.float64


# ---- |S| by counting -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_same_type_pairs_by_counting_equals_the_double_loop(seed):
    """Few types, few files, onsets on a coarse grid (ties), one token in six without length, so that same-file overlapping
    tokens of one type, nested ones and zero-length ones on another token's onset or end all occur."""
    from abnet3_amd import tde
    rng = np.random.default_rng(seed)
    T = 150
    types = [[], [1], [1, 2], [2, 1], [3]]
    seqs = [types[int(rng.integers(0, len(types)))] for _ in range(T)]
    f = rng.integers(0, 3, T).astype(np.int32)
    on = rng.integers(0, 12, T) * 0.25
    end = on + np.where(rng.random(T) < 1 / 6, 0.0, rng.integers(1, 6, T) * 0.25)
    tok_n = np.array([len(q) for q in seqs], dtype=np.int32)
    snapped = tde.Snapped(np.array([x for q in seqs for x in q], dtype=np.int32), np.cumsum(tok_n, dtype=np.int64) - tok_n, tok_n, None, None, None)
    flat = [(int(f[k]), float(on[k]), float(end[k])) for k in range(T)]
    want = full_np.same_type_pairs(flat, seqs)
    overlapping = sum(1 for i in range(T) for j in range(i + 1, T) if seqs[i] and seqs[i] == seqs[j] and full_np.overlap(flat[i], flat[j]))
    zero = sum(1 for i in range(T) if seqs[i] and end[i] == on[i])
    assert overlapping > 20 and zero > 5 and want > 0
    assert tde.same_type_pairs(snapped, f, on, end) == want
    assert tde.same_type_pairs(tde.Snapped(np.zeros(0, np.int32), np.zeros(3, np.int64), np.zeros(3, np.int32), None, None, None), f[:3], on[:3], end[:3]) == 0


# ---- the edges of snapping ----------------------------------------------------------------------------------------------
def test_a_token_that_straddles_an_ignored_phone_and_a_word_without_a_phone():
    from abnet3_amd import tde
    a = alignment_of(PHONES)
    s = tde.snap_tokens([('f', 0.1, 0.4), ('f', 0.2, 0.3), ('f', 0.25, 0.26)], a, ('SIL',))
    assert (s.lo[0], s.hi[0]) == (1, 3) and s.table[:2].tolist() == [a.symbols['b'], a.symbols['c']] and s.tok_n.tolist() == [2, 0, 0]
    assert s.lo[1:].tolist() == [-1, -1] and s.file.tolist() == [0, -1, -1]                # nothing but silence; 10 ms of it
    kept = tde.snap_tokens([('f', 0.1, 0.4)], a)                                            # nothing ignored: the same span, three phones
    assert (kept.lo[0], kept.hi[0], kept.tok_n[0]) == (1, 3, 3)
    words = ['f 0.0 0.2 x', 'f 0.2 0.3 SIL', 'f 0.2 0.3 hum', 'f 0.3 0.305 y', 'f 0.4 0.6 x']
    gold = tde.gold_words(alignment_of(words), a, ('SIL',))
    assert (gold.n_gold, gold.n_gold_empty) == (4, 2) and gold.spans == {(0, 0, 1), (0, 4, 5)}      # 'hum' covers only silence, 'y' 5 ms of c
    assert len(gold.lexicon) == 1 and gold.boundaries == {(0, 0), (0, 2), (0, 4), (0, 6)}
    files, symbols = tde_np.parse_alignment(PHONES)
    ref = full_np.gold(tde_np.parse_alignment(words)[0], files, symbols, ('SIL',))
    assert (ref['n_gold'], ref['n_gold_empty'], len(ref['spans']), len(ref['lexicon'])) == (4, 2, 2, 1)
    with pytest.raises(ValueError, match='alignment does not hold'):
        tde.gold_words(alignment_of(['g 0 1 x']), a)


def test_clusters_without_a_pair_and_a_span_in_two_clusters():
    single = [[('f', 0.0, 0.2)], [('f', 0.4, 0.6)], []]
    got, _ = module_scores(PHONES, single, ('SIL',), WORDS)
    assert math.isnan(got.ned) and math.isnan(got.ned_within) and got.grouping == (0.0, 0.0, 0.0)
    assert (got.n_pairs, got.n_skipped, got.n_same, got.n_clusters, got.n_tokens) == (0, 0, 1, 3, 2) and got.hist.sum() == 0
    assert got.token == (1.0, 2 / 3, 2.0 * (2 / 3) / (1.0 + 2 / 3))
    none, _ = module_scores(PHONES, [], ('SIL',), WORDS)
    assert none.token == (0.0, 0.0, 0.0) and none.type == (0.0, 0.0, 0.0) and none.boundary == (0.0, 0.0, 0.0) and none.n_tokens == 0
    assert none.hist.shape == (2, 2, 2) and none.coverage == 0.0
    # the same interval in two clusters (and a second interval that snaps to the same span) counts once in F
    twice = [[('f', 0.0, 0.2), ('f', 0.4, 0.6)], [('f', 0.0, 0.2), ('f', 0.005, 0.21), ('f', 0.3, 0.4)]]
    got, prepared = module_scores(PHONES, twice, ('SIL',), WORDS)
    assert prepared[1].lo.tolist() == [0, 4, 0, 0, 3] and got.n_tokens == 5
    assert got.token == (1.0, 1.0, 1.0) and got.boundary[:2] == (1.0, 1.0) and got.type == (1.0, 1.0, 1.0)
    files, symbols = tde_np.parse_alignment(PHONES)
    assert_scores_equal(got, full_np.evaluate_full(twice, files, symbols, ('SIL',), tde_np.parse_alignment(WORDS)[0]))
    assert got.n_pairs == 3 and got.n_same == 3           # four tokens "a b": six pairs, three of them overlap in time


def test_speakers_as_a_mapping_and_as_a_callable():
    from abnet3_amd import tde
    files = ['s1_a', 's2_b', b's1_c', 's2_b']
    assert tde.speaker_groups(files, lambda f: f[:2]).tolist() == [0, 1, 0, 1]
    assert tde.speaker_groups(files, {'s1_a': 'x', 's2_b': 'y', 's1_c': 'x'}).dtype == np.int32
    with pytest.raises(ValueError, match='no speaker'):
        tde.speaker_groups(files, {'s1_a': 'x'})


def test_the_command_line_knows_the_full_route(tmp_path):
    from abnet3_amd import tde
    with pytest.raises(SystemExit):
        tde.main(['x.classes', 'phones.txt', '--words', 'w.txt'])                            # --words belongs to --full
    with pytest.raises(SystemExit):
        tde.main(['phones.txt', '--full'])
    (tmp_path / 'spk.txt').write_text('f1 a\n\nf2 b\n')
    assert tde.read_speakers(str(tmp_path / 'spk.txt')) == {'f1': 'a', 'f2': 'b'}
    assert 'not computed' not in tde.__doc__ and 'evaluate_full' in tde.__doc__


# ---- the ledger and the refusals that need no launch --------------------------------------------------------------------
def declared(prefix='abns_'):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, text))


def test_eval_symbols_are_the_headers_section_and_the_librarys_exports(lib):
    import subprocess
    from abnet3_amd import _lib, build
    assert declared() == set(_lib.EVAL_SYMBOLS) == NAMES
    others = set(_lib.SYMBOLS)
    for k in vars(_lib):
        if k.startswith('NEXT') and k.endswith('_SYMBOLS'):
            others |= set(getattr(_lib, k))
    assert not NAMES & others and not [k for k in vars(_lib) if k.startswith('NEXT8')]
    nm = '/opt/rocm/lib/llvm/bin/llvm-nm' if os.path.exists('/opt/rocm/lib/llvm/bin/llvm-nm') else 'nm'
    out = subprocess.run([nm, '-D', '--defined-only', lib._name], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {p[2] for p in (line.split() for line in out.splitlines()) if len(p) >= 3 and p[1] in 'TtWw' and p[2].startswith('abns_')}
    assert exported == NAMES
    for name, (res, args) in _lib.EVAL_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert len(_lib.EVAL_SYMBOLS['abns_edit_cluster_hist'][1]) == 17
    assert lib.abn_abi_version() == 20 and _lib.ABI_VERSION == 20
    head = open(HEADER).read()
    top = head[:head.index('#ifndef')]
    assert 'abns_' in top and 'EVAL_SYMBOLS' in top
    assert 'edit_hist.hip' in build.SOURCES and 'edit_hist.hip' not in build.STRICT_FP


def test_queries_and_refusals_before_any_launch(lib):
    from abnet3_amd import _lib
    assert lib.abns_edit_hist_max_len() == lib.abn_edit_max_short() == 256
    ws = lib.abns_edit_cluster_hist_ws_bytes
    assert ws(-1, 1, 1) == -1 and b'abns_edit_cluster_hist_ws_bytes' in lib.abn_last_error()
    assert ws(1, -1, 1) == -1 and ws(1, 1, -1) == -1 and ws(1 << 31, 1, 1) == -1
    # one record per cluster, nothing per pair or per token
    assert ws(150000, 1000, 10 ** 8) == ws(150000, 1000, 0) == ws(2, 1000, 1) and 0 < ws(150000, 1000, 10 ** 8) <= 16 + 20 * 1000 + 8 + 256
    assert ws(0, 0, 0) > 0 and ws(5, 3, 4) % 256 == 0
    p = 256                                                                          # a non-null, aligned address that is never read
    first = np.array([0, 2, 2, 5], dtype=np.int64)
    ok = dict(sym=p, rows=40, tok_off=p, tok_n=p, tok_file=p, tok_on=p, tok_end=p, tok_group=0, n_tokens=5, cl_first=first.ctypes.data,
              n_clusters=3, M=12, hist=p, counts=p, ws=p, ws_bytes=ws(5, 3, 4), stream=0)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.abns_edit_cluster_hist(*[a[k] for k in ok])
    for M in (0, -1, 257):
        assert call(M=M) == _lib.E_ARG and b'M must lie in 1 .. 256' in lib.abn_last_error()
    for name in ('rows', 'n_tokens', 'n_clusters', 'ws_bytes'):
        assert call(**{name: -1}) == _lib.E_ARG, name
    assert b'negative' in lib.abn_last_error()
    for name in ('sym', 'tok_off', 'tok_n', 'tok_file', 'tok_on', 'tok_end', 'cl_first', 'hist', 'counts', 'ws'):
        assert call(**{name: 0}) == _lib.E_ARG, name
        assert b'null' in lib.abn_last_error()
    assert call(n_tokens=1 << 31) == _lib.E_ARG
    assert call(ws=p + 8) == _lib.E_ARG and b'aligned' in lib.abn_last_error()
    for bad in ([0, 3, 2, 5], [1, 2, 2, 5], [0, 2, 2, 4], [0, 2, 2, 6], [0, 6, 5, 5]):
        arr = np.array(bad, dtype=np.int64)
        assert call(cl_first=arr.ctypes.data) == _lib.E_ARG, bad
        assert b'cl_first' in lib.abn_last_error()
    assert call(ws_bytes=ws(5, 3, 4) - 1) == _lib.E_WORKSPACE and b'workspace' in lib.abn_last_error()


def test_cluster_histogram_refuses_on_the_host_what_needs_no_device(lib):
    """The checks that come before any upload: host columns of the wrong kind or rank (the device-side contract is
    tests/test_gpu_tde_full_contract.py's)."""
    from abnet3_amd import tde
    t = full_np.token_table(np.random.default_rng(0), [2, 3], [1, 2, 3], 4)
    args = [t[k] for k in ('table', 'tok_off', 'tok_n', 'tok_file', 'tok_on', 'tok_end', 'cl_first')]
    for k, bad in ((2, t['tok_n'].astype(np.float64)), (2, t['tok_n'][None]), (2, t['tok_n'].astype(np.int64) + (1 << 40))):
        a = list(args)
        a[k] = bad
        with pytest.raises(ValueError, match='cluster_histogram: tok_n'):
            tde.cluster_histogram(*a)
