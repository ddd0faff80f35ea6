"""The term-discovery prefilter without a GPU: the numpy restatement (tests/prefilter_np.py) on hand-made dot plots whose
answers can be written down and against a cell-by-cell loop from the definition, lsh_planes, the new entry points'
argument checks before any launch, the header, and TermDiscoverer's mask logic on a stubbed prefilter."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefilter_np  # noqa: E402
import terms_np  # noqa: E402


@pytest.mark.parametrize('n,m,span', [(10, 7, 4), (7, 10, 4), (5, 9, 64), (9, 5, 64), (6, 6, 6), (1, 8, 3), (8, 1, 3), (12, 12, 1)])
def test_an_all_hit_matrix(n, m, span):
    """run(i, j) = min(span, i + 1, j + 1): the largest is B = min(span, n, m), first reached on diagonal B - m (row
    B - 1, the last column)."""
    B = min(span, n, m)
    for dilate in (0, 1, 8):
        assert prefilter_np.runs(np.ones((n, m), dtype=bool), span, dilate) == (B, B - m, B - 1)
    assert prefilter_np.runs(np.zeros((n, m), dtype=bool), span) == (0, 0, -1)
    assert prefilter_np.runs(np.zeros((0, m), dtype=bool), span) == (0, 0, -1)
    assert prefilter_np.runs(np.zeros((n, 0), dtype=bool), span) == (0, 0, -1)


def test_a_single_planted_run():
    hit = np.zeros((40, 30), dtype=bool)
    for s in range(12):
        hit[20 + s, 5 + s] = True                      # diagonal 15, rows 20 .. 31
    hit[3, 9] = hit[30, 2] = True                       # stray hits
    assert prefilter_np.runs(hit, 32) == (12, 15, 31)
    assert prefilter_np.runs(hit, 8) == (8, 15, 27)    # the window is full after 8 rows: the first full one wins
    assert prefilter_np.runs(hit, 1) == (1, -6, 3)     # single hits tie: the smallest diagonal (3 - 9)
    hit[25, 10] = False                                 # a gap inside the run: 11 of the 12 cells
    assert prefilter_np.runs(hit, 32) == (11, 15, 31)
    assert prefilter_np.runs(hit, 5) == (5, 15, 24)


def test_a_run_that_steps_sideways_needs_dilation():
    hit = np.zeros((30, 30), dtype=bool)
    for s in range(8):
        hit[4 + s, 6 + s] = True                        # diagonal -2 ...
    for s in range(8, 16):
        hit[4 + s, 7 + s] = True                        # ... then one column to the right: diagonal -3
    assert prefilter_np.runs(hit, 32, 0) == (8, -3, 19)            # two runs of 8: the smaller diagonal
    best, diag, end1 = prefilter_np.runs(hit, 32, 1)
    assert best == 16 and end1 == 19 and diag in (-3, -2)
    assert (best, diag, end1) == (16, -3, 19)
    assert prefilter_np.runs(hit, 32, 1) == prefilter_np.runs_slow(hit, 32, 1)
    # the dilation does not reach outside the matrix and counts a cell once
    edge = np.zeros((3, 3), dtype=bool)
    edge[:, 0] = True
    assert prefilter_np.runs(edge, 3, 1) == (2, 0, 1) and prefilter_np.runs_slow(edge, 3, 1) == (2, 0, 1)


def test_the_restatement_equals_a_cell_by_cell_loop():
    rng = np.random.default_rng(3)
    some = 0
    for trial in range(60):
        n, m = int(rng.integers(1, 15)), int(rng.integers(1, 15))
        hit = rng.random((n, m)) < (0.15, 0.5, 0.9)[trial % 3]
        for span in (1, 2, 5, 64):
            for dilate in (0, 1, 3):
                got = prefilter_np.runs(hit, span, dilate)
                assert got == prefilter_np.runs_slow(hit, span, dilate), (trial, span, dilate)
                some += got[0] > 1
    assert some > 200


def one_table(rows=120, words=1):
    """A signature table in which row r equals row r - 40 for r in 40 .. 59 and nothing else repeats."""
    sig = (np.arange(rows * words, dtype=np.uint32) * np.uint32(2654435761)).reshape(rows, words)
    sig[40:60] = sig[0:20]
    return sig, np.ones(rows, np.uint8)


@pytest.mark.parametrize('w0', [0, 7, 30])
def test_exclude_removes_the_band_of_a_self_pair(w0):
    """The whole table against a window of itself that starts at w0: without exclusion the main diagonal (table row
    against the same table row: i - j = w0) wins; with it the planted repeat at distance 40."""
    sig, live = one_table()
    n, m = 120, 120 - w0
    args = (sig, live, [0], [n], sig, live, [w0], [m])
    assert [int(x[0]) for x in prefilter_np.diag_hits(*args, 0, span=32)] == [32, w0, w0 + 31]
    for exclude in (1, 20, 40):
        # table rows 0 .. 19 (i) against their copies, table rows 40 .. 59 (j + w0): diagonal w0 - 40, rows 0 .. 19; the
        # mirror image (i in 40 .. 59, j + w0 in 0 .. 19, diagonal w0 + 40) is as long at most and loses the tie
        assert [int(x[0]) for x in prefilter_np.diag_hits(*args, 0, span=32, exclude=exclude)] == [20, w0 - 40, 19]
        i, j = np.nonzero(prefilter_np.hit_matrix(sig, live, 0, n, sig, live, w0, m, 0, exclude))
        assert (np.abs(i - (j + w0)) == 40).all() and len(i) == 20 + max(0, 20 - w0)
    # beyond the repeat's distance nothing is left
    assert [int(x[0]) for x in prefilter_np.diag_hits(*args, 0, span=32, exclude=41)] == [0, 0, -1]
    # dead rows do not hit
    dead = live.copy()
    dead[45] = 0
    b, d, e = (int(x[0]) for x in prefilter_np.diag_hits(sig, dead, [0], [n], sig, dead, [w0], [m], 0, span=32, exclude=1))
    assert (b, d) == (19, w0 - 40)


def test_refusals_of_the_restatement():
    sig, live = one_table()
    off1, n1 = [0, 0, 100, 0, -1, 0], [10, -1, 30, 10, 5, 10]
    off2, n2 = [0, 0, 0, 119, 0, 0], [513, 5, 5, 2, 5, 0]
    b, d, e = prefilter_np.diag_hits(sig, live, off1, n1, sig, live, off2, n2, 32)
    assert b.tolist() == [-1, -1, -1, -1, -1, 0] and d.tolist() == [0] * 6 and e.tolist() == [-1] * 6
    assert prefilter_np.keep(np.array([-1, 0, 23, 24, 32]), 24).tolist() == [False, False, False, True, True]


def test_signatures_of_the_restatement():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((9, 7)).astype(np.float32)
    x[2] = 0.0
    x[4, 3] = np.nan
    x[6, 0] = np.inf
    x[7, 6] = -np.inf
    pl = prefilter_np.planes(7, 96, seed=2)
    sig, live, decided = prefilter_np.signatures(x, pl)
    assert live.tolist() == [1, 1, 0, 1, 0, 1, 0, 0, 1] and sig.dtype == np.uint32 and sig.shape == (9, 3)
    assert not sig[[2, 4, 6, 7]].any()
    bits = prefilter_np.unpack(sig, 96)
    assert np.array_equal(bits[0], (x[0].astype(np.float64) @ pl.astype(np.float64).T > 0).astype(np.uint8))
    assert np.array_equal(prefilter_np.pack(bits), sig)
    assert (sig[0, 0] >> np.uint32(5)) & 1 == int(np.dot(x[0].astype(np.float64), pl[5].astype(np.float64)) > 0)     # bit 5 of word 0
    assert decided[[0, 1, 3, 5, 8]].mean() > 0.99
    # opposite frames: every bit differs; the same frame scaled: none does
    y = np.stack([x[0], -x[0], 3.0 * x[0]]).astype(np.float32)
    s, _, _ = prefilter_np.signatures(y, pl)
    assert prefilter_np.popcount(s[0] ^ s[1]).sum() == 96 and prefilter_np.popcount(s[0] ^ s[2]).sum() == 0


def test_lsh_planes_are_reproducible():
    from abnet3_amd import prefilter
    import abnet3_amd
    a = prefilter.lsh_planes(40, 64, seed=1)
    assert a.dtype == np.float32 and a.shape == (64, 40)
    assert np.array_equal(a, np.random.default_rng(1).standard_normal((64, 40)).astype(np.float32))
    assert np.array_equal(a, prefilter.lsh_planes(40, 64, seed=1)) and np.array_equal(a, prefilter_np.planes(40, 64, 1))
    assert not np.array_equal(a, prefilter.lsh_planes(40, 64, seed=2))
    assert prefilter.lsh_planes(3).shape == (64, 3)
    assert abnet3_amd.lsh_planes is prefilter.lsh_planes and abnet3_amd.TermPrefilter is prefilter.TermPrefilter
    assert abnet3_amd.lsh_signatures is prefilter.lsh_signatures and abnet3_amd.diag_hits_batch is prefilter.diag_hits_batch
    for bits in (0, 16, 33, 288):
        with pytest.raises(ValueError, match='bits'):
            prefilter.lsh_planes(40, bits)
    with pytest.raises(ValueError, match='D must'):
        prefilter.lsh_planes(4097)
    p = prefilter.TermPrefilter()
    assert (p.bits, p.max_hamming, p.span, p.dilate, p.min_hits) == (64, 16, 32, 1, 24)
    p = prefilter.TermPrefilter(bits=128, span=20)
    assert (p.max_hamming, p.min_hits) == (32, 15)
    assert 'untuned' in prefilter.TermPrefilter.__doc__ and 'tuned' in prefilter.__doc__
    for bad in (dict(bits=48), dict(span=0), dict(span=65), dict(dilate=9), dict(dilate=-1), dict(max_hamming=65), dict(min_hits=-1)):
        with pytest.raises(ValueError):
            prefilter.TermPrefilter(**bad)


def test_header_binding_and_argument_checks_before_any_launch():
    from abnet3_amd import _lib, build, prefilter
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read(), flags=re.S)
    for name in ('abn_lsh_signatures', 'abn_lsh_diag_hits_batched'):
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.SYMBOLS, name
    assert len(_lib.SYMBOLS['abn_lsh_signatures'][1]) == 8 and len(_lib.SYMBOLS['abn_lsh_diag_hits_batched'][1]) == 20
    assert re.search(r'^#define ABN_ABI_VERSION 20$', text, flags=re.M) and _lib.ABI_VERSION == 20
    for name, value in (('MAX_BITS', prefilter.MAX_BITS), ('MAX_D', prefilter.MAX_D), ('MAX_SPAN', prefilter.MAX_SPAN),
                        ('MAX_DILATE', prefilter.MAX_DILATE), ('GRID_BLOCKS', prefilter.GRID_BLOCKS)):
        assert re.search(r'^#define ABN_LSH_%s %d$' % (name, value), text, flags=re.M), name
    assert 'lsh.hip' in build.SOURCES
    build.build()
    lib = _lib.load()
    assert lib.abn_abi_version() == 20
    a = 0x1000
    # abn_lsh_signatures(table, rows, D, planes, bits, sig, live, stream)
    assert lib.abn_lsh_signatures(None, 4, 40, None, 64, None, None, None) == _lib.E_ARG and b'null' in lib.abn_last_error()
    for ptrs in ((None, a, a, a), (a, None, a, a), (a, a, None, a), (a, a, a, None)):
        assert lib.abn_lsh_signatures(ptrs[0], 4, 40, ptrs[1], 64, ptrs[2], ptrs[3], None) == _lib.E_ARG
        assert b'null' in lib.abn_last_error()
    for bits in (0, 16, 31, 33, 48, 257, 288, -32):
        assert lib.abn_lsh_signatures(a, 4, 40, a, bits, a, a, None) == _lib.E_ARG and b'bits' in lib.abn_last_error(), bits
    for D in (0, -1, 4097):
        assert lib.abn_lsh_signatures(a, 4, D, a, 64, a, a, None) == _lib.E_ARG and b'D must' in lib.abn_last_error(), D
    assert lib.abn_lsh_signatures(a, -1, 40, a, 64, a, a, None) == _lib.E_ARG and b'rows' in lib.abn_last_error()
    assert lib.abn_lsh_signatures(None, 0, 40, None, 64, None, None, None) == 0                 # no rows: no launch
    # abn_lsh_diag_hits_batched(sig1, live1, rows1, sig2, live2, rows2, off1, n1, off2, n2, P, words, max_hamming, span, dilate,
    #                           exclude, best, diag, end1, stream)

    def call(P=1, words=2, max_hamming=16, span=32, dilate=1, exclude=0, tables=(a, a, 8, a, a, 8), cols=(a, a, a, a), out=(a, a, a)):
        return lib.abn_lsh_diag_hits_batched(*(tables + cols + (P, words, max_hamming, span, dilate, exclude) + out + (None,)))
    for k in range(4):
        assert call(cols=tuple(None if c == k else a for c in range(4))) == _lib.E_ARG and b'null' in lib.abn_last_error()
    for k in range(3):
        assert call(out=tuple(None if c == k else a for c in range(3))) == _lib.E_ARG and b'null' in lib.abn_last_error()
    for k in (0, 1, 3, 4):
        t = [a, a, 8, a, a, 8]
        t[k] = None
        assert call(tables=tuple(t)) == _lib.E_ARG and b'null' in lib.abn_last_error()
    for words in (0, 9, -1):
        assert call(words=words) == _lib.E_ARG and b'words' in lib.abn_last_error()
    for mh in (-1, 65):
        assert call(max_hamming=mh) == _lib.E_ARG and b'max_hamming' in lib.abn_last_error()
    assert call(words=1, max_hamming=33) == _lib.E_ARG and b'max_hamming' in lib.abn_last_error()
    for span in (0, 65, -3):
        assert call(span=span) == _lib.E_ARG and b'span' in lib.abn_last_error()
    for dilate in (-1, 9):
        assert call(dilate=dilate) == _lib.E_ARG and b'dilate' in lib.abn_last_error()
    assert call(exclude=-1) == _lib.E_ARG and b'exclude' in lib.abn_last_error()
    for t in ((a, a, 8, 0x2000, a, 8), (a, a, 8, a, 0x2000, 8), (a, a, 8, a, a, 9)):
        assert call(exclude=3, tables=t) == _lib.E_ARG and b'one table' in lib.abn_last_error()
    assert call(P=-1) == _lib.E_ARG
    assert call(P=0, tables=(None, None, 0, None, None, 0), cols=(None,) * 4, out=(None,) * 3) == 0      # no pairs: no launch
    assert call(P=0, span=99) == _lib.E_ARG                                                                # ... but still checked


class FakeCorpus(object):
    def __init__(self, lengths):
        self.names = ['utt%d' % k for k in range(len(lengths))]
        self.length = dict(zip(self.names, lengths))
        self.offset = dict(zip(self.names, np.concatenate(([0], np.cumsum(lengths)[:-1])).tolist()))

    def _name(self, f):
        return f


def discoverer(lengths, prefilter=None):
    """A TermDiscoverer over utterances of the given lengths with its kernel stubbed: align() records the kernel pairs it
    is given and answers 'no match'."""
    from abnet3_amd import terms
    td = terms.TermDiscoverer.__new__(terms.TermDiscoverer)
    td.corpus, td.names = FakeCorpus(lengths), ['utt%d' % k for k in range(len(lengths))]
    td.window, td.theta, td.min_frames, td.max_distance, td.merge_overlap = 512, np.float32(0.25), 50, None, 0.5
    td.exclude, td.chunk_pairs, td.distance, td.prefilter = 50, 1 << 18, 'cosine', prefilter
    td.seen = []

    def align(kp):
        td.seen.append(list(kp))
        return tuple([np.zeros(len(kp))] + [np.zeros(len(kp), np.int32)] + [np.full(len(kp), -1, np.int32)] * 4)
    td.align = align
    return td


class StubPrefilter(object):
    def __init__(self, rule):
        self.rule, self.calls = rule, []

    def keep(self, discoverer, kp):
        self.calls.append((discoverer, list(kp)))
        self.best = np.array([self.rule(*q) for q in kp], dtype=np.int32)
        return self.best >= 10


def test_discover_without_a_prefilter_builds_the_same_kernel_pairs():
    lengths = [150, 0, 700, 1300, 180]
    want = terms_np.kernel_pairs(lengths, terms_np.all_pairs(5), 512)
    td = discoverer(lengths)
    assert td.discover() == ([], [])
    assert td.seen == [want] and len(want) == 24
    assert (td.n_kernel_pairs, td.n_aligned_pairs, td.prefilter_best) == (24, 24, None)
    td.discover(pairs=[('utt3', 'utt2'), ('utt0', 'utt3')])
    assert td.seen[1] == terms_np.kernel_pairs(lengths, [(3, 2), (0, 3)], 512) and td.n_kernel_pairs == td.n_aligned_pairs == 7


def test_discover_aligns_what_the_prefilter_keeps_in_order():
    lengths = [150, 0, 700, 1300, 180]
    want = terms_np.kernel_pairs(lengths, terms_np.all_pairs(5), 512)
    rule = lambda u, v, w0, wn: 10 if (u + v + w0 // 256) % 3 == 0 else 9
    kept = [q for q in want if rule(*q) >= 10]
    assert 0 < len(kept) < len(want)
    stub = StubPrefilter(rule)
    td = discoverer(lengths, prefilter=stub)                        # the constructor's prefilter
    td.discover()
    assert td.seen == [kept] and stub.calls == [(td, want)]
    assert (td.n_kernel_pairs, td.n_aligned_pairs) == (len(want), len(kept))
    assert td.prefilter_best.dtype == np.int32 and td.prefilter_best.tolist() == [rule(*q) for q in want]
    other = StubPrefilter(lambda u, v, w0, wn: 10 if u == v else 0)  # discover()'s argument wins
    td.discover(prefilter=other)
    assert td.seen[1] == [q for q in want if q[0] == q[1]] and len(stub.calls) == 1 and len(other.calls) == 1
    none = StubPrefilter(lambda *q: 0)
    td.discover(prefilter=none)
    assert td.seen[2] == [] and td.n_aligned_pairs == 0 and td.matches == [] and td.clusters == []

    class Short(object):
        def keep(self, discoverer, kp):
            return np.ones(len(kp) - 1, dtype=bool)
    with pytest.raises(ValueError, match='mask'):
        td.discover(prefilter=Short())


def test_the_command_line_takes_the_prefilter_options(capsys):
    from abnet3_amd import terms
    with pytest.raises(SystemExit):
        terms.main(['--help'])
    text = capsys.readouterr().out
    for opt in ('--prefilter', '--bits', '--max-hamming', '--span', '--dilate', '--min-hits', '--lsh-seed'):
        assert opt in text, opt


def test_the_end_to_end_parameters_keep_the_planted_windows():
    """The GPU test's corpus and parameters in numpy: 7 of the 18 kernel pairs are kept -- the windows that hold at
    least 50 frames of a planted copy, each with best = 32 -- and every other pair has best <= 17; every pair the
    brute-force run takes a match from is among them."""
    feats, _times, _planted = terms_np.planted_corpus()
    names = sorted(feats)
    lengths = [len(feats[k]) for k in names]
    base = np.concatenate(([0], np.cumsum(lengths)[:-1]))
    table = np.concatenate([feats[k] for k in names])
    sig, live, _ = prefilter_np.signatures(table, prefilter_np.planes(40, 64, seed=1))
    kp = terms_np.kernel_pairs(lengths, terms_np.all_pairs(len(names)), 512)
    best = prefilter_np.best_runs(sig, live, base, lengths, kp, 50, 16, 32, 0)
    mask = prefilter_np.keep(best, 24)
    assert len(kp) == 18 and int(mask.sum()) == 7
    assert (best[mask] == 32).all() and best[~mask].max() <= 17
    matches, _ = terms_np.discover(names, feats, 0.05)
    kept = {q[:3] for q, m in zip(kp, mask) if m}
    for m in matches:
        assert any(u == m[0] and v == m[3] and w0 <= m[4] and m[5] < w0 + 512 for u, v, w0 in kept), m
